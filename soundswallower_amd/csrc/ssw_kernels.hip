/*
 * ssw_kernels.hip -- gfx950 (MI355X, CDNA4) kernels for the SoundSwallower acoustic hot path
 * and the C ABI of include/ssw_amd.h on top of them.
 *
 * All arithmetic that the reference does in float32 is done here in float32 with one rounding
 * per operation (no FMA contraction: this file is built with -ffp-contract=off and carries the
 * pragma below), in the reference's operation order; everything else is int32.  Citations are
 * file:line in the SoundSwallower tree.
 *
 * One translation unit, split over .inc files for reading (device code first, inside one
 * anonymous namespace, then the host side):
 *   ssw_dev_common.inc   truncation, density, wave reductions, LDS-only barrier
 *   ssw_k1a_chain.inc    ptm_topn_chain_kernel (exact frame-sequential top-N: eval_topn + eval_cb,
 *                        src/ptm_mgau.c:86-225) and topn_exact_step, the exact step the scans'
 *                        in-wave pass shares
 *   ssw_scan_common.inc  what the two speculative top-N scans share, each piece once: FramesParams,
 *                        the packed codeword order, the sort of the four candidates, the 5th-key
 *                        bound and the proof test, the mask of unscanned codebooks, the helpers of
 *                        the exact in-wave pass (wave_frame_densities, topn_self_determined,
 *                        start_order, carried_order_of, the masked walk, ms_exact_step) and the
 *                        statement of what that pass, written in each scan, must do
 *   ssw_k1a_frames.inc   ptm_topn_frames_kernel (speculative history-free top-N on the vector
 *                        unit with a proof test per pair), gather_last_orders_kernel
 *   ssw_k1a_mfma.inc     ptm_topn_mfma_kernel: the same scan with its multiply-adds on the matrix
 *                        cores (keys from two-part binary16 operands, exact re-evaluation, proof
 *                        and in-wave pass as above): what every batch takes
 *   ssw_senone_lds.inc   no HIP, ahead of the namespace: the dynamic LDS of the senone kernels,
 *                        SenoneCarve / MsSenoneCarve / Active2Carve / ListedCarve / ContListedCarve,
 *                        and FpaPlanCarve of the default configuration's plan kernel -- the kernel
 *                        takes its pointers and the launcher its byte count from the same struct
 *   ssw_senone_common.inc the steps of the reference's senone scorers that several kernels
 *                        share, once: clamp_i16, fast_logadd / ms_logadd, the padded table fill,
 *                        ptm_norm_pack4, wave_codebook_norm, ptm_slot_score, ms_slot_score,
 *                        ms_quad_scores, ms_finish, final_score, wave_best_or_zero,
 *                        move_exact_count (src/ptm_mgau.c:271-400, src/ms_senone.c:314-362)
 *   ssw_k1b_senone.inc   ptm_senone_kernel (codebook_norm + senone_eval, src/ptm_mgau.c:264-403),
 *                        ptm_senone_frame_kernel (one frame, active sets), ms_senone_kernel
 *   ssw_k4_feat.inc      feat_1s_c_d_dd_kernel (batch CMN + 1s_c_d_dd, src/feat.c:271-326)
 *   ssw_align_common.inc the frame step that the 3-state alignment kernels with their HMMs in
 *                        registers share, once (hmm_vit_eval_3st_lr, a lane's constants and HMM,
 *                        score look-ahead, renormalisation, evaluate-and-keep, the waves' exchange
 *                        slots, phone_transition as a carry chain, hmm_enter, record_transitions),
 *                        src/state_align_search.c:57-175, src/hmm.c:124-161, :482-567
 *   ssw_k2_align.inc     viterbi_align_mw_kernel / _mwb_kernel / _win_kernel / _reg_kernel /
 *                        viterbi_align_kernel (state_align_search step/finish,
 *                        src/state_align_search.c:177-268): tokens, replay, window, LDS / HBM state
 *   ssw_k2_anytopo.inc   viterbi_align_any_kernel: the same search over HMMs of 1, 2, 4 or 5 states
 *                        (hmm_vit_eval_5st_lr, hmm_vit_eval_anytopo, src/hmm.c:166-304, :671-739)
 *   ssw_search_common.inc the decisions of the reference's fsg_search that the three K5 kernels
 *                        share, once (start rule, beams, phone and cross-word transitions, twins'
 *                        order, final exit, segment writer, score look-ahead); K9 uses its flags,
 *                        twins' order, entering-list record and entry scan, src/fsg_search.c:310-925
 *   ssw_k5_firstpass.inc first_pass_kernel (fsg_search start/step/finish over the linear
 *                        grammar's phone trees, HMMs in registers), first_pass_big_kernel (state in
 *                        an HBM workspace), first_pass_win_kernel (a sliding window over LDS rings)
 *   ssw_k6_compact.inc   compact score rows: the plan of a batch of alignments (which of an
 *                        utterance's states share a senone, where each score goes), gather
 *   ssw_k7_fpactive.inc  the first pass in the default configuration (compallsen = no) as a
 *                        batch: per-frame listed sets from the search's exported HMM sets, the
 *                        senone kernel over them, the comparison that proves a trajectory
 *   ssw_k8_fe.inc        the MFCC front end for whole utterances: fe_spectrum_kernel (pre-emphasis,
 *                        window, fe_fft_real, power and mel spectra, one wave per frame),
 *                        fe_noise_kernel (fe_remove_noise, one wave per utterance),
 *                        fe_cep_kernel (log, DCT-II or legacy transform, lifter),
 *                        src/fe_sigproc.c:219-738, src/fe_noise.c:111-327
 *   ssw_k8_fe_any.inc    the same for every configuration fe_init accepts: fe_spectrum_any_kernel
 *                        (alpha of any value, remove_dc with the reference's ordered sum),
 *                        fe_cep_any_kernel (any ncep, htk, logspec, smoothspec)
 *   ssw_k9_grammar.inc   grammar_search_kernel: K5's search over the phone trees of any word FSG,
 *                        null transitions folded into the states' entering lists
 *                        (fsg_search_start / _null_prop / _find_exit, src/fsg_search.c:543-924)
 *                        grammar_search_big_kernel: the same search from an HBM workspace, for
 *                        grammars beyond one workgroup (ssw_grammar_prepare_large)
 *   ssw_k10_semi.inc     the s2_semi scorer of single-codebook models: semi_density_kernel (every
 *                        density exactly, the frame's candidates), semi_chain_kernel (eval_topn and
 *                        eval_cb over them, one wave per utterance and stream), semi_senone_kernel
 *                        (mgau_norm + get_scores_8b_feat_all), src/s2_semi_mgau.c:68-202, :425-443
 *   ssw_k11_cont.inc     the ms scorer on continuous-density models (one codebook per senone):
 *                        cont_score_kernel (compute_dist + senone_eval, a lane per senone),
 *                        cont_norm_kernel (the frame's minimum), src/ms_gauden.c:349-432,
 *                        src/ms_senone.c:314-362, src/ms_mgau.c:299-321
 *                        cont_listed_kernel (compallsen = no: a group of lanes per LISTED senone
 *                        over the senone-major table, src/ms_mgau.c:322-365)
 *   ssw_cont_select.inc  compute_dist's selection, once: cont_insert (sequential) and
 *                        cont_select_rank (a density's slot as a count; a host program can
 *                        include it on its own)
 *   ssw_k12_feat.inc     dynamic features of every type feat_init_s3file accepts, with batch or
 *                        live CMN, varnorm, an LDA and a subvector gather: feat_stats_kernel /
 *                        feat_chain_kernel (the utterances' means and scales, live CMN's state)
 *                        and feat_tile_kernel (frame-parallel), src/feat.c:437-712, :977-1008,
 *                        src/cmn.c:159-224, src/cmn_live.c:60-134, src/lda.c:124-144
 *   ssw_vad_core.inc     the reference's voice activity detector, each step once, for this file
 *                        and for ssw_vad.c's host path alike: the resamplers to 8 kHz, the band
 *                        splits, LogOfEnergy, the Gaussians, the minimum tracker, GmmProbability
 *                        (src/common_audio/vad/, src/common_audio/signal_processing/)
 *   ssw_k13_vad.inc      vad_batch_kernel: vad_classify over a batch of streams, a lane per
 *                        stream, audio staged through LDS, every per-sample buffer in LDS
 *   ssw_feat_tiles.inc   host, no HIP: the tile table and tile size of ssw_feat_batch_ex
 *   ssw_ws_layout.inc    host, no HIP: align256 and WsLayout, the one layout of a device
 *                        workspace (256-byte-aligned offsets in call order, the uploaded pieces
 *                        staged by fill(); a host program can include it on its own)
 *   ssw_xcd_cut.inc      host, no HIP: xcd_cut, the matrix-core scan's (codebook x stream, tile
 *                        group) pairs cut into eight chunks of equal cost, one per XCD
 *   ssw_slot_layout.inc  host, no HIP: slot_layout (the senone kernels' slot order: by codebook,
 *                        every run of consecutive ids padded to whole quads), senone_shape (their
 *                        workgroups' shape) and the rule that chooses between the two layouts
 *   ssw_fp_shape.inc     host, no HIP: fp_shape, what one launch of the first pass takes (the
 *                        per-utterance LDS, HBM-workspace and history sizes, each formula once;
 *                        register / window / HBM / HBM-banded kernel, threads, LDS bytes)
 *   ssw_fpa_shape.inc    host, no HIP: fpa_shape, what one call of the default configuration's loop
 *                        takes (the exported sets' layout, the list capacity, the LDS of its two
 *                        per-frame kernels from their carves, the 156 KB refusal), the comparison's
 *                        slices and the policy of its rounds (one by one / the whole batch)
 *   ssw_active_set.inc   host, no HIP: the second pass's active set from the phone windows
 *                        (active_first_frames, ActiveSetBuilder) and a continuous model's bitmap
 *                        rows of it (cont_active_rows)
 *   ssw_host_model.inc   also the host side's three shared helpers, each holding one policy:
 *                        devbuf_reserve (the grow-only device buffer: no HIP call unless it
 *                        grows, hipFree's implicit synchronisation, sticky error cleared),
 *                        WsLayout (above), stage_upload / stage_release (the pinned upload: the
 *                        slot's event is always recorded behind its copies)
 *   ssw_host_firstpass.inc  one first-pass run is an FpReq through fp_shape, fp_layout,
 *                        FpUpload (the cached-graphs policy), fp_launch, fp_fetch;
 *                        decoder_alignment's second half is an AlignSegReq through
 *                        align_word_segments' steps, its threaded ones over for_utt_ranges
 *   ssw_host_*.inc       device model and loaders' upload, batched scoring, alignment, the
 *                        mgau_t / search-module shaped objects, features, the front end
 *                        (ssw_host_fe.inc; its tables are built in ssw_model.c), device-memory
 *                        helpers, the RCCL gather of final alignments (ssw_host_comm.inc)
 */
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ssw_internal.h"

#define HIP_OK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            ssw_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,   \
                          __LINE__);                                                         \
            return -1;                                                                       \
        }                                                                                    \
    } while (0)

#include "ssw_senone_lds.inc"

namespace {
#include "ssw_dev_common.inc"
#include "ssw_k1a_chain.inc"
#include "ssw_senone_common.inc"
#include "ssw_scan_common.inc"
#include "ssw_k1a_frames.inc"
#include "ssw_top5_select.inc"
#define SSW_CONT_SEL_FN __host__ __device__ __forceinline__
#include "ssw_cont_select.inc"
#include "ssw_k1a_mfma.inc"
#include "ssw_k1b_senone.inc"
#include "ssw_k4_feat.inc"
#include "ssw_align_common.inc"
#include "ssw_k2_align.inc"
#include "ssw_k2_anytopo.inc"
#include "ssw_search_common.inc"
#include "ssw_k5_firstpass.inc"
#include "ssw_k6_compact.inc"
#include "ssw_k7_fpactive.inc"
#include "ssw_fe_log.inc"
#include "ssw_k8_fe.inc"
#include "ssw_k8_fe_any.inc"
#include "ssw_k9_grammar.inc"
#include "ssw_k10_semi.inc"
#include "ssw_k11_cont.inc"
#include "ssw_k12_feat.inc"
#include "ssw_k13_vad.inc"

} // namespace

#include "ssw_ws_layout.inc"
#include "ssw_xcd_cut.inc"
#include "ssw_slot_layout.inc"
#include "ssw_fp_shape.inc"
#include "ssw_fpa_shape.inc"
#include "ssw_feat_tiles.inc"
#include "ssw_host_model.inc"
#include "ssw_host_semi.inc"
/* ssw_host_cont.inc comes LAST: kernels are emitted in the order the host code first launches
 * them, and the continuous-model kernels behind every other one leave the code object's layout
 * ahead of them -- the placement of the PTM kernels -- as it was */
static int cont_check_shape(const ssw_model_s *m, int scorer);
static int cont_refuse(const ssw_model_s *m, const char *who);
static int cont_launch(ssw_model_s *m, const float *d_feats, int32_t n_frames, int16_t *d_out,
                       hipStream_t st);
static int cont_refuse_active(const ssw_model_s *m, const char *who);
/* one launch of cont_listed_kernel: device pointers; d_row_of_frame NULL = frame t reads bitmap
 * row t; cap <= 0 = n_sen; d_yes only with full == 2 */
struct ContListedReq {
    const float *d_feats;
    int32_t n_frames;
    const uint32_t *d_listed;
    const int32_t *d_row_of_frame;
    int16_t *d_out;
    const int16_t *d_yes;
    int cap, full;
};
static size_t cont_listed_lds(const ssw_model_s *m, int cap);
static int cont_listed_launch(ssw_model_s *m, const ContListedReq &Q, hipStream_t st);
static int cont_align_active(ssw_model_t *m, const float *d_feats, int32_t n_utts,
                             const int32_t *frame_off, const int32_t *phone_off,
                             const uint16_t *senid, const int16_t *tmatid, const int32_t *sf,
                             const int32_t *ef, const uint32_t *seed_active,
                             ssw_align_entry_t *state_io, int32_t *status, int16_t *d_senscr,
                             void *stream);
#include "ssw_host_score.inc"
#include "ssw_host_align.inc"
#include "ssw_host_compact.inc"
#include "ssw_active_set.inc"
#include "ssw_host_active.inc"
#include "ssw_host_mllr.inc"
#include "ssw_host_mgau.inc"
#include "ssw_host_search.inc"
#include "ssw_host_feat.inc"
#include "ssw_host_fe.inc"
#include "ssw_host_fe_any.inc"
#include "ssw_host_firstpass.inc"
#include "ssw_host_fpactive.inc"
#include "ssw_host_grammar.inc"
#include "ssw_host_devmem.inc"
#include "ssw_host_comm.inc"
#include "ssw_host_cont.inc"
/* ... and the feature kernels of every configuration behind those, for the same reason */
#include "ssw_host_featex.inc"
/* ... and the listed-senone kernel of continuous models behind those */
#include "ssw_host_cont_listed.inc"
/* ... and the voice activity detector's behind those */
#include "ssw_host_vad.inc"
