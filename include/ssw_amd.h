/*
 * ssw_amd.h -- C ABI of the MI355X-native SoundSwallower acoustic hot path.
 *
 * Everything here is `extern "C"`, plain pointers and sizes.  Each entry point names the
 * reference interface it stands in for (file:line relative to the SoundSwallower tree) so a
 * maintainer can bind it from the reference's C code; INTEGRATION.md shows the binding.
 *
 * Conventions follow the reference: int return, 0 on success, < 0 on error (the message is
 * kept per thread and returned by ssw_last_error()); constructors return NULL on error;
 * objects are freed by their *_free function.  Calls are synchronous unless a stream is passed.
 * Pointers named d_* are device (HIP) pointers, everything else is host memory.
 *
 * Threading: as the reference's decoder, a model is NOT re-entrant.  An ssw_model_t owns the
 * workspaces its calls use (top-N block, alignment and first-pass arenas, cached utterance
 * offsets, the score rows of ssw_align_text_batch): one call at a time per model, from any
 * thread; calls on different models -- one per host thread or per stream of work -- run side by
 * side.  Host-only calls (ssw_first_pass_prepare, ssw_alignment_populate, the dictionary and JSON
 * functions) only read the model and may run beside a device call on it.  The rule is enforced:
 * a compute call that finds another thread inside one on the same model fails with "the model is
 * in use by another thread" instead of sharing its workspaces.
 *
 * Inputs: non-finite features are not refused (checking every row would cost a pass over the
 * batch); every (codebook, stream) pair they touch fails the scan's proof test and is scored by
 * the exact in-wave pass.  PTM scorer (round 5): that pass does what the reference does with
 * them -- its (int32) casts of a NaN are x86's 0x80000000, and eval_cb's staged dimension walk
 * (src/ptm_mgau.c:150-225) drops every density of a stream with a NaN in dimensions 0..8 while
 * a NaN confined to the last four dimensions lets densities through with INT32_MIN -- so NaN
 * and +-Inf rows score as in the reference (tests/test_gpu_nonfinite.py, against the oracle
 * compiled on x86).  ms scorer: infinities likewise; with a NaN the reference's compute_dist
 * (src/ms_gauden.c:397-420) leaves its top-N entries as they were, i.e. reads the PREVIOUS
 * frame's ids from its buffer -- a result no batch can reproduce and none is claimed.
 * ms scorer on a continuous-density model (one codebook per senone, ssw_model_is_continuous):
 * equality with the reference is claimed for finite features under which every codebook takes
 * at least topn densities (every density scores >= (float)INT32_MIN: any real cepstral input).
 * Otherwise the reference again reads stale ids from its persistent buffer; the result here is
 * a deterministic row (an entry no density filled counts as density 0 at WORST_DIST) and no fault.
 * Range: any finite feature gives the reference's scores, but the fast path of the scoring
 * kernels (the matrix-core scan, binary16 operands) only trusts frames whose features lie
 * within +-255 -- cepstral features of the shipped front end are a tenth of that; a frame
 * beyond takes the exact in-wave pass, ~13 x the work.  Data in another scale altogether
 * (integer-scaled cepstra) is scored fastest with SSW_SCAN=fma, the vector-unit scan, which
 * has fp32's range.
 */
#ifndef SSW_AMD_H
#define SSW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSW_ABI_VERSION 2 /* 2: ssw_model_info_t grew (scan_mode ..), round 5 */

/* ------------------------------------------------------------------------------------ */
/* Configuration: the scalar parameters the path reads from config_t                     */
/* (include/soundswallower/config_defs.h:94-97, 198-253).                                */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_config_s {
    double logbase;   /* "logbase"   1.0001 */
    double varfloor;  /* "varfloor"  1e-4   */
    double mixwfloor; /* "mixwfloor" 1e-7   */
    double tmatfloor; /* "tmatfloor" 1e-4   */
    int32_t topn;     /* "topn"      4      */
    int32_t ds;       /* "ds"        1      */
    int32_t aw;       /* "aw"        1      */
    int32_t device;   /* HIP device ordinal; -1 = current device; SSW_DEVICE_NONE = load the
                         host tables only (loader checks), every compute call then fails */
} ssw_config_t;
#define SSW_DEVICE_NONE (-2)

void ssw_config_defaults(ssw_config_t *cfg);
const char *ssw_last_error(void);
int ssw_abi_version(void);

/* ------------------------------------------------------------------------------------ */
/* Acoustic model: replaces the loading half of acmod_load_am (src/acmod.c:62-129):      */
/* bin_mdef_read (src/bin_mdef.c:310), tmat_init (src/tmat.c:107), gauden_init           */
/* (src/ms_gauden.c:304), read_sendump / read_mixw (src/ptm_mgau.c:456, 611),            */
/* senone_mixw_read (src/ms_senone.c:103).  Tables are derived on the host exactly as    */
/* the reference derives them, then laid out for the GPU and uploaded once.              */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_model_s ssw_model_t;

/* sendump or mixw may be NULL (one of them is required for scoring); mdef/tmat may be NULL
 * when only scoring tables are wanted and n_sen can be taken from mixw. */
ssw_model_t *ssw_model_load(const char *mdef, const char *means, const char *variances,
                            const char *sendump, const char *mixw, const char *tmat,
                            const ssw_config_t *cfg);
void ssw_model_free(ssw_model_t *m);

typedef struct ssw_model_info_s {
    int32_t n_cb, n_feat, n_density, veclen_total;
    int32_t n_sen, n_ci_sen, n_ciphone, n_phone, n_emit_state, n_tmat, n_sseq, sil;
    int32_t n_floored, topn, has_ptm, has_ms, device;
    int32_t veclen[8];
    /* ABI 2.  The speculative top-N scan runs on the matrix cores only on a device that has
     * passed the load-time self-test of the one hardware property its error bound assumes (the
     * accumulation error of v_mfma_f32_32x32x16_f16, csrc/ssw_model.c): ssw_model_load measures
     * it with adversarial and random cancelling tiles against fp64 / closed-form sums, and on a
     * failure (or a HIP error) every batch takes the vector-unit scan, whose bound is replayed on
     * the CPU.  scan_mode: 1 matrix cores, 0 vector unit.  mfma_selftest: 1 passed, -1 failed
     * (fell back), 0 not run (no device, no scan tables, SSW_MFMA_SELFTEST=off). */
    int32_t scan_mode, mfma_selftest;
    float mfma_selftest_worst_u; /* worst |D - exact| / sum |terms| seen, in u = 2^-24 */
    float mfma_selftest_ms;      /* what the self-test added to ssw_model_load */
} ssw_model_info_t;
int ssw_model_info(const ssw_model_t *m, ssw_model_info_t *out);
/* one line on the self-test's outcome ("" when it did not run); owned by the model */
const char *ssw_model_selftest_message(const ssw_model_t *m);

/* Host copies of the derived tables, for loader parity checks.  Returns a pointer owned by
 * the model and writes the byte size.  Layouts: MEAN/VAR float32 in s3 file order
 * [cb][feat][density][veclen]; DET float32 [cb][feat][density]; PTM_MIXW uint8
 * [feat][density][n_sen]; MS_PDF uint8 [sen][feat][density]; TP uint8 [tmat][n][n+1];
 * SSEQ uint16 [n_sseq][n_emit]; SEN2CB int16 [n_sen]; LOGADD8 uint8[256];
 * PHONE_SSID / PHONE_TMAT int32 [n_phone].  The last four are the device-layout Gaussian
 * tables (no reference counterpart; exposed so the scan's error bound can be replayed on
 * the CPU): REC float32 [cb*feat][density][32] = mean[0..15) | det[15] | scale[16..31);
 * SCAN_REC the same shape holding the quadratic form a[0..15) | c[15] | b[16..31);
 * SCAN_D0 float32 [cb*feat][32], element 0 = the codebook's reference det (and, for the
 * matrix-core scan, 1 = 2^s, 2 = 2^-s, 3 = 2^ec: its operands' scales, csrc/ssw_model.c);
 * SCAN_EXACT uint32 [cb*feat][132] = count, then the densities scored in the exact form;
 * SCAN_REC_MFMA / SCAN_EXACT_MFMA the same two for the matrix-core scan (its own error
 * constant; its c is what the two parts below add up to, unscaled), SCAN_WFRAG uint16
 * (binary16) [cb*feat][4][2][2][64][8]: those records, scaled by 2^-s (c by 2^-(s + ec)), cut
 * into two binary16 parts in MFMA A-fragment order. */
enum ssw_table {
    SSW_TAB_MEAN = 0, SSW_TAB_VAR, SSW_TAB_DET, SSW_TAB_PTM_MIXW, SSW_TAB_MS_PDF, SSW_TAB_TP,
    SSW_TAB_SSEQ, SSW_TAB_SEN2CB, SSW_TAB_LOGADD8, SSW_TAB_PHONE_SSID, SSW_TAB_PHONE_TMAT,
    SSW_TAB_REC, SSW_TAB_SCAN_REC, SSW_TAB_SCAN_D0, SSW_TAB_SCAN_EXACT,
    SSW_TAB_SCAN_REC_MFMA, SSW_TAB_SCAN_EXACT_MFMA, SSW_TAB_SCAN_WFRAG
};
const void *ssw_model_table(const ssw_model_t *m, int which, size_t *nbytes);

/* ------------------------------------------------------------------------------------ */
/* MLLR speaker adaptation: mllr_t (include/soundswallower/mllr.h:58-67), mllr_read      */
/* (src/ps_mllr.c:47-127) and gauden_mllr_transform (src/ms_gauden.c:459-539), which      */
/* every scorer's `transform` slot ends in.                                               */
/* ------------------------------------------------------------------------------------ */
/* Laid out exactly as mllr_t: the pointer acmod_update_mllr hands to the vtable's transform
 * slot is read as one of these.  A[f][class][row][col], b[f][class][row], h[f][class][row]. */
typedef struct ssw_mllr_s {
    int refcnt;
    int n_class;
    int n_feat;
    int *veclen;
    float ****A;
    float ***b;
    float ***h;
    int32_t *cb2mllr; /* unused, as in the reference */
} ssw_mllr_t;

/* mllr_read: the text file of whitespace-separated numbers -- n_class, n_feat, then per stream
 * its veclen and per class A[veclen][veclen], b[veclen], h[veclen].  NULL on error
 * (ssw_last_error: a file that cannot be opened, a short file, n_class < 1). */
ssw_mllr_t *ssw_mllr_read(const char *path);
/* From flat arrays: A[f] float32 [n_class][veclen[f]][veclen[f]], b[f] and h[f] float32
 * [n_class][veclen[f]].  The numbers are copied. */
ssw_mllr_t *ssw_mllr_create(int32_t n_class, int32_t n_feat, const int32_t *veclen,
                            const float *const *A, const float *const *b, const float *const *h);
ssw_mllr_t *ssw_mllr_retain(ssw_mllr_t *mllr);
int ssw_mllr_free(ssw_mllr_t *mllr); /* the references left */

/* gauden_mllr_transform on the model, in place: class 0 of the transform (the reference uses no
 * other) on the means and variances AS THE FILES HOLD THEM -- a transform is never applied on top
 * of an earlier one, applying twice equals applying once, and NULL puts the files' parameters
 * back -- then every table derived from them is rebuilt and, on a device model, copied into the
 * allocations the load made.  Works on a SSW_DEVICE_NONE model (host tables only).  Refused
 * before anything is touched, model and device unchanged: n_feat or a veclen that is not the
 * model's, n_class < 1, a non-finite number in class 0, a model in use by another thread.
 * 0, or -1 (ssw_last_error).  Rows scored earlier (on the device, or held by ssw_mgau_prescore)
 * are those of the parameters they were scored with: the caller scores again. */
int ssw_model_apply_mllr(ssw_model_t *m, const ssw_mllr_t *mllr);
/* 0 after load, +1 per successful ssw_model_apply_mllr (a NULL one included): callers that cache
 * rows compare it */
int ssw_model_mllr_generation(const ssw_model_t *m);
/* measurement aid (tools/bench_mllr.py): what the last successful ssw_model_apply_mllr took, in
 * ms -- [0] the host transform and table rebuild, [1] the synchronise and the copies to the
 * device (0 on a SSW_DEVICE_NONE model) */
int ssw_model_mllr_timing(const ssw_model_t *m, float ms[2]);

/* ------------------------------------------------------------------------------------ */
/* Batched senone scoring (NEW: the reference scores one frame per call).                */
/* One call scores every frame of a batch of utterances with compallsen = yes:           */
/*   acmod_score -> ptm_mgau_frame_eval   (src/acmod.c:822-860, src/ptm_mgau.c:408-454)   */
/*   acmod_score -> ms_cont_mgau_frame_eval (src/ms_mgau.c:278-368)                       */
/* feats: float32 [n_frames][veclen_total] (streams back to back, the row acmod keeps in  */
/* feat_buf, src/feat.c:386-395).  utt_off: int32 [n_utts+1], frame offsets; every         */
/* utterance starts from the reset top-N history {cw = m, score = INT32_MIN}              */
/* (src/ptm_mgau.c:706-713).  out: int16 [n_frames][n_sen].                               */
/* ------------------------------------------------------------------------------------ */
/* SSW_SCORER_S2_SEMI: acmod_score -> s2_semi_mgau_frame_eval (src/s2_semi_mgau.c:829-875), the   */
/* scorer of single-codebook (semi-continuous) models: n_feat <= 8 streams of <= 32 dimensions,  */
/* <= 256 densities, topn 1..4, any ds, topn_beam 0.  Its top-N history is the same two-slot     */
/* ring; it normalises per stream by the best density and not over the senones.  Equality with  */
/* the reference is claimed for finite features; a NaN or infinite feature gives a              */
/* deterministic row and no fault.                                                              */
enum ssw_scorer { SSW_SCORER_PTM = 0, SSW_SCORER_MS = 1, SSW_SCORER_S2_SEMI = 2 };
/* the scorer acmod_load_am would choose for the model without senmgau (src/acmod.c:101-119):
 * PTM when the codebooks number the CI phones, are at most 256 and 8-bit mixture weights are
 * loaded; else S2_SEMI for a single codebook with such weights; else MS when a mixture_weights
 * file gave its table; else -1 */
int ssw_model_scorer(const ssw_model_t *m);
/* 1 for a continuous-density model: its codebooks number its senones (and are neither one nor
 * the CI phones) and a mixture_weights file was given.  Such a model is the ms scorer's with the
 * reference's .cont. map, sen2cb[s] = s (src/ms_senone.c:238-250): ssw_model_scorer answers
 * SSW_SCORER_MS.  Limits, refused at load by name: <= 8 streams of <= 64 dimensions, <= 64
 * densities, topn <= 8 or >= the densities (then all of them, in index order, no selection), no
 * sendump, <= 32767 senones.  It is scored in whole rows (compallsen = yes): ssw_score_batch(_ex,
 * _host), the ms drop-in, ssw_forced_align_batch, ssw_align_text_batch, ssw_first_pass_batch and
 * ssw_recognize_batch take it (flags, carry_in, carry_out and ds are ignored, as for ms).  The
 * *_active entry points (the reference's default configuration, compallsen = no) refuse it by
 * name until ssw_model_enable_active has been called on it, and take it from then on:
 * ms_cont_mgau_frame_eval then evaluates the codebooks of the listed senones only and normalises
 * over them (src/ms_mgau.c:322-365).  The compact-row calls, ssw_score_batch_topn, the
 * ssw_debug_scan_* calls and SSW_SCAN / SSW_SCAN_AUDIT settings are refused by name for every
 * continuous model. */
int ssw_model_is_continuous(const ssw_model_t *m);
/* continuous model: build and upload the senone-major table of the listed-senone kernel; from
 * then on the *_active entry points take the model.  Idempotent.  0 for a model that is not
 * continuous (its *_active calls need nothing).  -1: no device, out of memory (model unchanged).
 * The table holds the Gaussians once more in a second layout, i.e. it doubles their device
 * memory; ssw_model_apply_mllr keeps it up to date and ssw_model_free releases it. */
int ssw_model_enable_active(ssw_model_t *m);
int ssw_model_active_enabled(const ssw_model_t *m);   /* 1 / 0 */
/* test surface, like the other ssw_debug_* calls: ms_cont_mgau_frame_eval(compallsen = no) for a
 * batch.  listed: host uint32 [n_frames][(n_sen + 31) / 32], bridges being ordinary bits.
 * full 0: only listed entries of d_out are written; 1: the others as senone_listed_kernel<true>
 * writes them for ms.  Refused unless the model is continuous and enabled. */
int ssw_debug_cont_score_listed(ssw_model_t *m, const float *d_feats, int32_t n_frames,
                                const uint32_t *listed, int32_t full, int16_t *d_out, void *stream);

/* device pointers, asynchronous on `stream` (a hipStream_t, NULL = default stream) */
int ssw_score_batch(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                    const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream);
/* The same with the reference's history semantics made available to batches.  The reference
 * never resets the PTM top-N history after start-up: it carries from utterance to utterance
 * (acmod_start_utt only resets frame_idx, src/acmod.c:367) and across acmod_rewind from the
 * first pass of forced alignment into the second (src/decoder.c:786-793, src/ptm_mgau.c:425-448);
 * only the codeword ORDER matters (tie-breaks among equal truncated scores).
 * The reference's history is a ring of TWO slots indexed by frame % 2 (n_fast_hist = 2,
 * src/ptm_mgau.c:425-437, :804) and frame numbers restart at 0 with every utterance and after
 * acmod_rewind: frame t > 0 starts from frame t - 1, but frame 0 copies slot 1 -- the final order
 * of the last ODD-numbered frame scored before it.  After an utterance of even length that is
 * its last frame; after one of odd length T >= 3 it is frame T - 2; an utterance of one frame
 * leaves slot 1 as it found it.
 *   flags      SSW_SCORE_CARRY_UTTS: no reset at the utterance boundaries of the batch: each
 *              utterance's frame 0 starts from slot 1 as the utterances before it left it
 *              SSW_SCORE_CARRY_OUT_REWIND: see carry_out
 *   carry_in   optional uint32 [n_cb * n_feat], 4 codewords packed best first: the order the
 *              batch's first frame starts from (NULL = the reset history)
 *   carry_out  optional uint32 [n_cb * n_feat] (makes the call synchronous).  Default: the order
 *              after the batch's last frame -- carry_in of a call that CONTINUES the same utterance
 *              (cut it after an even number of frames if an utterance boundary with
 *              SSW_SCORE_CARRY_UTTS follows, so that the parity of its frames is kept).  With
 *              SSW_SCORE_CARRY_OUT_REWIND: slot 1 after the batch -- carry_in of the next
 *              UTTERANCE, or of the second pass of decoder_alignment over the same utterance after
 *              acmod_rewind (with SSW_SCORE_CARRY_UTTS the batch's utterances are walked back to
 *              the last one with two frames; without it only the last utterance counts; if no
 *              frame wrote the slot, carry_in / the reset order comes back).
 *              Frame down-sampling (ssw_config_t.ds > 1): the call has no argument for the frame
 *              number its first frame has within the utterance -- every utterance of a call is
 *              numbered from 0, and with it the frames a codebook is re-scanned on (frame % ds ==
 *              0, src/ptm_mgau.c:241).  A call that CONTINUES an utterance is therefore only the
 *              reference's scoring when the calls before it end after a multiple of lcm(2, ds)
 *              frames of that utterance (2: the parity above; ds: the phase).
 * The ms scorer keeps no history and reads no ds: the three are ignored for it.
 * SSW_SCORER_S2_SEMI keeps the same ring of two slots (src/s2_semi_mgau.c:845-855): flags,
 * carry_in and carry_out mean the same, a word packing the stream's (up to) 4 codewords. */
#define SSW_SCORE_CARRY_UTTS 1u
/* the caller runs kernels of ANOTHER stream beside this call (the alignment of the previous
 * chunk beside the scoring of the next, section "Multi-GPU" / soundswallower_amd/jobs.py): the
 * persistent scoring workgroups then leave after 8 frame pairs instead of staying for the
 * whole batch, so the other stream finds free wave slots every ~100 us.  Same results. */
#define SSW_SCORE_SHARE_DEVICE 2u
#define SSW_SCORE_CARRY_OUT_REWIND 4u
int ssw_score_batch_ex(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                       const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream,
                       uint32_t flags, const uint32_t *carry_in, uint32_t *carry_out);
/* host pointers, synchronous: copies in, scores, copies out -- as a three-stage pipeline over
 * sub-batches of whole utterances (~1024 frames) through pinned staging.  History reset per
 * utterance.  An utterance of more than 16,384 frames (SSW_HOST_PIPE_CAP) is scored in pieces
 * of that many that hand the history on, so the staging the model keeps for this call stops at
 * 2 x 16,384 feature rows + score rows pinned on the host and as many on the device (en-us:
 * 2 x 171 MB each), however long the utterances are.  A piece keeps the frame numbers of its
 * utterance: with ds > 1 it re-scans on the frames the uncut utterance re-scans on, whether or not
 * ds divides the piece length (the cap is rounded down to even, nothing else). */
int ssw_score_batch_host(ssw_model_t *m, int scorer, const float *feats, int32_t n_frames,
                         const int32_t *utt_off, int32_t n_utts, int16_t *out);
/* Debug/parity view of the PTM top-N state after normalisation for every frame of the last
 * ssw_score_batch* call: cw uint8 / score int32 laid out [n_frames][n_cb][n_feat][topn]. */
int ssw_score_batch_topn(ssw_model_t *m, int32_t n_frames, uint8_t *cw, int32_t *score);
/* Debug/parity view of the matrix core itself: D = A B + C, one v_mfma_f32_32x32x16_f16 per tile
 * (host pointers; A [n_tiles][32][16], B [n_tiles][16][32] binary16 bit patterns, C, D
 * [n_tiles][32][32] float).  The scan's error bound assumes an accumulation error of at most
 * 34 x 2^-24 of the sum of the |terms| for this instruction (csrc/ssw_model.c);
 * tests/test_gpu_mfma_bound.py measures it with this call. */
int ssw_debug_mfma_f16_tiles(ssw_model_t *m, const uint16_t *A, const uint16_t *B, const float *C,
                             float *D, int32_t n_tiles);
/* Debug/parity view of the matrix-core scan: the raw keys (upper bounds of the densities,
 * relative to the codebook's reference level SCAN_D0, before their widening) of codebook x
 * stream `cbf` for every frame of d_feats, computed exactly as the scan computes them.
 * keys: host float [n_frames][128]; inert rows (SCAN_EXACT_MFMA densities) read about -3e38. */
int ssw_debug_scan_keys(ssw_model_t *m, const float *d_feats, int32_t n_frames, int32_t cbf,
                        float *keys);
/* Debug view of the scan's selection alone: the five best of caller-supplied keys per frame, found
 * as the matrix-core scan finds them (the keys laid out as its tiles deliver them, then its
 * selection network, swap of the wave's halves and merge).  Host pointers: keys float
 * [n_frames][128] by density (their low 7 bits are overwritten with labels, as in the scan); idx
 * int32 [n_frames][5] densities, best first; top float [n_frames][5] their keys, label bits
 * cleared.  Needs a model loaded on a device, nothing of the model itself. */
int ssw_debug_scan_top5(ssw_model_t *m, const float *keys, int32_t n_frames, int32_t *idx,
                        float *top);
/* Counters of the last PTM batch: [0] = (chain,frame) pairs the history-free pass could not
 * prove order-independent and handed to the exact sequential pass, [1] = pairs total. */
int ssw_score_batch_stats(ssw_model_t *m, int64_t stats[2]);
/* In-process audit of the matrix-core scan (round 5).  With SSW_SCAN_AUDIT=k in the environment
 * when the model is loaded, every k-th wave of the scan hands ALL of its frames to the exact
 * in-wave pass -- proven or not -- and compares what the exact pass finds for a pair the scan had
 * proven with what the scan wrote for it.  stats[0] = proven pairs so audited, stats[1] = of
 * those, pairs that differ: 0 unless the scan's error bound does not hold on this device (the
 * load-time self-test of ssw_model_info_t checks the same assumption on synthetic tiles; the
 * audit checks the claim itself on the caller's data).  Running totals since ssw_model_load;
 * results are the same with and without the audit.  Cost at k = 1: the scan ~13 x. */
int ssw_scan_audit_stats(ssw_model_t *m, int64_t stats[2]);

/* Per-kernel timing with HIP events recorded on the launch stream (for bench.py's roofline
 * line).  When enabled every ssw_score_batch call brackets each kernel with events;
 * ssw_get_kernel_timing synchronises and returns the last call's milliseconds.  Return value 2:
 * ms[0] = top-N (density) kernel(s), ms[1] = senone kernel.  Return value 1 (a batch large
 * enough to be scored in pieces, scan and senone launches alternating: there is no split):
 * ms[0] = the whole call (ms[1] is set to 0 when n >= 2).  An event between two launches costs
 * ~2 us of its own.  -1 on error.  After a call with SSW_SCORER_S2_SEMI and with n >= 3 the return
 * value is 3: ms[0] = its density and chain kernels, ms[1] = its senone kernel, ms[2] = the chain
 * kernel's share of ms[0]. */
int ssw_set_kernel_timing(ssw_model_t *m, int enable);
int ssw_get_kernel_timing(ssw_model_t *m, float *ms, int n);
/* measurement aid: `reps` ssw_score_batch calls on the same batch back to back, then one
 * synchronise (tools/bench_frame_sync.py) */
int ssw_debug_score_loop(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                         const int32_t *utt_off, int32_t n_utts, int16_t *d_out, int32_t reps,
                         void *stream);

/* ------------------------------------------------------------------------------------ */
/* Scorer object: drop-in for mgau_t / mgaufuncs_t (include/soundswallower/acmod.h:93-111).*/
/* The first two members mirror mgau_t so acmod can write frame_idx                       */
/* (src/acmod.c:367,748,760) and call through vt.                                         */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_mgau_s ssw_mgau_t;
typedef struct ssw_mgaufuncs_s {
    const char *name;
    int (*frame_eval)(ssw_mgau_t *mgau, int16_t *senscr, uint8_t *senone_active,
                      int32_t n_senone_active, float **feat, int32_t frame,
                      int32_t compallsen);
    /* mllr: an ssw_mllr_t / the reference's mllr_t.  ssw_model_apply_mllr on the model behind
     * the scorer; the rows ssw_mgau_prescore holds are dropped, the top-N history is left alone
     * (as in the reference).  0, or -1: a refused transform, or NULL (the reference never
     * passes one; the model stays as it is) */
    int (*transform)(ssw_mgau_t *mgau, void *mllr);
    void (*free)(ssw_mgau_t *mgau);
} ssw_mgaufuncs_t;
struct ssw_mgau_s {
    ssw_mgaufuncs_t *vt;
    int frame_idx;
};

/* ptm_mgau_init(acmod_t *) (ptm_mgau.h:94) / ms_mgau_init(acmod_t *) (ms_mgau.h) */
ssw_mgau_t *ssw_ptm_mgau_init(ssw_model_t *m);
ssw_mgau_t *ssw_ms_mgau_init(ssw_model_t *m);
/* s2_semi_mgau_init(acmod_t *) (s2_semi_mgau.h) for a single-codebook model: the vtable's name is
 * "s2_semi".  frame_eval scores a frame acmod has not scored yet (frame >= frame_idx) from the
 * other history slot's order and gives an earlier frame its slot's row again.  With compallsen =
 * 0 the listed senones (bridge entries of the delta list included) get the values compallsen = 1
 * gives them and every other senone 0: this scorer's Gaussians and normalisation do not depend on
 * the list.  ssw_mgau_reset_hist and ssw_mgau_prescore work as for PTM. */
ssw_mgau_t *ssw_s2_semi_mgau_init(ssw_model_t *m);
/* ptm_mgau_reset_fast_hist (src/ptm_mgau.c:694) without its reallocation */
void ssw_mgau_reset_hist(ssw_mgau_t *mgau);
/* NEW: score a whole utterance in one batch and cache it; frame_eval(frame) then copies row
 * `frame`.  Without it frame_eval scores one frame per call on the GPU. */
int ssw_mgau_prescore(ssw_mgau_t *mgau, const float *feats, int32_t n_frames);

/* ------------------------------------------------------------------------------------ */
/* Forced alignment: state_align_search (src/state_align_search.c) + hmm_vit_eval         */
/* (src/hmm.c:741) + the state level of alignment_t (include/soundswallower/alignment.h). */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_align_entry_s {
    int32_t start, duration, score; /* alignment_entry_t.{start,duration,score} */
} ssw_align_entry_t;

/* Batch of independent utterances.
 *   d_senscr  int16 [total_frames][n_sen]   scores as acmod_score returns them
 *   frame_off int32 [n_utts+1]              rows of d_senscr per utterance
 *   phone_off int32 [n_utts+1]              phones per utterance (offsets into per-phone arrays)
 *   senid     uint16 [total_phones][n_emit] mdef->sseq[ssid][j] (src/hmm.c:99)
 *   tmatid    int16 [total_phones]
 *   sf, ef    int32 [total_phones]          state_align_search.c:464-471 (0 / INT_MAX = free)
 *   state_io  [total_phones*n_emit]         in: what alignment_populate left in the state
 *                                           entries (src/ps_alignment.c:237-239); out: backtrace
 *   status    int32 [n_utts]                0 ok, -1 "Failed to reach final state",
 *                                           -(2+frame) "Alignment failed in frame"
 * All host pointers except d_senscr.  Synchronous.
 * n_emit is the transition matrices' (hmm_vit_eval, src/hmm.c:741-759): 3 takes
 * hmm_vit_eval_3st_lr in the kernels this library is built around; 5 (hmm_vit_eval_5st_lr) and
 * 1, 2, 4 (hmm_vit_eval_anytopo) take one plain kernel, a wave per utterance.  More than
 * HMM_MAX_NSTATE = 5 states is refused, as hmm_context_init does (src/hmm.c:60-64). */
int ssw_align_batch(ssw_model_t *m, const int16_t *d_senscr, int32_t n_utts,
                    const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                    const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                    ssw_align_entry_t *state_io, int32_t *status, void *stream);
/* How the last alignments were made (round 5).  Utterances of up to 1024 phones first go through
 * a kernel that keeps, per state and frame, a 2-bit back-pointer instead of the reference's
 * {history, score} token (src/state_align_search.c:149-175) and recovers the scores the backtrace
 * needs by replaying the path; what that kernel cannot follow -- the reference's stale-exit-score
 * and left-over-t2 cases (src/hmm.c:496-520), a backtrace that runs into a missing token -- it
 * hands, untouched, to the kernel with the full tokens.  stats[0] = utterances that took the
 * byte-token kernel, stats[1] = of those, the ones that were handed on; running totals since
 * ssw_model_load.  Results are the same either way; SSW_ALIGN_BT=0 skips the first kernel. */
int ssw_align_stats(ssw_model_t *m, int64_t stats[2]);
/* The same search in the reference's DEFAULT configuration (compallsen = no), scoring included:
 * acmod scores only the senones of the HMMs the search has active (acmod_activate_hmm /
 * acmod_flags2list, src/acmod.c:905-999 -- a uint8 delta list whose gaps above 255 list extra
 * senones), the PTM scorer scans only the codebooks those senones belong to, normalises over
 * them and subtracts the best LISTED score from every entry (src/ptm_mgau.c:264-403), and this
 * search never clears acmod's set (src/state_align_search.c:186-189): frame t sees the seed --
 * what the first pass left active, seed_active uint32 [n_utts][(n_sen + 31) / 32], bit b of
 * word b / 32, or NULL -- plus the senones of every phone entered so far.  Which phones are
 * entered when follows from sf / ef alone when those do not decrease along an utterance (the
 * windows alignment_populate produces); otherwise the call is refused.  d_feats: feature rows
 * [total_frames][veclen_total]; d_senscr: optional int16 [total_frames][n_sen] that receives
 * the scores exactly as acmod->senone_scores would hold them frame by frame.  Other arguments
 * and results as ssw_align_batch.  PTM scorer, history reset per utterance.
 * Limits (the call aligns over compact score rows, see below): 3-state HMMs, at most 64
 * codebooks, utterances of at most 10,922 phones (a row's per-state indices are 16 bits) --
 * beyond them the call is refused with an error; ssw_score_batch + ssw_align_batch take any
 * length but are the compallsen = yes configuration, i.e. other scores. */
int ssw_align_batch_active(ssw_model_t *m, const float *d_feats, int32_t n_utts,
                           const int32_t *frame_off, const int32_t *phone_off,
                           const uint16_t *senid, const int16_t *tmatid, const int32_t *sf,
                           const int32_t *ef, const uint32_t *seed_active,
                           ssw_align_entry_t *state_io, int32_t *status, int16_t *d_senscr,
                           void *stream);
/* The same with the scorer named (round 3): SSW_SCORER_MS follows ms_cont_mgau_frame_eval's
 * active-list half (src/ms_mgau.c:322-365): only the listed senones are evaluated and written,
 * normalised by the best of them with the int16 clamp (bridge entries of the delta list are
 * listed entries).  d_senscr rows hold 0 wherever the frame's list has no entry: acmod's buffer
 * would still show the last value of an entry that has dropped out of the list -- only bridge
 * entries ever do, when a senone between their neighbours joins the set, and no HMM reads them. */
int ssw_align_batch_active_ex(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_utts,
                              const int32_t *frame_off, const int32_t *phone_off,
                              const uint16_t *senid, const int16_t *tmatid, const int32_t *sf,
                              const int32_t *ef, const uint32_t *seed_active,
                              ssw_align_entry_t *state_io, int32_t *status, int16_t *d_senscr,
                              void *stream);
/* Compact score rows (NEW, round 5).  state_align_search only ever reads the scores of its own
 * phones' senones -- it activates just those (src/state_align_search.c:186-189), and in the
 * default configuration acmod then scores nothing else (src/acmod.c:905-945).  When the phone
 * strings of a batch are known before it is scored (BASELINE configs 3 and 5; the second pass of
 * decoder_alignment, whose phones come from alignment_populate), a PLAN lets the scorer store,
 * per utterance, rows of that utterance's states only -- [n_frames_u][3 n_phones_u rounded up to
 * even] int16 instead of [n_frames_u][n_sen]: 0.9 KB instead of 10 KB per frame for a 150-phone
 * utterance of en-us -- which the alignment kernel then reads coalesced instead of gathering
 * three scattered 2-byte values per phone from rows it touches nearly every sector of.  Every
 * senone is still evaluated (compallsen = yes: the frame's best score is taken over all of
 * them, src/ptm_mgau.c:394-400): the scores, and so the alignments, are those of
 * ssw_score_batch + ssw_align_batch bit for bit.  A senone several states of an utterance
 * share is stored once, at the first of them.
 *   ssw_compact_plan_create   frame_off / phone_off / senid as ssw_align_batch takes them (host);
 *                             builds the device tables on `stream` and returns when they are
 *                             complete.  Utterances of up to 10,922 phones.
 *   ssw_compact_plan_elems    int16 elements the compact buffer needs (the caller allocates it)
 *   ssw_compact_plan_rows     utterance u's rows: offset (elements) and row length in the buffer;
 *                             state k of the utterance (3 per phone) at column k, or at the
 *                             column of the first state with the same senone
 *   ssw_score_batch_compact   ssw_score_batch_ex for the plan's batch (utterance offsets = the
 *                             plan's frame_off; history reset per utterance), asynchronous on
 *                             `stream`; flags: SSW_SCORE_SHARE_DEVICE
 *   ssw_align_batch_compact   ssw_align_batch over those rows (tmatid, sf, ef, state_io, status
 *                             as there; the utterances, phones and senones are the plan's);
 *                             flags: SSW_ALIGN_STATE_OUT_ONLY -- state_io is output only, the
 *                             entries the backtrace does not write (states a path skips,
 *                             utterances without an alignment) come back as zeros instead of
 *                             what the caller passed in: saves the upload of 36 bytes per phone
 * A plan is bound to its model and can be used any number of times. */
typedef struct ssw_compact_plan_s ssw_compact_plan_t;
ssw_compact_plan_t *ssw_compact_plan_create(ssw_model_t *m, int32_t n_utts,
                                            const int32_t *frame_off, const int32_t *phone_off,
                                            const uint16_t *senid, void *stream);
void ssw_compact_plan_free(ssw_compact_plan_t *plan);
size_t ssw_compact_plan_elems(const ssw_compact_plan_t *plan);
int ssw_compact_plan_rows(const ssw_compact_plan_t *plan, int32_t utt, long long *row_off,
                          int32_t *stride);
/* (SSW_SCORER_S2_SEMI and single-codebook models: refused, as are ssw_compact_plan_create and
 * ssw_align_batch_active(_ex) -- that scorer stores whole rows only) */
int ssw_score_batch_compact(ssw_model_t *m, int scorer, const float *d_feats,
                            const ssw_compact_plan_t *plan, int16_t *d_compact, void *stream,
                            uint32_t flags);
int ssw_align_batch_compact(ssw_model_t *m, const ssw_compact_plan_t *plan,
                            const int16_t *d_compact, const int16_t *tmatid, const int32_t *sf,
                            const int32_t *ef, ssw_align_entry_t *state_io, int32_t *status,
                            void *stream, uint32_t flags);
#define SSW_ALIGN_STATE_OUT_ONLY 1u

/* alignment_propagate (src/ps_alignment.c:316-352): sums children into parents.
 * parent[i] = index of child i's parent; parents must appear in non-decreasing order. */
int ssw_alignment_propagate(const ssw_align_entry_t *child, const int32_t *parent,
                            int32_t n_child, ssw_align_entry_t *parent_out, int32_t n_parent);

/* Search-module shaped object: state_align_search_init/start/step/finish/free
 * (state_align_search.h:89-92; vtable slots of search_module.h:72-83).  The constructor takes
 * what state_align_search_init reads from the alignment's phone level
 * (src/state_align_search.c:458-471): per phone ssid, tmatid, start, duration. */
typedef struct ssw_state_align_search_s ssw_state_align_search_t;
ssw_state_align_search_t *ssw_state_align_search_init(ssw_model_t *m, ssw_mgau_t *mgau,
                                                      int32_t n_phones, const int32_t *ssid,
                                                      const int32_t *tmatid,
                                                      const int32_t *start,
                                                      const int32_t *duration);
int ssw_state_align_search_start(ssw_state_align_search_t *s);
/* feat = the frame's feature row; frames must be stepped in order from 0 */
int ssw_state_align_search_step(ssw_state_align_search_t *s, const float *feat, int frame_idx);
/* runs scoring + Viterbi + backtrace for all stepped frames; fills state/phone entries */
int ssw_state_align_search_finish(ssw_state_align_search_t *s);
int32_t ssw_state_align_search_n_frames(const ssw_state_align_search_t *s);
const ssw_align_entry_t *ssw_state_align_search_states(const ssw_state_align_search_t *s,
                                                       int32_t *n);
const ssw_align_entry_t *ssw_state_align_search_phones(const ssw_state_align_search_t *s,
                                                       int32_t *n);
void ssw_state_align_search_free(ssw_state_align_search_t *s);

/* ------------------------------------------------------------------------------------ */
/* Lexicon glue (host C): what decoder_alignment needs to go from       */
/* words + word windows to the per-phone rows state_align_search_init reads.               */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_dict_s ssw_dict_t;
/* dict_init (src/dict.c): text dictionaries "word PH PH ...", main then filler; <s>, </s>,
 * <sil> always exist.  Words with unknown phones are skipped. */
ssw_dict_t *ssw_dict_load(const ssw_model_t *m, const char *dict_path, const char *filler_path);
void ssw_dict_free(ssw_dict_t *d);
int32_t ssw_dict_size(const ssw_dict_t *d);
/* CI phone ids of a word's pronunciation; returns its length or -1 when unknown */
int32_t ssw_dict_pron(const ssw_dict_t *d, const char *word, int32_t *ciphones, int32_t max);
const char *ssw_ciphone_name(const ssw_model_t *m, int32_t ci);
/* bin_mdef_phone_id_nearest (src/bin_mdef.c:666-720); pos: 0 internal, 1 begin, 2 end, 3 single */
int32_t ssw_phone_id_nearest(const ssw_model_t *m, int32_t b, int32_t l, int32_t r, int32_t pos);
/* alignment_add_word per word + alignment_populate (src/ps_alignment.c:114-247): returns the
 * number of phones written (ssid, tmatid, and optionally cipid, parent word, and the word's
 * start/duration copied to each phone, which is what state_align_search_init turns into
 * sf/ef), or -1 (unknown word, too many phones). */
int32_t ssw_alignment_populate(const ssw_model_t *m, const ssw_dict_t *d, int32_t n_words,
                               const char *const *words, const int32_t *start,
                               const int32_t *duration, int32_t max_phones, int32_t *ssid,
                               int32_t *tmatid, int32_t *cipid, int32_t *parent,
                               int32_t *ph_start, int32_t *ph_duration);

/* Dictionary word ids (dict_wordid / dict_wordstr); alternates are words of their own,
 * "forward(2)".  ssw_dict_word returns NULL and ssw_dict_word_id -1 when unknown. */
const char *ssw_dict_word(const ssw_dict_t *d, int32_t wid);
int32_t ssw_dict_word_id(const ssw_dict_t *d, const char *word);
/* dict_basewid (the word an alternate belongs to; itself otherwise) and dict_filler_word
 * (from the filler dictionary, <s> and </s> excepted; src/dict.c:373-384) */
int32_t ssw_dict_base_id(const ssw_dict_t *d, int32_t wid);
int32_t ssw_dict_is_filler(const ssw_dict_t *d, int32_t wid);

/* Words added at run time.  The filler range is fixed when the dictionary is loaded, as
 * dict_init fixes filler_start and filler_end (src/dict.c:318, 337: the words of the filler
 * file, then <s>, </s> and <sil> where the file lacks them, so all three lie inside the range;
 * dict_filler_word excepts <s> and </s> by id, :378-383).  A word added later lies past
 * filler_end: it is no filler, and the silence loops of the graph builders
 * (fsg_search_add_silences, src/fsg_search.c:84-119) pass it over.
 *
 * decoder_add_word (src/decoder.c:801-865) on a loaded dictionary: phones = CI phone names
 * separated by white space.  Returns the new word id (appended: ids never move), or -1 with
 * the dictionary unchanged: an unknown phone (named), a word that exists, "w(2)" whose base
 * word is missing (src/dict.c:92-102), no phones, more phones than ssw_dict_load takes (256),
 * white space in the word.  An alternate "w(2)" is linked at the head of its base word's list
 * (src/dict.c:104-107), so graphs built with use_altpron after the add offer it.  Objects built
 * before the add (compiled grammars, graphs, plans) are snapshots and stay as they are, as the
 * reference's search_module_reinit does not add alternates again either.  Pointers that
 * ssw_dict_word returned stay valid when the dictionary grows.  Cross-word triphones are looked
 * up per phone pair when a graph or an alignment is built, so dict2pid_add_word has no
 * counterpart.  Adding while another thread runs any call on the same dictionary is the
 * caller's error. */
int32_t ssw_dict_add_word(ssw_dict_t *d, const ssw_model_t *m, const char *word, const char *phones);
/* decoder_lookup_word (src/decoder.c:867-888): the phone names separated by one space into
 * out (cut to max - 1 characters and terminated when max > 0); returns the length it needs
 * without the terminator, -1 for an unknown word. */
int32_t ssw_dict_lookup_word(const ssw_dict_t *d, const ssw_model_t *m, const char *word,
                             char *out, int32_t max);

/* ------------------------------------------------------------------------------------ */
/* First pass of forced alignment: which fillers and alternate          */
/* pronunciations the text is spoken with, and every word's frames -- the word windows the  */
/* second pass (ssw_align_batch) is constrained to.  Replaces, for the linear grammar        */
/* decoder_set_align_text builds (src/decoder.c:686-735):                                    */
/*   fsg_search_init: silence / filler loops, alternates     src/fsg_search.c:84-170, 172-253 */
/*   fsg_lextree_init: per-state phone trees                 src/fsg_lextree.c:85-276, 356-660 */
/*   fsg_search_start / _step / _finish: beam Viterbi        src/fsg_search.c:665-852          */
/*   fsg_history_entry_add: word exits                       src/fsg_history.c:129-205         */
/*   fsg_search_find_exit / _seg_iter: backtrace             src/fsg_search.c:854-925,1085-1143 */
/* The graphs are built on the host, the search runs on the GPU, one workgroup per          */
/* utterance, over senone scores already in HBM (ssw_score_batch).                          */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_first_pass_config_s {
    double beam, pbeam, wbeam; /* 1e-48, 1e-48, 7e-29 (config_defs.h) */
    double wip, pip;           /* 0.65, 1.0 */
    float lw;                  /* 6.5 */
    float silprob, fillprob;   /* 0.005, 1e-8 */
    int32_t use_filler;        /* fsgusefiller, 1 */
    int32_t use_altpron;       /* fsgusealtpron, 1 */
    /* ssw_align_text_batch only, PTM scorer: score the second pass as decoder_alignment does
     * (src/decoder.c:786-793, src/ptm_mgau.c:425-448) -- again, after the rewind, every
     * utterance starting from the top-N history its own first pass left -- instead of feeding
     * both passes with the scores made from the reset history.  The two differ only where
     * truncated densities tie; costs a second scoring pass.  0 by default. */
    int32_t two_pass_history;
} ssw_first_pass_config_t;
void ssw_first_pass_config_defaults(ssw_first_pass_config_t *cfg);

typedef struct ssw_word_seg_s {
    int32_t wid;      /* dictionary word id (ssw_dict_word): text word, alternate or filler */
    int32_t start;    /* first frame */
    int32_t duration; /* frames */
    int32_t score;    /* path score at the word's exit (fsg_hist_entry_score) */
} ssw_word_seg_t;

/* d_senscr: int16 [n_frames][n_sen] device scores of the whole batch (utterance u owns
 * frames utt_off[u] .. utt_off[u+1]); words: the texts, utterance u = words[word_off[u] ..
 * word_off[u+1]).  seg: [n_utts][max_seg]; n_seg[u] = segments written, or -1 when the
 * grammar's final state is not reached in the last frame that has word exits ("Final result
 * does not match the grammar", src/fsg_search.c:913-916), or -(2 + k) when the search succeeded
 * but its k segments do not fit max_seg (call again with max_seg >= k; ssw_forced_align_batch
 * and ssw_align_text_batch do that themselves).
 * cfg NULL = defaults.  Returns 0, or -1 (unknown word, graph too large, no device).
 * Synchronous on `stream`. */
int ssw_first_pass_batch(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                         const int16_t *d_senscr, int32_t n_frames, const int32_t *utt_off,
                         int32_t n_utts, const int32_t *word_off, const char *const *words,
                         int32_t max_seg, int32_t *n_seg, ssw_word_seg_t *seg, void *stream);

/* The first pass in two halves, for pipelines: ssw_first_pass_prepare builds the graphs of a
 * batch of texts on the host (no device call; safe on another host thread while the GPU works
 * on the previous batch), ssw_first_pass_run / ssw_forced_align_planned search them.  A plan
 * can be run any number of times (e.g. the same texts against several recordings) and is
 * freed by the caller. */
typedef struct ssw_first_pass_plan_s ssw_first_pass_plan_t;
ssw_first_pass_plan_t *ssw_first_pass_prepare(const ssw_model_t *m, const ssw_dict_t *d,
                                              const ssw_first_pass_config_t *cfg, int32_t n_utts,
                                              const int32_t *word_off, const char *const *words);
void ssw_first_pass_plan_free(ssw_first_pass_plan_t *plan);
int ssw_first_pass_run(ssw_model_t *m, const ssw_first_pass_plan_t *plan, const int16_t *d_senscr,
                       int32_t n_frames, const int32_t *utt_off, int32_t max_seg, int32_t *n_seg,
                       ssw_word_seg_t *seg, void *stream);

/* decoder_alignment (src/decoder.c:737-798) for a batch: first pass, then alignment_add_word
 * with the first pass's word windows + alignment_populate, the state alignment constrained to
 * those windows (state_align_search_init / step / finish), alignment_propagate.  The result
 * holds one alignment_t-shaped record per utterance -- word, phone and state entries with
 * (start, duration, score) -- read with the accessors below.  Arguments as
 * ssw_first_pass_batch.  Returns NULL on a call-level error; per-utterance outcomes are in
 * ssw_alignment_set_status: 0 aligned, 1 the first pass did not reach the end of the text,
 * 2 the second pass failed ("Failed to reach final state" / "Alignment failed in frame"),
 * 3 the utterance's text was rejected (decoder_set_align_text's "Unknown word ..."; the message
 * is in ssw_alignment_set_message) -- the other utterances of the batch are aligned all the same. */
typedef struct ssw_alignment_set_s ssw_alignment_set_t;
ssw_alignment_set_t *ssw_forced_align_batch(ssw_model_t *m, const ssw_dict_t *d,
                                            const ssw_first_pass_config_t *cfg,
                                            const int16_t *d_senscr, int32_t n_frames,
                                            const int32_t *utt_off, int32_t n_utts,
                                            const int32_t *word_off, const char *const *words,
                                            void *stream);
/* ssw_forced_align_batch with the graphs prepared beforehand (ssw_first_pass_prepare) */
ssw_alignment_set_t *ssw_forced_align_planned(ssw_model_t *m, const ssw_dict_t *d,
                                              const ssw_first_pass_plan_t *plan,
                                              const int16_t *d_senscr, int32_t n_frames,
                                              const int32_t *utt_off, void *stream);
/* The same from FEATURES: scores the batch's feature rows in HBM (d_feats float32
 * [n_frames][39], e.g. from ssw_feat_batch) with `scorer` into a workspace the model keeps,
 * then ssw_forced_align_batch -- decoder_start_utt .. decoder_alignment for a batch, minus the
 * MFCC front end, in one call. */
ssw_alignment_set_t *ssw_align_text_batch(ssw_model_t *m, const ssw_dict_t *d,
                                          const ssw_first_pass_config_t *cfg, int scorer,
                                          const float *d_feats, int32_t n_frames,
                                          const int32_t *utt_off, int32_t n_utts,
                                          const int32_t *word_off, const char *const *words,
                                          void *stream);
/* The first pass -- and decoder_alignment -- in the reference's DEFAULT configuration
 * (compallsen = no) for a batch (NEW, round 6).  There acmod scores, frame by frame, only the
 * senones of the HMMs the search holds active -- fsg_search_sen_active rebuilds the set before
 * every frame (src/fsg_search.c:310-325, :677-680), acmod_flags2list turns it into the uint8
 * delta list with its bridge entries (src/acmod.c:947-999), the PTM scorer scans the codebooks of
 * the listed senones, normalises over them and subtracts the best listed score
 * (src/ptm_mgau.c:264-403) -- so frame t can only be scored once frame t - 1 has been searched.
 * These calls break that dependency by speculation and proof: a trajectory of active sets is
 * assumed (the search over the compallsen = yes scores gives the first one), the whole batch is
 * scored with exactly those per-frame sets, the search runs again on those scores, and an
 * utterance whose search took the assumed sets frame for frame has, by induction over the
 * frames, read nothing but the scores the reference would have computed: it IS the reference's
 * search.  Any other utterance is right up to and including the set of its first differing
 * frame and goes round again from the sets it just took; the proven prefix grows every round.
 * Word segmentations and scores are those of the reference's default configuration (they differ
 * from the compallsen = yes ones: another normaliser per frame and, through its clamp, slightly
 * other pruning).  Texts of any length (beyond 1,024 phone-tree HMMs the long-text search
 * kernels export their sets, as ssw_first_pass_batch uses them); 3-state HMMs, <= 64 codebooks,
 * ds = 1; history reset per utterance.
 *   d_feats      feature rows [n_frames][veclen] in HBM (ssw_feat_batch)
 *   seed_active  NULL, or host uint32 [n_utts][(n_sen + 31) / 32]: acmod's flags after each
 *                utterance's last frame -- what ssw_align_batch_active takes as its seed
 *   d_senscr     NULL, or device int16 [n_frames][n_sen]: the score rows exactly as acmod's
 *                buffer would hold them frame by frame (costs one more scoring pass)
 *   rounds       NULL, or host int32 [n_utts]: searches over default-configuration scores the
 *                utterance took (1: its first assumption was proven)
 * other arguments and results as ssw_first_pass_batch.  Synchronous on `stream`.
 * Device memory the model keeps for these calls (grow-only, freed with the model): two tables
 * of exported sets (8 bytes per 64 phone-tree HMMs and frame), a bitmap of listed senones per
 * frame (n_sen / 8 bytes), the longest utterance's score rows once more, and -- when d_senscr
 * is NULL -- the batch's score rows [n_frames][n_sen] (shared with ssw_align_text_batch).
 * SSW_SCORER_S2_SEMI: this call, ssw_align_text_batch_active and ssw_recognize_batch_active take
 * the compallsen = yes route -- whole rows, one search.  For that scorer the two configurations
 * are the same computation (s2_semi_mgau_frame_eval evaluates every Gaussian and normalises per
 * stream whatever the active set is; the list only restricts which senones are summed), so the
 * results are the default configuration's all the same.  rounds are 1, the stats count one round
 * per utterance, d_senscr receives whole rows, and seed_active / listed are refused: no sets of
 * listed senones are made. */
int ssw_first_pass_batch_active(ssw_model_t *m, const ssw_dict_t *d,
                                const ssw_first_pass_config_t *cfg, int scorer,
                                const float *d_feats, int32_t n_frames, const int32_t *utt_off,
                                int32_t n_utts, const int32_t *word_off, const char *const *words,
                                int32_t max_seg, int32_t *n_seg, ssw_word_seg_t *seg,
                                uint32_t *seed_active, int16_t *d_senscr, int32_t *rounds,
                                void *stream);
/* running totals since ssw_model_load: [0] utterances searched that way, [1] their rounds
 * summed, [2] rounds of the last call, [3] utterances that needed more than one */
int ssw_first_pass_active_stats(ssw_model_t *m, int64_t stats[4]);
/* ssw_align_text_batch in the default configuration: that first pass, alignment_populate with
 * its word windows, the second pass as ssw_align_batch_active_ex runs it (acmod's set starts
 * from what the first pass's last frame left and only grows), alignment_propagate.
 * cfg->two_pass_history (PTM scorer): the second pass of every utterance starts, as
 * decoder_alignment's does after acmod_rewind, from the top-N history its own first pass left
 * in slot 1 -- every codebook's list after the last odd-numbered frame, the codebooks that
 * frame did not scan included; 0 (default): from the reset history.  The two differ only
 * where truncated densities tie; on the reference's recordings they do not (tests). */
ssw_alignment_set_t *ssw_align_text_batch_active(ssw_model_t *m, const ssw_dict_t *d,
                                                 const ssw_first_pass_config_t *cfg, int scorer,
                                                 const float *d_feats, int32_t n_frames,
                                                 const int32_t *utt_off, int32_t n_utts,
                                                 const int32_t *word_off, const char *const *words,
                                                 void *stream);
/* Debug / parity view: the top-N orders the last ssw_align_text_batch_active call with
 * two_pass_history handed from every utterance's first pass to its second: host uint32
 * [n_utts][n_cb * n_feat], 4 codewords packed best first. */
int ssw_first_pass_active_carry(ssw_model_t *m, int32_t n_utts, uint32_t *rows);
int32_t ssw_alignment_set_status(const ssw_alignment_set_t *a, int32_t utt);
const char *ssw_alignment_set_message(const ssw_alignment_set_t *a, int32_t utt);
/* each returns the number of entries and points the outputs (any may be NULL) at arrays owned
 * by the set: words -> dictionary ids; phones -> CI phone id and parent word index;
 * states -> senone id and parent phone = index / 3 */
int32_t ssw_alignment_set_words(const ssw_alignment_set_t *a, int32_t utt, const int32_t **wid,
                                const ssw_align_entry_t **al);
int32_t ssw_alignment_set_phones(const ssw_alignment_set_t *a, int32_t utt, const int32_t **cipid,
                                 const int32_t **parent, const ssw_align_entry_t **al);
int32_t ssw_alignment_set_states(const ssw_alignment_set_t *a, int32_t utt,
                                 const uint16_t **senid, const ssw_align_entry_t **al);
/* decoder_result_json(d, utt_start, align_level) for utterance `utt` of the set (align_level 1:
 * words and phones, 2: states too): "t" of the top level is the hypothesis string as
 * decoder_hyp builds it (base words, fillers left out), "d" the reference's decoder_n_frames
 * (the utterance's frames + 1) / frate, word texts are dictionary strings ("de(2)").  The
 * posterior of the first pass is not computed: top-level "p" is 1.000.  snprintf-style return;
 * -1 when the utterance has no alignment. */
int32_t ssw_alignment_set_json(const ssw_alignment_set_t *a, int32_t utt, double utt_start,
                               int32_t frate, int32_t align_level, char *out, int32_t out_len);
void ssw_alignment_set_free(ssw_alignment_set_t *a);

/* The graph ssw_first_pass_batch searches for one text, node by node (host only, works without
 * a device): the phone-tree HMMs of fsg_lextree_init with their entry penalty, predecessor,
 * FSG state and context sets.  flags: 1 word-initial, 2 word-final, 4 exit valid for every
 * right context, 8 / 16 / 32 member / first / last of a group of word-final HMMs that can never
 * differ (alternates pronounced alike).  beams[3] receives beam, pbeam, wbeam in score units.  Returns the node
 * count (which may exceed max_nodes: only max_nodes are written) or -1. */
typedef struct ssw_fp_node_s {
    uint16_t senid[3];
    int16_t tmat;
    int32_t pen, parent;
    uint32_t flags;
    int32_t ci_ext, state, to_state, wid;
    uint64_t ctxt;
} ssw_fp_node_t;
int32_t ssw_first_pass_graph(const ssw_model_t *m, const ssw_dict_t *d,
                             const ssw_first_pass_config_t *cfg, int32_t n_words,
                             const char *const *words, int32_t max_nodes, ssw_fp_node_t *nodes,
                             int32_t *beams);

/* decoder_result_json(d, utt_start, align_level >= 1) (src/decoder.c:1339-1593): the one-line
 * JSON the reference prints for an alignment, {"b","d","p","t","w":[...]} with b/d in seconds
 * (frames / frate) and p = logmath_exp(score).  hyp / hyp_logprob are the first pass's text
 * and posterior (decoder_hyp / decoder_prob: not part of this path, passed through).  Phones
 * must be grouped by ascending parent word, as ssw_alignment_populate writes them; pass
 * state_senid / state_al (3 per phone) for align_level 2, NULL for level 1.  Writes at most
 * out_len bytes (NUL-terminated) and returns the full length, snprintf-style; -1 on bad
 * arguments. */
int32_t ssw_alignment_json(const ssw_model_t *m, const char *hyp, int32_t hyp_logprob,
                           double utt_start, int32_t frate, int32_t n_frames, int32_t n_words,
                           const char *const *words, const ssw_align_entry_t *word_al,
                           int32_t n_phones, const int32_t *cipid, const int32_t *parent,
                           const ssw_align_entry_t *phone_al, const uint16_t *state_senid,
                           const ssw_align_entry_t *state_al, char *out, int32_t out_len);

/* ------------------------------------------------------------------------------------ */
/* Recognition against a word FSG: decoder_set_fsg + decoder_process_* + decoder_hyp /       */
/* decoder_seg_iter for a batch, over compallsen = yes scores.  Replaces:                     */
/*   fsg_model_init / _trans_add / _null_trans_add / _null_trans_closure, fsg_model_read      */
/*                                                 src/fsg_model.c:62-219, 453-708            */
/*   fsg_search_init: dictionary check, silences, alternates  src/fsg_search.c:84-253          */
/*   fsg_lextree_init with null transitions                  src/fsg_lextree.c:85-276, 356-660 */
/*   fsg_search_start / _null_prop / _word_trans / _step      src/fsg_search.c:543-802          */
/*   fsg_search_find_exit / _hyp / _seg_iter, fsg_seg_bp2itor src/fsg_search.c:854-1143         */
/* Not covered: JSGF imports and the three half-built grammars the reference searches after   */
/* logging an error (see ssw_jsgf_build_fsg), lattices / best path /                           */
/* N-best, tag transitions, grammars of more than 30000 phone-tree HMMs (up to there with     */
/* ssw_grammar_prepare_large, and in the default configuration, ssw_recognize_batch_active,    */
/* with ssw_grammar_prepare_large_active).                                                     */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_fsg_s ssw_fsg_t;
/* fsg_model_init + fsg_model_trans_add / fsg_model_null_trans_add per transition, in the order
 * given (src/fsg_model.c:62-148, 453-471; the reference's Python create_fsg): word[i] NULL or ""
 * makes transition i a null transition.  Refused, with the reference's message where it has one:
 * a state out of range ("Invalid from-state %d" / "Invalid to-state %d", :605-618), a
 * probability <= 0 or > 1 (:623-628), a word the dictionary lacks ("The word '%s' is missing in
 * the dictionary", src/fsg_search.c:120-141; d may be NULL: checked by ssw_grammar_prepare
 * then), a model of more than 64 CI phones.  The log probabilities, the null closure, the
 * silences and the alternates depend on lw, silprob, ... and are made by ssw_grammar_prepare. */
ssw_fsg_t *ssw_fsg_create(const ssw_model_t *m, const ssw_dict_t *d, const char *name,
                          int32_t n_states, int32_t start, int32_t final, int32_t n_trans,
                          const int32_t *from, const int32_t *to, const float *prob,
                          const char *const *word);
/* fsg_model_readfile (src/fsg_model.c:505-708): the .fsg text format -- FSG_BEGIN <name>,
 * NUM_STATES | N, START_STATE | S, FINAL_STATE | F, TRANSITION | T <from> <to> <prob> [<word>],
 * FSG_END; lines that start with '#', blank lines and lines with other first words are skipped;
 * a line's first word may be a prefix of the keyword, as in the reference.  Refusals as above,
 * plus its "... declaration missing" / "... declaration malformed" / "Line[%d]: ... missing". */
ssw_fsg_t *ssw_fsg_read(const ssw_model_t *m, const ssw_dict_t *d, const char *path);
void ssw_fsg_free(ssw_fsg_t *f);
const char *ssw_fsg_name(const ssw_fsg_t *f);
int32_t ssw_fsg_n_states(const ssw_fsg_t *f);
/* fsg_model_write (src/fsg_model.c:764-793) of the grammar as fsg_model_read leaves it
 * (searched = 0: null transitions closed) or as fsg_search_init does (searched = 1: silence and
 * filler loops and alternates added, src/fsg_search.c:229-233), the links in fsg_model_arcs
 * order (:248-302).  cfg NULL = defaults.  snprintf-style return; -1 on error. */
int32_t ssw_fsg_write(const ssw_fsg_t *f, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                      int32_t searched, char *out, int32_t out_len);
/* ------------------------------------------------------------------------------------ */
/* JSGF grammars: decoder_set_jsgf_string / decoder_set_jsgf_file (src/decoder.c:609-683).    */
/* Replaces, on the host (none of these calls touches the device):                            */
/*   the scanner and parser                       src/jsgf_scanner.l, src/jsgf_parser.y        */
/*   jsgf_define_rule, _kleene_new, _optional_new, the rule table  src/jsgf.c:173-205, 611-642 */
/*   jsgf_rule_iter, jsgf_get_rule, jsgf_get_public_rule           src/jsgf.c:423-481          */
/*   expand_rule / expand_rhs / jsgf_build_fsg                     src/jsgf.c:298-421, 483-539 */
/* Not covered: import (refused as unsupported); and, a deliberate difference, the grammars    */
/* whose expansion fails -- an undefined rule in a right-hand side, recursion that is not      */
/* right-recursion, <VOID>.  The reference logs the error, ignores it and searches what was    */
/* built up to there; here the build is refused with the reference's error text.              */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_jsgf_s ssw_jsgf_t;
/* jsgf_parse_string / jsgf_parse_file (src/jsgf.c:820-887).  NULL with the error set: a syntax
 * error ("... at line %d current token '%s'"), an import, a file that cannot be read ("Failed to
 * open %s for parsing").  Tags are parsed and dropped; a quoted token keeps its quotes. */
ssw_jsgf_t *ssw_jsgf_parse_string(const char *text);
ssw_jsgf_t *ssw_jsgf_parse_file(const char *path);
void ssw_jsgf_free(ssw_jsgf_t *j);
/* jsgf_grammar_name */
const char *ssw_jsgf_name(const ssw_jsgf_t *j);
/* jsgf_rule_iter / jsgf_rule_name / jsgf_rule_public: the rules, internal ones (<grammar.gNNNNN>)
 * included, index i in the order the reference's hash table walks them (src/hash_table.c) */
int32_t ssw_jsgf_n_rules(const ssw_jsgf_t *j);
const char *ssw_jsgf_rule_name(const ssw_jsgf_t *j, int32_t i);
int32_t ssw_jsgf_rule_public(const ssw_jsgf_t *j, int32_t i);
/* jsgf_get_public_rule (src/jsgf.c:444-469): the first public rule in that order, or -1 */
int32_t ssw_jsgf_public_rule(const ssw_jsgf_t *j);
/* jsgf_get_rule (:429-442): name is "grammar.rule", looked up as <grammar.rule>; index or -1 */
int32_t ssw_jsgf_find_rule(const ssw_jsgf_t *j, const char *name);
/* jsgf_build_fsg (:483-539): rule `rule` expanded, state number for state number; the grammar is
 * named after the rule, angle brackets included.  As in the reference the expansion divides the
 * leading weights of a rule's alternatives by their sum IN PLACE, so j changes: a second build
 * starts from the weights the first left.  d may be NULL, as for ssw_fsg_create.  Refused: the
 * three cases above ("Undefined rule in RHS: %s", "Only right-recursion is permitted (in %s.%s)"),
 * a weight that is not in (0, 1] after normalisation, a word the dictionary lacks. */
ssw_fsg_t *ssw_jsgf_build_fsg(const ssw_model_t *m, const ssw_dict_t *d, ssw_jsgf_t *j, int32_t rule);
/* decoder_set_jsgf_string / decoder_set_jsgf_file up to decoder_set_fsg (src/decoder.c:609-683):
 * toprule ("grammar.rule", the reference's -toprule) or, when NULL, the first public rule.
 * "Start rule %s not found", "No public rules found in input string" / "... in PATH". */
ssw_fsg_t *ssw_fsg_from_jsgf_string(const ssw_model_t *m, const ssw_dict_t *d, const char *text,
                                    const char *toprule);
ssw_fsg_t *ssw_fsg_from_jsgf_file(const ssw_model_t *m, const ssw_dict_t *d, const char *path,
                                  const char *toprule);

/* ssw_first_pass_graph for a grammar: the phone-tree HMMs fsg_lextree_init makes of it
 * (src/fsg_lextree.c:85-276, 356-660), host only. */
int32_t ssw_grammar_graph(const ssw_model_t *m, const ssw_dict_t *d,
                          const ssw_first_pass_config_t *cfg, const ssw_fsg_t *fsg,
                          int32_t max_nodes, ssw_fp_node_t *nodes, int32_t *beams);

/* decoder_set_fsg for n_fsgs grammars (src/decoder.c:596-607 -> fsg_search_init / _reinit,
 * src/fsg_search.c:171-307): the graphs are built once, on the host (no device call), and stay on the device
 * while the plan is the last one searched.  Refused: an unknown word, a grammar of more than
 * SSW_GRAMMAR_MAX_HMMS phone-tree HMMs or whose exchange arrays outgrow the workgroup's LDS
 * (the message names the count and the limit).  cfg NULL = defaults. */
#define SSW_GRAMMAR_MAX_HMMS 4096
typedef struct ssw_grammar_plan_s ssw_grammar_plan_t;
ssw_grammar_plan_t *ssw_grammar_prepare(const ssw_model_t *m, const ssw_dict_t *d,
                                        const ssw_first_pass_config_t *cfg, int32_t n_fsgs,
                                        const ssw_fsg_t *const *fsgs);
void ssw_grammar_plan_free(ssw_grammar_plan_t *plan);
/* phone-tree HMMs of grammar `fsg` of the plan (fsg_lextree_n_pnode), -1 when out of range */
int32_t ssw_grammar_plan_hmms(const ssw_grammar_plan_t *plan, int32_t fsg);
/* ssw_grammar_prepare for grammars of up to max_hmms phone-tree HMMs, with exchange arrays of
 * any size; max_hmms <= SSW_GRAMMAR_LARGE_MAX_HMMS, the reference's default maxhmmpf: beyond it
 * the reference narrows its beams frame by frame (src/fsg_search.c:376-394), which is not
 * rebuilt.  Refused, on the host: max_hmms beyond the ceiling, a grammar of more than max_hmms
 * HMMs (the message names the count and the limit), and what ssw_grammar_prepare refuses
 * otherwise (a grammar keeps at most 65535 states and entering-list entries).
 * The plan is opt-in because it costs.  A plan whose grammars all fit ssw_grammar_prepare's
 * limits is searched by the same kernels as a plan made there.  A plan that holds at least one
 * grammar beyond them is searched ENTIRELY by a kernel that keeps the HMMs and the exchange
 * arrays in a per-utterance HBM workspace (about 100 bytes per HMM and entering-list entry),
 * small grammars included, which the one-workgroup kernels hold in registers and search faster.  Its history tables
 * ((frames + 1) x entering-list entries x 8 bytes per utterance) are held to
 * SSW_GRAMMAR_HIST_BYTES by searching the call's utterances in groups, one launch after the other;
 * only an utterance that exceeds the budget alone is refused.  ssw_grammar_search_batch,
 * ssw_recognize_batch and the ssw_recognition_set_* readers take such a plan as any other;
 * ssw_recognize_batch_active refuses it, naming the grammar and its HMM count, unless it was made
 * by ssw_grammar_prepare_large_active below. */
#define SSW_GRAMMAR_LARGE_MAX_HMMS 30000
ssw_grammar_plan_t *ssw_grammar_prepare_large(const ssw_model_t *m, const ssw_dict_t *d,
                                              const ssw_first_pass_config_t *cfg, int32_t n_fsgs,
                                              const ssw_fsg_t *const *fsgs, int32_t max_hmms);
/* ssw_grammar_prepare_large -- the same checks, limits and messages -- for a plan that
 * ssw_recognize_batch_active takes as well where it holds a grammar beyond one workgroup: the
 * reference's DEFAULT configuration (compallsen = no) for grammars of up to max_hmms phone-tree
 * HMMs.  Per frame the senones of the HMMs in pnode_active are the ones scored
 * (fsg_search_sen_active, src/fsg_search.c:310-325, through acmod's flags2list with its bridges,
 * src/acmod.c:947-999) before fsg_search_step searches it (src/fsg_search.c:664-739); here the
 * HBM-workspace kernel writes those sets out, one bit per HMM and frame, and the rounds of
 * speculation and proof run over them as over a small plan's -- each round searches the
 * utterances not yet proven, history group by history group.  The sets take frames x
 * ceil(HMMs / 64) x 8 bytes per utterance, twice, for the whole call.  The flag changes nothing
 * in ssw_grammar_search_batch and ssw_recognize_batch, and a flagged plan whose grammars all fit
 * one workgroup is searched by the one-workgroup kernels in either configuration. */
ssw_grammar_plan_t *ssw_grammar_prepare_large_active(const ssw_model_t *m, const ssw_dict_t *d,
                                                     const ssw_first_pass_config_t *cfg,
                                                     int32_t n_fsgs, const ssw_fsg_t *const *fsgs,
                                                     int32_t max_hmms);
/* 1 for a plan made by ssw_grammar_prepare_large_active, 0 for any other, -1 for NULL */
int32_t ssw_grammar_plan_active(const ssw_grammar_plan_t *plan);
/* launches ssw_grammar_search_batch would search these utterances in (host only): 1 unless the
 * plan is on the HBM-workspace kernel and the history tables exceed the budget; 0 without
 * utterances; -1 where the call would be refused */
int32_t ssw_grammar_history_groups(const ssw_grammar_plan_t *plan, const int32_t *fsg_of_utt,
                                   const int32_t *utt_off, int32_t n_utts);

/* one history entry of the best path (fsg_seg_bp2itor, src/fsg_search.c:1032-1055) */
typedef struct ssw_fsg_seg_s {
    int32_t wid;  /* dictionary word id; -1 for a null transition ("(NULL)") */
    int32_t sf, ef; /* first and last frame; a null entry has sf = ef (-1 at the start state) */
    int32_t ascr; /* score - predecessor's score - lscr */
    int32_t lscr; /* the link's log probability >> 10 */
} ssw_fsg_seg_t;

/* decoder_start_utt .. decoder_end_utt of fsg_search for a batch (src/fsg_search.c:665-852):
 * utterance u (score rows utt_off[u] .. utt_off[u+1] of d_senscr, int16 [n_frames][n_sen] in
 * HBM) is searched against grammar fsg_of_utt[u] of the plan (NULL: grammar 0 for all).  NULL
 * on a call-level error, which includes a history table beyond SSW_GRAMMAR_HIST_BYTES (or the
 * environment's SSW_GRAMMAR_HIST_MB).  Per utterance (ssw_recognition_set_status): 0 a
 * hypothesis; 1 "Final result does not match the grammar in frame N" (fsg_search_find_exit,
 * :913-917); 2 no history entry at all (find_exit's "No hypothesis (yet)", :876-878).
 * Synchronous on `stream`. */
#define SSW_GRAMMAR_HIST_BYTES ((size_t)4 << 30)
typedef struct ssw_recognition_set_s ssw_recognition_set_t;
ssw_recognition_set_t *ssw_grammar_search_batch(ssw_model_t *m, const ssw_dict_t *d,
                                                const ssw_grammar_plan_t *plan,
                                                const int32_t *fsg_of_utt,
                                                const int16_t *d_senscr, int32_t n_frames,
                                                const int32_t *utt_off, int32_t n_utts,
                                                void *stream);
/* the same from FEATURES (d_feats float32 [n_frames][39]): ssw_score_batch of all senones into
 * a workspace the model keeps (acmod_score with compallsen = yes), then the search */
ssw_recognition_set_t *ssw_recognize_batch(ssw_model_t *m, const ssw_dict_t *d,
                                           const ssw_grammar_plan_t *plan,
                                           const int32_t *fsg_of_utt, int scorer,
                                           const float *d_feats, int32_t n_frames,
                                           const int32_t *utt_off, int32_t n_utts, void *stream);
/* ssw_recognize_batch in the reference's DEFAULT configuration (compallsen = no): what a caller
 * of decoder_set_fsg, decoder_process_int16 and decoder_hyp gets from an unmodified library.
 * Replaces, per frame, fsg_search_sen_active (src/fsg_search.c:310-325: the senones of the HMMs
 * in pnode_active are the ones acmod scores), acmod's flags2list with its bridge entries
 * (src/acmod.c:947-999) in front of the scorer, and fsg_search_step (src/fsg_search.c:664-739),
 * for a batch, by the speculation and proof ssw_first_pass_batch_active describes above: the
 * sets of active HMMs are assumed, the batch is scored with them, searched, and an utterance
 * whose search took the assumed sets frame for frame is the reference's search.  Hypotheses,
 * scores and segments are those of the default configuration (the texts are the compallsen = yes
 * ones on the reference's recordings, every score differs).  Limits as
 * ssw_first_pass_batch_active: 3-state HMMs, <= 64 codebooks, ds = 1 with the PTM scorer, the
 * per-frame kernels' LDS against the plan's largest grammar; refused with a message otherwise,
 * as is a plan with a grammar beyond one workgroup that ssw_grammar_prepare_large_active did not
 * make.
 *   d_senscr  NULL, or device int16 [n_frames][n_sen]: the rows as acmod's buffer would hold
 *             them (ssw_grammar_search_batch over them gives the same set)
 *   listed    NULL, or host uint32 [n_frames][(n_sen + 31) / 32]: the proven listed senones of
 *             every frame, bridges included
 *   rounds    NULL, or host int32 [n_utts]: searches over default-configuration scores the
 *             utterance took (1: its first assumption was proven; 0 only for a call without
 *             utterances)
 * The set is read through the ssw_recognition_set_* calls below.  Synchronous on `stream`. */
ssw_recognition_set_t *ssw_recognize_batch_active(ssw_model_t *m, const ssw_dict_t *d,
                                                  const ssw_grammar_plan_t *plan,
                                                  const int32_t *fsg_of_utt, int scorer,
                                                  const float *d_feats, int32_t n_frames,
                                                  const int32_t *utt_off, int32_t n_utts,
                                                  int16_t *d_senscr, uint32_t *listed,
                                                  int32_t *rounds, void *stream);
/* ssw_first_pass_active_stats for ssw_recognize_batch_active: [0] utterances searched that way
 * since ssw_model_load, [1] their rounds summed, [2] rounds of the last call, [3] utterances
 * that needed more than one */
int ssw_grammar_active_stats(ssw_model_t *m, int64_t stats[4]);
int32_t ssw_recognition_set_status(const ssw_recognition_set_t *r, int32_t utt);
const char *ssw_recognition_set_message(const ssw_recognition_set_t *r, int32_t utt);
/* decoder_seg_iter (src/fsg_search.c:1084-1142): the path's entries, null transitions
 * included; returns their number (0 without a hypothesis) and points *seg at the set's array */
int32_t ssw_recognition_set_segments(const ssw_recognition_set_t *r, int32_t utt,
                                     const ssw_fsg_seg_t **seg);
/* decoder_hyp's score (fsg_search_hyp, src/fsg_search.c:935-1030): 0, or -1 without a hypothesis */
int32_t ssw_recognition_set_score(const ssw_recognition_set_t *r, int32_t utt, int32_t *score);
/* decoder_hyp's text: base words, fillers and null transitions left out.  snprintf-style;
 * -1 without a hypothesis (also when every entry is a filler or null: hyp_str NULL, :999-1002) */
int32_t ssw_recognition_set_hyp(const ssw_recognition_set_t *r, int32_t utt, char *out,
                                int32_t out_len);
/* decoder_result_json(d, utt_start, 0) (src/decoder.c:1339-1379, 1502-1593): the line with
 * its newline; a word's p = logmath_exp(ascr + lscr), top-level p 1.000 (decoder_prob is 0
 * without bestpath), "(NULL)" entries included, "t":"","w":[] without a hypothesis. */
int32_t ssw_recognition_set_json(const ssw_recognition_set_t *r, int32_t utt, double utt_start,
                                 int32_t frate, char *out, int32_t out_len);
void ssw_recognition_set_free(ssw_recognition_set_t *r);

/* decoder_result_json(d, start, 1 or 2) after a grammar: decoder_alignment (src/decoder.c:737-798)
 * for every utterance of a recognition set.  The best path's entries are walked in order
 * (decoder_seg_iter); an entry whose word is no dictionary word ("(NULL)", wid < 0) is skipped
 * (:759-761); every other one, fillers and alternate pronunciations included, is
 * alignment_add_word(wid, sf, ef - sf + 1), the windows as they are (the contiguity assert of
 * :763 is compiled out of a release build); then alignment_populate (:769), the state alignment
 * constrained to those windows (state_align_search_init / step / finish, :777-795) and
 * alignment_propagate.  The set is read with the ssw_alignment_set_* calls; per utterance:
 *   0  aligned
 *   1  no hypothesis (decoder_seg_iter NULL, :753-755; recognition status 1 or 2): the
 *      recognition set's message, e.g. "Final result does not match the grammar in frame N"
 *   2  alignment_populate or the second pass failed; also a path without a dictionary word on it
 *      (null transitions only), with a message saying so -- no equality with the reference is
 *      claimed for that one
 * and the other utterances of the batch are aligned all the same.  ssw_alignment_set_json of
 * such a set prints decoder_hyp's text -- the recognition set's hypothesis, which follows the
 * GRAMMAR's filler marking -- as the top-level "t".
 *
 * ssw_recognition_set_align: over whole rows in HBM (d_senscr int16 [n_frames][n_sen], the rows
 * the search read: compallsen = yes); follows ssw_grammar_search_batch or ssw_recognize_batch.
 * NULL with a message for a set made with another model or frame counts that are not the set's. */
ssw_alignment_set_t *ssw_recognition_set_align(ssw_model_t *m, const ssw_recognition_set_t *r,
                                               const int16_t *d_senscr, int32_t n_frames,
                                               const int32_t *utt_off, void *stream);
/* ssw_recognize_batch, then ssw_recognition_set_align over the same rows.  two_pass_history (PTM
 * and s2_semi scorers): the rows are made again between the two searches from the top-N order
 * every utterance's own search left, as ssw_align_text_batch does (src/decoder.c:786-793,
 * src/ptm_mgau.c:425-448).  rec_out: NULL, or receives the recognition set, equal in every
 * accessor to ssw_recognize_batch's for the same input; the caller frees both sets. */
ssw_alignment_set_t *ssw_recognize_align_batch(ssw_model_t *m, const ssw_dict_t *d,
                                               const ssw_grammar_plan_t *plan,
                                               const int32_t *fsg_of_utt, int scorer,
                                               const float *d_feats, int32_t n_frames,
                                               const int32_t *utt_off, int32_t n_utts,
                                               int32_t two_pass_history,
                                               ssw_recognition_set_t **rec_out, void *stream);
/* The same in the reference's DEFAULT configuration (compallsen = no): ssw_recognize_batch_active,
 * then the second pass scoring for itself as ssw_align_batch_active_ex does, its active set
 * seeded with acmod's flags after the grammar search's last frame (no bridges) and only growing
 * from there (src/state_align_search.c:186-189); with two_pass_history (PTM) it starts from the
 * orders the search left in history slot 1.  The s2_semi scorer takes the whole-rows route, as
 * in every *_active call; a continuous model is refused by name until
 * ssw_model_enable_active was called on it, and is then served by its listed-senone kernel
 * (two_pass_history is ignored for it, as for ms: that scorer keeps no history).  Limits and refusals as
 * ssw_recognize_batch_active (a plan with a grammar beyond one workgroup must come from
 * ssw_grammar_prepare_large_active) and ssw_align_batch_active_ex, reported under this name.
 * rounds as ssw_recognize_batch_active's. */
ssw_alignment_set_t *ssw_recognize_align_batch_active(ssw_model_t *m, const ssw_dict_t *d,
                                                      const ssw_grammar_plan_t *plan,
                                                      const int32_t *fsg_of_utt, int scorer,
                                                      const float *d_feats, int32_t n_frames,
                                                      const int32_t *utt_off, int32_t n_utts,
                                                      int32_t two_pass_history,
                                                      ssw_recognition_set_t **rec_out,
                                                      int32_t *rounds, void *stream);

/* ------------------------------------------------------------------------------------ */
/* Dynamic features on the device: feat_s2mfc2feat_live for whole    */
/* utterances with feat = 1s_c_d_dd, cmn = batch ("current"), no varnorm / agc / lda       */
/* (src/feat.c:977-1008, 589-632; src/cmn.c:168-200).  d_cep [n_frames][ncep] MFCC rows     */
/* -> d_out [n_frames][3*ncep] = cep | delta | delta-delta, i.e. the 0-12/13-25/26-38       */
/* stream split the scorers read.  Bit-exact float32, synchronous on `stream`.            */
/* ------------------------------------------------------------------------------------ */
int ssw_feat_batch(ssw_model_t *m, const float *d_cep, int32_t n_frames,
                   const int32_t *utt_off, int32_t n_utts, int32_t ncep, float *d_out,
                   void *stream);

/* ------------------------------------------------------------------------------------ */
/* Dynamic features as the model's feat_params.json says: every configuration that          */
/* feat_init_s3file accepts and feat_s2mfc2feat_block_utt computes for whole utterances     */
/* (src/feat.c:732-927, :977-1008; src/cmn.c:159-224; src/cmn_live.c:60-134;                */
/* src/lda.c:84-144).  Bit-exact float32.  Streaming calls (an utterance in pieces), an     */
/* LDA over several streams and AGC (the reference has none) are out of scope.              */
/* ------------------------------------------------------------------------------------ */
enum ssw_cmn { SSW_CMN_NONE = 0, SSW_CMN_BATCH = 1, SSW_CMN_LIVE = 2 };
/* the settings of config_defs.h FEAT_OPTIONS (include/soundswallower/config_defs.h:418-450);
 * defaults are the reference's.  An empty string is an unset (NULL) setting. */
typedef struct ssw_feat_config_s {
    char feat[64];      /* "feat"     1s_c_d_dd */
    int32_t ceplen;     /* "ceplen"   13 (0 reads as 13, src/feat.c:741-742) */
    int32_t cmn;        /* "cmn"      live (enum ssw_cmn; batch = current, live = prior) */
    int32_t varnorm;    /* "varnorm"  no */
    int32_t ldadim;     /* "ldadim"   0 = every row of the matrix */
    int32_t from_file;  /* ssw_model_feat_config: 1 when feat_params.json was read */
    char cmninit[512];  /* "cmninit"  40,3,-1 */
    char lda[1024];     /* "lda"      path of the feature transform; ssw_model_feat_config: unset =
                         *            the file feature_transform beside the means file, if there
                         *            is one (src/decoder.c:90-119) */
    char svspec[512];   /* "svspec"   e.g. 24,0-11/25,12-23/26-38 */
} ssw_feat_config_t;
void ssw_feat_config_defaults(ssw_feat_config_t *cfg);
/* the FEAT_OPTIONS keys of a feat_params.json over *cfg (which holds the defaults): 0 read,
 * 1 no such file, -1 unusable (ssw_last_error: bad JSON, an unknown cmn, a value of the
 * wrong type) */
int ssw_feat_config_read(const char *path, ssw_feat_config_t *cfg);
/* What ssw_model_load read from the model directory's feat_params.json, over the defaults
 * (from_file says whether there was one).  0, or -1 on NULL. */
int ssw_model_feat_config(const ssw_model_t *m, ssw_feat_config_t *out);

/* A resolved configuration with its device tables (feature recipe, LDA matrix, subvector
 * gather).  cfg NULL = the model's own.  The type is resolved by feat_init_s3file's chain of
 * comparisons, in its order: s2_4x; s3_1x39 / 1s_12c_12d_3p_12dd; the prefixes 1s_c_d_dd,
 * 1s_c_d_ld_dd, cep_dcep / 1s_c_d, cep / 1s_c, 1s_3c / 1s_4c; else the generic
 * "n,n,...[:window]".  Refused by name, before anything is uploaded, with the reference's own
 * reason where it has one: LDA or svspec with more than one stream; a matrix whose width is not
 * the stream's; varnorm with cmn = live; s2_4x / s3_1x39 with ceplen != 13; a malformed generic
 * type or svspec; an unreadable or corrupt matrix file; and this implementation's limits:
 * ceplen 1..64, window <= 8, at most 8 streams, at most 256 LDA rows, svspec dimensions below
 * the raw dimension.  NULL on error (ssw_last_error). */
typedef struct ssw_feat_s ssw_feat_t;
ssw_feat_t *ssw_feat_create(ssw_model_t *m, const ssw_feat_config_t *cfg);
void ssw_feat_free(ssw_feat_t *f);
int32_t ssw_feat_out_dim(const ssw_feat_t *f);  /* floats per output row */
int32_t ssw_feat_raw_dim(const ssw_feat_t *f);  /* before LDA and svspec: the stream lengths' sum */
int32_t ssw_feat_window(const ssw_feat_t *f);
int32_t ssw_feat_n_streams(const ssw_feat_t *f); /* feat_dimension1: subvectors, else streams */
/* feat_dimension2 of stream i (the LDA's rows, a subvector's length, the stream's); -1 */
int32_t ssw_feat_stream_len(const ssw_feat_t *f, int32_t i);
int32_t ssw_feat_tile_frames(const ssw_feat_t *f); /* frames one workgroup computes */
/* live CMN's running estimate (cmn_t: cmn_mean, sum, nframe), host memory */
typedef struct ssw_cmn_state_s {
    float mean[64], sum[64];
    int32_t nframe;
} ssw_cmn_state_t;
/* the state of a fresh decoder: cmninit as cmn_set_repr reads it (src/cmn.c:112-140; values
 * beyond the list stay 0, nframe 500), all zeros without a cmninit or with cmn = none */
int ssw_feat_cmn_prior(const ssw_feat_t *f, ssw_cmn_state_t *out);
/* d_cep [n_frames][ncep] (ncep must be the configuration's ceplen) -> d_out
 * [n_frames][ssw_feat_out_dim], utterance u = frames utt_off[u] .. utt_off[u + 1] (host int32
 * [n_utts + 1], non-decreasing from 0 to n_frames).  cmn_state, with cmn = live only:
 *   NULL      every utterance is the first of a fresh decoder (the prior is cmninit);
 *   non-NULL  in/out: the batch's utterances are one decoder's, in order -- after each come
 *             cmn_live's shift (nframe > 800, src/cmn_live.c:131-133) and cmn_live_update
 *             (src/feat.c:944-945; an empty utterance gets the update alone).
 * With cmn = batch or none the state is neither read nor written.  feat NULL = a
 * configuration the model builds once from its own settings and keeps.  Synchronous on
 * `stream`; 0, or -1 (ssw_last_error). */
int ssw_feat_batch_ex(ssw_model_t *m, ssw_feat_t *feat, const float *d_cep, int32_t n_frames,
                      const int32_t *utt_off, int32_t n_utts, int32_t ncep, float *d_out,
                      ssw_cmn_state_t *cmn_state, void *stream);

/* ------------------------------------------------------------------------------------ */
/* MFCC front end on the device: 16-bit PCM -> cepstra for  */
/* whole utterances, as fe_start + fe_process_int16 over all samples + fe_end compute them */
/* (src/fe_interface.c:86-330, :560-690; src/fe_sigproc.c:70-738; src/fe_noise.c:111-327). */
/* Bit-exact float32.  Streaming calls (fe_process_int16 in pieces) are out of scope.      */
/* ------------------------------------------------------------------------------------ */
/* the front-end settings of config_defs.h FE_OPTIONS (include/soundswallower/config_defs.h:
 * 299-412) that ssw_fe_batch reads; defaults are the reference's */
enum ssw_fe_transform { SSW_FE_LEGACY = 0, SSW_FE_DCT = 1, SSW_FE_HTK = 2 };
typedef struct ssw_fe_config_s {
    double samprate;      /* "samprate"      16000 */
    double wlen;          /* "wlen"          0.025625 */
    double alpha;         /* "alpha"         0.97 */
    double lowerf;        /* "lowerf"        133.33334 */
    double upperf;        /* "upperf"        6855.4976 */
    int32_t frate;        /* "frate"         100 */
    int32_t nfft;         /* "nfft"          0 = from the window (512 at 16 kHz) */
    int32_t ncep;         /* "ncep"          13 */
    int32_t nfilt;        /* "nfilt"         40 */
    int32_t lifter;       /* "lifter"        0 */
    int32_t transform;    /* "transform"     legacy (enum ssw_fe_transform) */
    int32_t remove_noise; /* "remove_noise"  no */
    int32_t unit_area;    /* "unit_area"     yes */
    int32_t round_filters;/* "round_filters" yes */
    int32_t dither;       /* "dither"        no */
    int32_t remove_dc;    /* "remove_dc"     no */
    int32_t doublebw;     /* "doublebw"      no */
    int32_t smoothspec;   /* "smoothspec"    no */
    int32_t logspec;      /* "logspec"       no */
    int32_t warp;         /* 1 when "warp_params" is given (frequency warping) */
    int32_t from_file;    /* ssw_model_fe_config: 1 when feat_params.json was read */
} ssw_fe_config_t;
void ssw_fe_config_defaults(ssw_fe_config_t *cfg);
/* What ssw_model_load read from feat_params.json beside the `means` file (the model
 * directory; acmod reads the same file, src/config.c:441-510 parses it), over the defaults;
 * the feature stage's keys (feat, ceplen, cmn, cmninit, varnorm, lda, ldadim, svspec) are left
 * to ssw_model_feat_config, every other unknown key is ignored.  0, or -1 on NULL. */
int ssw_model_fe_config(const ssw_model_t *m, ssw_fe_config_t *out);
/* Frames the front end makes of n_samples samples at 16 kHz (fe_process_int16 + fe_end,
 * src/fe_interface.c:560-690): 0 for 0 samples, 1 below one window (410 samples), else
 * 2 + (n - 410) / 160 -- the last is fe_end's zero-padded overflow frame.  -1 on error. */
int64_t ssw_fe_frame_count(const ssw_model_t *m, int64_t n_samples);
/* The front end for a batch of utterances: d_pcm int16 in HBM, utterance u = samples
 * samp_off[u] .. samp_off[u + 1] (host int64 [n_utts + 1], samp_off[0] = 0) -> d_cep float32
 * [total frames][ncep] in HBM, frame_off_out host int32 [n_utts + 1] (ready for
 * ssw_feat_batch).  Every utterance starts afresh (fe_start_utt: pre-emphasis and noise
 * tracker reset).  cfg NULL = the model's feat_params.json.  Supported: samprate 16000,
 * frate 100, wlen 0.025625, nfft 0 or 512, ncep 13, alpha 0.97, transform legacy or dct,
 * nfilt 1..64 with every filter at least one DFT point wide, 0 <= lowerf < upperf <=
 * samprate / 2, any lifter >= 0, remove_noise yes / no, unit_area and round_filters yes;
 * anything else (htk, dither, remove_dc, doublebw, smoothspec, logspec, warping, other
 * rates) is refused with an error.  Tables (fe_create_hamming, fe_build_melfilters,
 * fe_compute_melcosine, fe_create_twiddle, the lifter) are built on the host with libm and
 * uploaded once per configuration.  Synchronous on `stream`; 0, or -1 (ssw_last_error). */
int ssw_fe_batch(ssw_model_t *m, const ssw_fe_config_t *cfg, const int16_t *d_pcm,
                 const int64_t *samp_off, int32_t n_utts, float *d_cep, int32_t *frame_off_out,
                 void *stream);
/* ssw_fe_batch at each utterance's own sample rate, as the reference computes cepstra at the
 * rate the audio has (fe_init, src/fe_interface.c:55-160, 255-301): utterance u is at
 * samprate[u] Hz (host double [n_utts]; NULL = cfg->samprate for all; cfg NULL = the model's
 * feat_params.json).  One batch may mix rates.  Per rate, as fe_init derives them:
 *   samprate     whole hertz (an integer setting, config_defs.h:320-323); 0 = the lowest of
 *                8000, 11025, 16000, 22050, 32000, 44100, 48000 that is at least
 *                (int)(2 upperf) (minimum_samprate, src/fe_interface.c:66-81)
 *   frame shift  (int)(samprate / frate + 0.5), frame size (int)(wlen samprate + 0.5), in float
 *   nfft         0 = per utterance, the smallest power of 2 >= (int)(wlen samprate); else that
 *                power of 2 for every utterance, at least every utterance's window
 * Refused, naming the reason, as fe_init refuses them: frate < 1, > samprate or > 32767; a
 * frame shift <= 1; a frame size below the shift; an nfft that is not a power of 2 or is below
 * the window; upperf > samprate / 2 + 1 (src/fe_interface.c:299-301).  This front end's own
 * limit: FFTs of 64 .. 8192 points (8 kHz at 256 up to 192 kHz at 8192 with the default
 * window).  Refused as by ssw_fe_batch: a mel filter narrower than one DFT point (the reference
 * makes NaN cepstra of it), htk, dither, remove_dc, doublebw, smoothspec, logspec, warping,
 * ncep != 13, alpha != 0.97, unit_area or round_filters off.  A bad entry anywhere in
 * samprate[] refuses the whole call before any launch, with nothing written.  frame_off_out,
 * d_cep and the rest as ssw_fe_batch; at 16000 Hz the cepstra are ssw_fe_batch's, byte for
 * byte.  Tables that depend on the rate are built per distinct (samprate, nfft) and uploaded
 * once per configuration and rate.  Synchronous on `stream`; 0, or -1 (ssw_last_error). */
int ssw_fe_batch_ex(ssw_model_t *m, const ssw_fe_config_t *cfg, const int16_t *d_pcm,
                    const int64_t *samp_off, const double *samprate, int32_t n_utts,
                    float *d_cep, int32_t *frame_off_out, void *stream);
/* ssw_fe_batch_ex for float32 samples: what fe_process_float32 over all samples + fe_end
 * compute (src/fe_interface.c:578-712, src/fe_sigproc.c:350-376, 413-444).  Every argument,
 * refusal, frame count, per-utterance rate and table as ssw_fe_batch_ex; the sample type is the
 * one difference.  The reference keeps its sample buffer in float32, spch[i] = sample *
 * 32768.0F (FLOAT32_SCALE, include/soundswallower/fe.h:370), and fe_end's overflow frame is
 * the raw floats scaled the same way (create_overflow_frame, src/fe_interface.c:503-510), so
 * every sample, and the prior sample of a frame, enters pre-emphasis as
 * (double)(float)(x * 32768.0f).  The product is by a power of two and therefore exact, for
 * subnormal products too, except where it overflows to infinity.  Everything after that point
 * is the int16 path's code.  The cepstra equal the reference's for finite samples of any
 * magnitude: values outside [-1, 1) are not clipped, +-0 gives 0, x / 32768 of int16 audio gives
 * ssw_fe_batch_ex's bytes.  For a non-finite sample the call is deterministic and does not
 * fault, no address is computed from a sample, and the frames whose window and prior sample
 * hold none are as without it (with remove_noise the tracker carries it forward). */
int ssw_fe_batch_f32(ssw_model_t *m, const ssw_fe_config_t *cfg, const float *d_pcm,
                     const int64_t *samp_off, const double *samprate, int32_t n_utts,
                     float *d_cep, int32_t *frame_off_out, void *stream);
/* Frames ssw_fe_batch_ex makes of n_samples samples at samprate Hz (one entry of its
 * samprate[]; cfg NULL = feat_params.json): 0 for 0 samples, 1 below one window, else the full
 * frames 1 + (n - size) / shift and fe_end's frame of the samples left over (src/fe_interface.c:
 * 560-712; 2 + (n - size) / shift whenever size > shift).  -1 on error, as ssw_fe_batch_ex
 * refuses the settings. */
int64_t ssw_fe_frame_count_ex(const ssw_model_t *m, const ssw_fe_config_t *cfg,
                              double samprate, int64_t n_samples);
/* measurement aid: with ssw_set_kernel_timing on, the last ssw_fe_batch(_ex, _f32, _any) call's
 * milliseconds per kernel -- ms[0] spectrum (framing, FFT, mel; every FFT size's launch),
 * ms[1] noise removal (0 when off), ms[2] log, DCT and lifter.  0, or -1 when no timed call
 * has been made. */
int ssw_fe_kernel_timing(ssw_model_t *m, float ms[3]);

/* ------------------------------------------------------------------------------------ */
/* The front end in every configuration fe_init accepts (src/fe_interface.c:84-330,        */
/* src/fe_sigproc.c:70-738, src/fe_warp.c, src/fe_warp_inverse_linear.c,                   */
/* src/fe_warp_affine.c, src/fe_warp_piecewise_linear.c).  ssw_fe_batch, _ex and _f32 above */
/* keep their family of settings and their refusals; these take the rest.  Bit-exact       */
/* float32 against fe_process_int16 / fe_process_float32 over all samples + fe_end.        */
/* ------------------------------------------------------------------------------------ */
/* A resolved configuration: ssw_fe_config_t with the two settings that are strings,
 * "warp_type" (inverse_linear, affine or piecewise_linear; NULL = inverse_linear, the default)
 * and "warp_params" (NULL or "" = no warping).  cfg NULL = the model's feat_params.json with the
 * warp strings it read there (a non-NULL string still overrides).  Host work only: the settings
 * are checked and the warp parameters parsed as each type's set_parameters parses them (atof of
 * blank-separated tokens, one for inverse_linear, two for the others, the rest ignored; slope 0 =
 * no warping; piecewise_linear's F = 0 means 0.85 samprate) and kept in the ssw_fe_t -- the
 * reference keeps them in process-wide statics.  Accepted besides what ssw_fe_batch_ex takes:
 *   alpha          any finite float32; 0 copies the samples (fe_copy_to_frame,
 *                  src/fe_sigproc.c:297-309), which differs from a product by 0 for a
 *                  non-finite float32 sample
 *   remove_dc      after pre-emphasis and zero padding the mean of the frame_size doubles, summed
 *                  in index order with the zeros of a short last frame, is subtracted, then the
 *                  window applied (fe_hamming_window, :277-285)
 *   transform htk  fe_dct2 with C0 scaled by sqrt_inv_2n (:677-699); the lifter follows
 *   ncep           1 .. 64; it may exceed nfilt
 *   logspec        rows of nfilt floats, (float)log(mfspec + 1e-4); no lifter
 *   smoothspec     rows of nfilt floats, fe_dct2 then fe_dct3 (:714-726); wins over logspec
 *   doublebw, unit_area = no, round_filters = no   fe_build_melfilters (:85-199)
 *   warping        fe_mel and fe_melinv through the warping function; a warped frequency above
 *                  Nyquist only makes the reference warn, and is used here as there
 * Refused, naming the reason: dither (its random stream belongs to a process's lifetime); with
 * cfg NULL, a feat_params.json whose input_endian is not the host's; a warp_type that is none of
 * the three ("Unimplemented warping function ..."); cfg->warp set without warp_params; ncep or
 * nfilt outside 1 .. 64; a negative lifter; lowerf < 0 or >= upperf.  At the first rate where it
 * shows, ssw_fe_batch_any and ssw_fe_frames refuse what ssw_fe_batch_ex refuses of framing and
 * filters (a filter with no DFT point, or narrower than one), and a doublebw bank whose outer
 * edges fall below 0 or above Nyquist -- a deliberate difference: the reference warns there and
 * goes on without a filter bank.  NULL on error (ssw_last_error). */
typedef struct ssw_fe_s ssw_fe_t;
ssw_fe_t *ssw_fe_create(ssw_model_t *m, const ssw_fe_config_t *cfg, const char *warp_type,
                        const char *warp_params);
void ssw_fe_free(ssw_fe_t *fe);
/* fe_get_output_size: floats per row, ncep, or nfilt with logspec / smoothspec.  -1 on NULL. */
int32_t ssw_fe_out_dim(const ssw_fe_t *fe);
/* ssw_fe_frame_count_ex for a resolved configuration */
int64_t ssw_fe_frames(const ssw_fe_t *fe, double samprate, int64_t n_samples);
/* ssw_fe_batch_ex (sample_type 0: d_pcm int16) or ssw_fe_batch_f32 (1: float32) under fe's
 * settings: every other argument as there, d_cep float32 [total frames][ssw_fe_out_dim(fe)].
 * Tables that depend on the rate -- warping depends on the Nyquist frequency -- are built per
 * distinct (fe's settings, samprate, nfft) at the first call that needs them.  A configuration
 * that ssw_fe_batch_ex takes runs its kernels and gives its bytes.  With remove_dc the frame's
 * sum is the reference's: a parallel reduction where the host proves from alpha's bit pattern,
 * the frame size and the sample type that no order of summing rounds (int16 samples and, e.g.,
 * alpha 0.97 at any supported frame size), else a sum in index order (float32 samples; int16
 * with an alpha on a fine grid, such as 0.001).  0, or -1 (ssw_last_error). */
int ssw_fe_batch_any(ssw_model_t *m, ssw_fe_t *fe, const void *d_pcm, int32_t sample_type,
                     const int64_t *samp_off, const double *samprate, int32_t n_utts,
                     float *d_cep, int32_t *frame_off_out, void *stream);
/* 1 when ssw_fe_batch_ex takes the settings of the model's feat_params.json (no warping, the
 * host's input_endian) or reports why that file cannot be used, 0 when only ssw_fe_batch_any
 * takes them; -1 on NULL */
int ssw_model_fe_plain(const ssw_model_t *m);
/* "warp_type" and "warp_params" as ssw_model_load read them from feat_params.json
 * ("inverse_linear" and "" when absent; "warp_params": "" or null reads as ""), truncated to the
 * buffers.  0, or -1 on bad arguments. */
int ssw_model_fe_warp(const ssw_model_t *m, char *type, int32_t type_len, char *params,
                      int32_t params_len);

/* ------------------------------------------------------------------------------------ */
/* Multi-GPU (NEW: the reference is single-process).  The path shards by utterance -- one   */
/* process per GPU, the model replicated, no exchange while scoring and aligning -- and the  */
/* only collective is ONE gather of the final alignment entries over RCCL (xGMI inside a      */
/* node).  What is gathered is the state level of alignment_t (include/soundswallower/         */
/* alignment.h:60-109) as ssw_align_batch returns it; alignment_propagate then runs wherever   */
/* the word / phone levels are wanted.  RCCL is bound at run time, so single-GPU hosts do not  */
/* need it installed.                                                                          */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_comm_s ssw_comm_t;
#define SSW_COMM_ID_BYTES 128
/* ncclGetUniqueId: called by ONE rank, which hands the 128 bytes to the others by whatever
 * channel the host has (MPI, a file, torch.distributed ...) */
int ssw_comm_unique_id(char id[SSW_COMM_ID_BYTES]);
/* ncclCommInitRank on `device`; collective over the n_ranks callers */
ssw_comm_t *ssw_comm_init(const char id[SSW_COMM_ID_BYTES], int32_t n_ranks, int32_t rank,
                          int32_t device);
/* wrap a communicator the host already has (an ncclComm_t); not destroyed by ssw_comm_free */
ssw_comm_t *ssw_comm_from_nccl(void *nccl_comm, int32_t n_ranks, int32_t rank, int32_t device);
/* A host with a transport of its own (MPI_Allgather, a test double): `fn` must deliver, on
 * every rank, the n_int32_per_rank words each rank passes in `send` to recv[r * n_int32_per_rank
 * ..] for r = 0 .. n_ranks - 1 (host memory on both sides) and return 0.  ssw_gather_alignments
 * then pads, exchanges and unpacks through it without touching RCCL or HIP. */
typedef int (*ssw_all_gather_fn)(void *ctx, const void *send, void *recv, size_t n_int32_per_rank);
ssw_comm_t *ssw_comm_from_transport(ssw_all_gather_fn fn, void *ctx, int32_t n_ranks, int32_t rank);
void ssw_comm_free(ssw_comm_t *c);
/* Collective.  local: this rank's n_local entries (the state entries of its utterances, in its
 * shard's order); counts [n_ranks]: entries of every rank -- known to all of them, being a
 * function of the transcripts and the shard plan; out [sum(counts)]: all entries in rank order,
 * on every rank (host memory).  One padded ncclAllGather; synchronous on `stream`. */
int ssw_gather_alignments(ssw_comm_t *c, const ssw_align_entry_t *local, int32_t n_local,
                          const int32_t *counts, ssw_align_entry_t *out, void *stream);
/* ncclCommCount of the communicator (the ranks RCCL itself says it spans); n_ranks of a host
 * transport.  -1 on error. */
int32_t ssw_comm_count(ssw_comm_t *c);

/* device-memory helpers so a C caller needs no HIP headers */
void *ssw_device_malloc(size_t nbytes);
void ssw_device_free(void *d_ptr);
/* free and total memory of the current device (hipMemGetInfo): a job sizes what it keeps
 * resident by it (soundswallower_amd/jobs.py) */
int ssw_device_mem_info(size_t *free_bytes, size_t *total_bytes);
int ssw_memcpy_h2d(void *d_dst, const void *src, size_t nbytes);
int ssw_memcpy_d2h(void *dst, const void *d_src, size_t nbytes);
int ssw_device_synchronize(void);
/* independent (non-blocking) streams for the `stream` arguments above, e.g. to score the next
 * chunk of a job while ssw_align_batch works through the previous one */
void *ssw_stream_create(void);
void ssw_stream_destroy(void *stream);
int ssw_stream_synchronize(void *stream);

/* ------------------------------------------------------------------------------------ */
/* Voice activity detection and endpointing for batches of audio streams (vad.h,          */
/* endpointer.h: src/ps_vad.c, src/ps_endpointer.c over src/common_audio/vad/ and          */
/* src/common_audio/signal_processing/).  All of it is integer arithmetic, so the           */
/* decisions EQUAL the reference's.  No model is involved: the object owns its workspace.  */
/* ------------------------------------------------------------------------------------ */
typedef struct ssw_vad_s ssw_vad_t;
/* vad_init + vad_set_input_params (src/ps_vad.c:49-128).  mode 0..3 (vad_mode_t; another is
 * refused: "Invalid VAD mode %d").  sample_rate 0 = 16000, frame_length 0 = 0.03 s.  The
 * detector works at the rate r of 8000, 16000, 32000, 48000 with the smallest |1 - r /
 * sample_rate| below 0.5 ("No suitable sampling rate found for %d" when there is none), on
 * frames of (size_t)(r * frame_length) samples OF THE CALLER'S AUDIO, which must be 10, 20 or
 * 30 ms at r ("Unsupported frame length %f", WebRtcVad_ValidRateAndFrameLength,
 * src/common_audio/vad/webrtc_vad.c:92-115).  NULL on refusal (ssw_last_error). */
ssw_vad_t *ssw_vad_create(int32_t mode, int32_t sample_rate, double frame_length);
void ssw_vad_free(ssw_vad_t *v);
int32_t ssw_vad_frame_size(const ssw_vad_t *v);    /* vad_frame_size, samples; -1 on NULL */
double ssw_vad_frame_length(const ssw_vad_t *v);   /* vad_frame_length: frame_size / sample_rate */
int32_t ssw_vad_sample_rate(const ssw_vad_t *v);   /* vad_sample_rate: the caller's rate */
int32_t ssw_vad_closest_rate(const ssw_vad_t *v);  /* the rate the detector works at */
/* whole frames in n_samples samples: n_samples / frame_size; -1 on error */
int64_t ssw_vad_frame_count(const ssw_vad_t *v, int64_t n_samples);

/* What VadInstT (src/common_audio/vad/vad_core.h:25-51) carries from frame to frame, mode
 * thresholds apart (they belong to the ssw_vad_t).  Plain data: copy it, keep it, hand it back. */
typedef struct ssw_vad_state_s {
    int32_t downsampling_filter_states[4]; /* WebRtcVad_Downsampling: [0..1] 16 -> 8, [2..3] 32 -> 16 */
    int32_t s_48_24[8], s_24_24[16], s_24_16[8], s_16_8[8]; /* WebRtcSpl_State48khzTo8khz */
    int32_t frame_counter;
    int16_t noise_means[12], speech_means[12], noise_stds[12], speech_stds[12];
    int16_t over_hang, num_of_speech;
    int16_t index_vector[96], low_value_vector[96]; /* the minimum tracker's ages and values */
    int16_t mean_value[6];                          /* its smoothed medians */
    int16_t upper_state[5], lower_state[5], hp_filter_state[4];
    int16_t initialised; /* 42 (kInitCheck) once set up; anything else: the batch call starts afresh */
    int16_t reserved;
} ssw_vad_state_t;
/* the state after WebRtcVad_InitCore (src/common_audio/vad/vad_core.c:491-545) */
void ssw_vad_state_init(ssw_vad_state_t *s);

/* vad_classify (src/ps_vad.c:154-160) over every whole frame of every stream: d_pcm int16 in
 * HBM, stream u = samples samp_off[u] .. samp_off[u + 1] (host int64 [n_streams + 1]); frames
 * are ssw_vad_frame_size samples, the samples left after the last whole frame are not read.
 * d_is_speech int8 [total frames] in HBM holds vad_classify's return value per frame: 1 speech,
 * 0 not.  (GmmProbability's own value, 2 + over_hang during the hang-over, never leaves
 * WebRtcVad_Process: src/common_audio/vad/webrtc_vad.c:86-88 makes it 1.)  frame_off_out host
 * int32 [n_streams + 1].  state NULL: every stream starts afresh; else host [n_streams], read
 * where .initialised is 42 (else started afresh) and written with the state after the stream's
 * last frame, so a stream may arrive in pieces of whole frames.  Kept as the reference has it:
 * at 48 kHz WebRtcVad_CalcVad48khz (vad_core.c:607-630) resamples the frame's FIRST 10 ms once
 * per 10 ms of frame and never reads the rest; the model update's multiply wraps
 * (vad_core.c:117-120); a frame of digital silence takes LogOfEnergy's energy == 0 branch and
 * one whose total energy stays at or below kMinEnergy skips the Gaussians and the update.
 * Synchronous on `stream`; 0, or -1 (ssw_last_error). */
int ssw_vad_batch(ssw_vad_t *v, const int16_t *d_pcm, const int64_t *samp_off, int32_t n_streams,
                  int8_t *d_is_speech, int32_t *frame_off_out, ssw_vad_state_t *state,
                  void *stream);
/* How many of a workgroup's 64 lanes ssw_vad_batch gives streams: 8, 16, 32 or 64, or 0 (the
 * default) for the rule that spreads a batch over the device's compute units first -- 8 until
 * 8 per unit no longer covers the batch, then 16, 32, 64.  The results do not depend on it.
 * 0, or -1 on another value. */
int ssw_vad_set_streams_per_workgroup(ssw_vad_t *v, int32_t streams);
/* the same over host pointers with no device call, from the same arithmetic source */
int ssw_vad_batch_host(const ssw_vad_t *v, const int16_t *pcm, const int64_t *samp_off,
                       int32_t n_streams, int8_t *is_speech, int32_t *frame_off_out,
                       ssw_vad_state_t *state, int16_t *features);
/* parity view: the last ssw_vad_batch call's int16 [total frames][7] -- the six band
 * log-energies WebRtcVad_CalculateFeatures made and its total_energy -- copied to the host
 * buffer `out` of n_frames rows.  (ssw_vad_batch_host writes the same rows to `features` when
 * that is not NULL.)  0, or -1 when there was no call or n_frames is not its frame count. */
int ssw_vad_debug_features(ssw_vad_t *v, int16_t *out, int64_t n_frames);

/* one utterance the endpointer cut out of a stream */
typedef struct ssw_endpoint_seg_s {
    int64_t first_sample; /* in the stream: the first frame endpointer_process handed back */
    int64_t n_samples;    /* frames handed back x frame size + endpointer_end_stream's out_nsamp */
    double speech_start;  /* endpointer_speech_start, seconds */
    double speech_end;    /* endpointer_speech_end */
} ssw_endpoint_seg_t;
typedef struct ssw_endpoints_s ssw_endpoints_t;
/* Host only.  endpointer_init's window arithmetic (src/ps_endpointer.c:53-94; window 0 = 0.3,
 * ratio 0 = 0.9; "Ratio %.2f makes start-pointing stupid or impossible (%d frames of %d)" and
 * the end-pointing twin refuse) and endpointer_process over is_speech[0 .. n_frames) followed
 * by one endpointer_end_stream with tail_samples samples (0 .. frame_size), replayed without
 * the audio (:129-322).  Times are accumulated as there, by repeated addition of the frame
 * length.  The result holds one stream (index 0).  NULL on refusal (ssw_last_error). */
ssw_endpoints_t *ssw_endpoints_from_decisions(const ssw_vad_t *v, double window, double ratio,
                                              const int8_t *is_speech, int64_t n_frames,
                                              int64_t tail_samples);
/* ssw_vad_batch (every stream afresh), the decisions brought to the host, and the replay per
 * stream with the samples left after its last whole frame as the tail (zero of them included) */
ssw_endpoints_t *ssw_endpoint_batch(ssw_vad_t *v, double window, double ratio,
                                    const int16_t *d_pcm, const int64_t *samp_off,
                                    int32_t n_streams, void *stream);
int32_t ssw_endpoints_streams(const ssw_endpoints_t *e);
int32_t ssw_endpoints_count(const ssw_endpoints_t *e, int32_t stream); /* segments; -1 on error */
int ssw_endpoints_get(const ssw_endpoints_t *e, int32_t stream, int32_t k, ssw_endpoint_seg_t *out);
void ssw_endpoints_free(ssw_endpoints_t *e);

#ifdef __cplusplus
}
#endif
#endif /* SSW_AMD_H */
