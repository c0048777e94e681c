/* ssw_host_score.inc -- host: batched scoring entry points.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
static int
ensure_score_ws(ssw_model_s *m, int n_frames, int n_utts)
{
    if ((size_t)n_frames > m->ws_frames) {
        (void)hipFree(m->d_topn_cw);
        (void)hipFree(m->d_topn_sc);
        m->d_topn_cw = NULL;
        m->d_topn_sc = NULL;
        m->ws_frames = 0;
        if ((uint64_t)n_frames * (uint64_t)m->n_cbf > 0xffffffffull) {
            ssw_set_error("batch of %d frames is too large (frames x codebooks x streams must fit 32 bits)",
                          n_frames);
            return -1;
        }
        if (dev_alloc(&m->d_topn_cw, (size_t)n_frames * m->n_cbf) < 0
            || dev_alloc(&m->d_topn_sc, (size_t)n_frames * m->n_cbf) < 0)
            return -1;
        m->ws_frames = (size_t)n_frames;
    }
    if (m->d_nfixed == NULL) {
        if (dev_alloc(&m->d_nfixed, 4) < 0)
            return -1;
        HIP_OK(hipMemset(m->d_nfixed, 0, 4 * sizeof(unsigned long long)));
    }
    /* utterance offsets, start bits and skip bits share ONE buffer, laid out so that a call
     * uploads them with one copy: [offsets: ws_utts words][start bits: nw][skip bits: nw], nw =
     * the words THIS batch's bits take (meta_nw, kept with the cached offsets) */
    const size_t need_bits = 2 * (((size_t)n_frames + 31) / 32 + 2);
    if ((size_t)n_utts + 1 > m->ws_utts || need_bits > m->ws_bits) {
        (void)hipFree(m->d_utt_off);
        m->d_utt_off = NULL;
        m->d_utt_start = NULL;
        m->ws_utts = m->ws_bits = 0;
        if (m->utt_cache)
            m->utt_cache->clear(); /* everything has to be uploaded again */
        const size_t wu = std::max((size_t)n_utts + 1, m->ws_utts_hint), wb = std::max(need_bits, m->ws_bits_hint);
        uint32_t *meta = NULL;
        if (dev_alloc(&meta, wu + wb) < 0)
            return -1;
        m->d_utt_off = reinterpret_cast<int *>(meta);
        m->d_utt_start = meta + wu;
        m->ws_utts = m->ws_utts_hint = wu;
        m->ws_bits = m->ws_bits_hint = wb;
    }
    return 0;
}

static int
check_scorer_shape(const ssw_model_s *m, int scorer)
{
    const ssw_host_model_t *h = m->h;
    if (m->device == SSW_DEVICE_NONE) {
        ssw_set_error("model was loaded with device = SSW_DEVICE_NONE (tables only): no GPU, "
                      "no scoring -- there is no CPU fallback");
        return -1;
    }
    if (h->continuous)
        return cont_check_shape(m, scorer);
    if (scorer == SSW_SCORER_S2_SEMI || h->sc_rec != NULL)
        return semi_check_shape(m, scorer);
    if (scorer == SSW_SCORER_PTM && h->ptm_mixw == NULL) {
        ssw_set_error("model has no PTM mixture weights (sendump / mixw)");
        return -1;
    }
    if (scorer == SSW_SCORER_MS && h->ms_pdf == NULL) {
        ssw_set_error("the ms scorer needs a mixture_weights file (src/ms_mgau.c:208-212)");
        return -1;
    }
    if (scorer == SSW_SCORER_MS && (h->logadd8_size != 256 || h->cfg.aw == 0)) {
        ssw_set_error("ms scorer: unsupported log base (add table of %d entries) or aw = 0",
                      h->logadd8_size);
        return -1;
    }
    if (scorer != SSW_SCORER_PTM && scorer != SSW_SCORER_MS) {
        ssw_set_error("unknown scorer %d", scorer);
        return -1;
    }
    if (h->n_density != 128 || h->cfg.topn != 4 || h->n_cb > 255) {
        ssw_set_error("PTM kernels are built for 128 densities, top-4, <= 255 codebooks "
                      "(model: %d densities, topn %d, %d codebooks)",
                      h->n_density, h->cfg.topn, h->n_cb);
        return -1;
    }
    for (int f = 0; f < h->n_feat; ++f)
        if (h->veclen[f] != 13) {
            ssw_set_error("PTM kernels are built for 13-dimensional streams");
            return -1;
        }
    return 0;
}

static void
fill_chain_params(const ssw_model_s *m, ChainParams &P, const float *d_feats)
{
    const ssw_host_model_t *h = m->h;
    memset(&P, 0, sizeof(P));
    P.rec = m->d_rec;
    P.feats = d_feats;
    P.utt_off = m->d_utt_off;
    P.topn_cw = m->d_topn_cw;
    P.topn_sc = m->d_topn_sc;
    P.n_cbf = m->n_cbf;
    P.n_feat = h->n_feat;
    P.featdim = h->veclen_total;
    P.ds = h->cfg.ds < 1 ? 1 : h->cfg.ds;
    for (int f = 0; f < h->n_feat; ++f)
        P.featoff[f] = h->featoff[f];
}

/* the packed persistent kernel serves the ms scorer too (its marked-frame fallback covers what
 * 16 bits cannot hold); ms_senone_kernel keeps aw != 1, the un-normalised mode of the one-frame
 * active-set call, small batches and SSW_MS_SENONE=old (tests, A/B) */
static bool
ms_takes_packed_kernel(const ssw_model_s *m, int n_frames)
{
    const ssw_host_model_t *h = m->h;
    int tab_max = 0;
    for (int i = 0; i < 256; ++i)
        tab_max = h->logadd8[i] > tab_max ? h->logadd8[i] : tab_max;
    return h->cfg.aw == 1 && !m->ms_raw && n_frames >= 4 * 512 && h->n_cb <= 64
        && 255 + 640 + 6 * tab_max < SSW_LOGADD_MIRROR && !m->kn.ms_senone_old;
}

/* cp != NULL: compact rows (ssw_host_compact.inc) -- d_out is then the compact buffer and
 * frame_base the batch frame number of this launch's first frame; only for launches that take
 * the persistent kernel (the caller checks senone_compact_ok) */
static int
launch_senone(ssw_model_s *m, int scorer, int n_frames, const uint32_t *cw, const int4 *sc,
              int16_t *d_out, bool move_stats, hipStream_t st, bool share_device = false,
              const ssw_compact_plan_s *cp = NULL, int frame_base = 0)
{
    const ssw_host_model_t *h = m->h;
    SenoneParams S;
    memset(&S, 0, sizeof(S));
    S.topn_cw = cw;
    S.topn_sc = sc;
    S.mixw = scorer == SSW_SCORER_MS ? m->d_ms_pdf : m->d_mixw;
    S.aw = h->cfg.aw;
    S.zero = h->zero8;
    S.raw = m->ms_raw;
    S.quad_cb = m->d_quad_cb;
    S.quad_info = m->d_quad_info;
    S.slot_sen = m->d_slot_sen;
    S.logadd8 = m->d_logadd8;
    S.logadd_mirror = m->d_logadd_mirror + (scorer == SSW_SCORER_MS ? SSW_LOGADD_MIRROR : 0);
    S.nfixed = move_stats ? m->d_nfixed : NULL;
    S.nfixed_acc = m->stats_accumulate;
    S.out = d_out;
    if (cp != NULL) {
        S.utt_of_frame = cp->d_utt_of_frame;
        S.cutt_off = cp->d_frame_off;
        S.cstride = cp->d_cstride;
        S.crow_off = cp->d_crow_off;
        S.cpos = cp->d_cpos;
        S.frame_base = frame_base;
    }
    S.n_frames = n_frames;
    S.n_cb = h->n_cb;
    S.n_feat = h->n_feat;
    S.n_density = h->n_density;
    S.n_sen = h->n_sen;
    S.slot_stride = m->slot_stride;
    S.n_quads = m->n_quads;
    S.tab_max = 0;
    for (int i = 0; i < 256; ++i)
        S.tab_max = h->logadd8[i] > S.tab_max ? h->logadd8[i] : S.tab_max;
    /* the PTM kernel indexes a 512-entry table with |x - y|, x >= -3 tab_max, y <= 255 + 96 */
    if (scorer != SSW_SCORER_MS && 255 + SSW_MAX_NEG_ASCR + 3 * S.tab_max >= SSW_LOGADD_LDS) {
        ssw_set_error("unsupported log-add table (largest entry %d)", S.tab_max);
        return -1;
    }
    /* Shape of the PTM workgroups (measured on MI355X, en-us, 4096 frames, round 2 kernel):
     * frames per workgroup x quads per thread = 4 x 2 (704 threads, 2 groups per CU) 41.4 us,
     * 2 x 3 (448 threads, 4 groups per CU, 28 waves) 39.5 us, 2 x 4 44.2, 1 x 3 42.0, 1 x 4 45.6:
     * two frames share a prologue, and seven-wave groups fill the CU's 32 wave slots where
     * eleven-wave ones leave ten empty.  Small batches: one frame per group, as many threads as
     * there are quads.  SSW_SEN_FPB / SSW_SEN_R override (tuning). */
    const bool ptm = scorer != SSW_SCORER_MS;
    const Knobs &kn = m->kn;
    int fpb = n_frames >= 4 * 512 ? 2 : 1;
    if (kn.sen_fpb != 0 && n_frames >= 4 * 512)
        fpb = kn.sen_fpb;
    size_t lds = 0; /* set once fpb is final */
    int R = (m->n_quads + SEN_MAX_THREADS - 1) / SEN_MAX_THREADS;
    const bool ms_packed = !ptm && ms_takes_packed_kernel(m, n_frames);
    if (cp != NULL && !ptm && !ms_packed) {
        ssw_set_error("internal error: compact rows asked of the un-packed ms senone kernel");
        return -1;
    }
    if ((ptm || ms_packed) && fpb == 2 && R < 4) { /* about seven waves per group */
        const int r7 = (m->n_quads + 447) / 448;
        R = r7 > R ? (r7 > 4 ? 4 : r7) : R;
    }
    if (kn.sen_r != 0)
        R = kn.sen_r;
    int threads = ((m->n_quads + R - 1) / R + 63) & ~63;
    if (threads < 256)
        threads = 256; /* the prologue copies the 256-entry table with the first 256 threads */
    if (threads > SEN_MAX_THREADS || (scorer == SSW_SCORER_MS && threads < m->n_cbf)) {
        ssw_set_error("unsupported senone/codebook shape (%d quads, %d codebook x stream)",
                      m->n_quads, m->n_cbf);
        return -1;
    }
    if (scorer == SSW_SCORER_MS && !ms_packed) {
        lds = 256 + 20 * (size_t)m->n_cbf + 16 * sizeof(int);
#define SSW_MS_LAUNCH(RR)                                                                    \
    if (h->n_feat == 3 && !kn.sen_generic)                                                   \
        hipLaunchKernelGGL((ms_senone_kernel<RR, 3>), dim3(n_frames), dim3(threads), lds, st, S); \
    else                                                                                     \
        hipLaunchKernelGGL((ms_senone_kernel<RR, 0>), dim3(n_frames), dim3(threads), lds, st, S)
        switch (R) {
        case 1: SSW_MS_LAUNCH(1); break;
        case 2: SSW_MS_LAUNCH(2); break;
        case 3: SSW_MS_LAUNCH(3); break;
        case 4: SSW_MS_LAUNCH(4); break;
        default:
            ssw_set_error("too many senones (%d quads)", m->n_quads);
            return -1;
        }
#undef SSW_MS_LAUNCH
        HIP_OK(hipGetLastError());
        return 0;
    }
    /* one item of the top-N block per thread (the persistent kernel keeps it in registers) */
    if (threads < fpb * m->n_cbf)
        fpb = 1;
    if (threads < m->n_cbf) {
        ssw_set_error("unsupported senone/codebook shape (%d quads, %d codebook x stream)",
                      m->n_quads, m->n_cbf);
        return -1;
    }
    /* LDS: mirrored table | norm[3][fpb][8] | red[16] | item[2][n_cbf][fpb] of 32 bytes */
    lds = (ms_packed ? 2 * SSW_LOGADD_MIRROR : SSW_LOGADD_MIRROR)
        + 3 * 4 * (size_t)(ms_packed ? ((h->n_cb + 7) & ~7) : SSW_MAX_FEAT) * fpb + 16 * sizeof(int)
        + 2 * 32 * (size_t)m->n_cbf * fpb
        + 20 * (size_t)((fpb * m->n_cbf + 63) & ~63) /* DMA staging: scores + codewords */
        + 8 * (size_t)R * threads + 16;             /* senone ids of every quad */
    /* persistent groups: as many as the chip holds at once (32 wave slots per CU), each taking
     * the units (fpb frames) g, g + grid, ...; SSW_SEN_GROUPS overrides (tuning: 0 = one group
     * per unit, the round-2 form) */
    const int n_units = (n_frames + fpb - 1) / fpb;
    int per_cu = 32 / (threads / 64);
    per_cu = per_cu < 1 ? 1 : per_cu;
    int groups = m->n_cu * per_cu;
    /* SSW_SCORE_SHARE_DEVICE: no group stays for more than 8 units, so that a kernel of another
     * stream (the alignment of the previous chunk, jobs.py) gets wave slots every ~100 us
     * instead of waiting for a whole 256,000-frame launch to drain (config 5 on one GPU: 56-59
     * -> 53-57 ms; alone, the shorter stay costs 3 % at 65,536 frames) */
    if (share_device && groups < (n_units + 7) / 8)
        groups = (n_units + 7) / 8;
    if (kn.sen_groups >= 0)
        groups = kn.sen_groups > 0 ? kn.sen_groups : n_units;
    const dim3 grid(groups < n_units ? groups : n_units);
    /* (the instances with the stream count as a run-time value serve models that do not have 3
     * streams; SSW_SEN_GENERIC=1 runs them on the others as well, for the tests) */
    const bool nf3 = h->n_feat == 3 && !kn.sen_generic;
    if (fpb != 1 && fpb != 2) {
        ssw_set_error("senone kernel: %d frames per group (1 or 2)", fpb);
        return -1;
    }
#define SSW_SEN_LAUNCH_C(RR, FP, NFV, MSV, CV)                                               \
    hipLaunchKernelGGL((ptm_senone_kernel<4, RR, FP, NFV, MSV, CV>), grid, dim3(threads), lds, st, S)
#define SSW_SEN_LAUNCH_NF(RR, FP, MSV, CV)                                                   \
    if (nf3)                                                                                 \
        SSW_SEN_LAUNCH_C(RR, FP, 3, MSV, CV);                                                \
    else                                                                                     \
        SSW_SEN_LAUNCH_C(RR, FP, 0, MSV, CV)
#define SSW_SEN_LAUNCH_FP(RR, MSV, CV)                                                       \
    if (fpb == 2) {                                                                          \
        SSW_SEN_LAUNCH_NF(RR, 2, MSV, CV);                                                   \
    } else {                                                                                 \
        SSW_SEN_LAUNCH_NF(RR, 1, MSV, CV);                                                   \
    }
#define SSW_SEN_LAUNCH(RR)                                                                   \
    if (ms_packed && cp != NULL) {                                                           \
        SSW_SEN_LAUNCH_FP(RR, true, true);                                                   \
    } else if (ms_packed) {                                                                  \
        SSW_SEN_LAUNCH_FP(RR, true, false);                                                  \
    } else if (cp != NULL) {                                                                 \
        SSW_SEN_LAUNCH_FP(RR, false, true);                                                  \
    } else {                                                                                 \
        SSW_SEN_LAUNCH_FP(RR, false, false);                                                 \
    }
    switch (R) {
    case 1: SSW_SEN_LAUNCH(1); break;
    case 2: SSW_SEN_LAUNCH(2); break;
    case 3: SSW_SEN_LAUNCH(3); break;
    case 4: SSW_SEN_LAUNCH(4); break;
    default:
        ssw_set_error("too many senones (%d quads)", m->n_quads);
        return -1;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

/* per-frame active sets of a compallsen = no batch (device pointers; ssw_host_active.inc) */
struct ActiveSets {
    const int32_t *seg_of_frame;
    const unsigned long long *seg_cbmask;
    SenoneActive2Params *a2; /* filled by the caller but for the top-N block and the model's tables */
    /* or (a2 == NULL): a listed set per frame as a bitmap, ssw_k7_fpactive.inc -- listed, cbmask,
     * out, full, cap are the caller's, the rest is filled here */
    const SenoneListedParams *ls;
};

/* batches from this many frames take the matrix-core scan.  Rounds 2-3: 2,049, where the bf16
 * form caught up with the vector-unit scan; the binary16 form of round 4 is ahead at every
 * size measured -- 256 frames: 15.7 against 27.6 us, 1,024: 17.9 against 30.4, 2,048: 23.2
 * against 44.4 (DESIGN.md section 5) -- so every batch takes it; SSW_SCAN=fma or a larger
 * SSW_MFMA_MIN_FRAMES keep the vector-unit scan (tests, A/B) */
#define SSW_MFMA_MIN_FRAMES_DEFAULT 1
static int
score_batch_impl(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                 const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream,
                 uint32_t flags, const uint32_t *carry_in, uint32_t *carry_out,
                 const ActiveSets *act = NULL, const uint32_t *d_carry_rows = NULL,
                 const ssw_compact_plan_s *cp = NULL, int frame_base = 0);

extern "C" int
ssw_score_batch(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream)
{
    return score_batch_impl(m, scorer, d_feats, n_frames, utt_off, n_utts, d_out, stream, 0u, NULL,
                            NULL);
}

extern "C" int
ssw_score_batch_ex(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                   const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream,
                   uint32_t flags, const uint32_t *carry_in, uint32_t *carry_out)
{
    return score_batch_impl(m, scorer, d_feats, n_frames, utt_off, n_utts, d_out, stream, flags,
                            carry_in, carry_out);
}

/* what every scoring call ends in: the counters, and carry_out read back */
static int
score_batch_finish(ssw_model_t *m, bool ms, int32_t n_frames, const int32_t *utt_off, int32_t n_utts,
                   hipStream_t st, uint32_t flags, const uint32_t *carry_in, uint32_t *carry_out)
{
    const bool chain = (flags & SSW_SCORE_CARRY_UTTS) != 0 && !ms;
    const int64_t pairs = (int64_t)n_frames * m->n_cbf;
    m->last_n_frames = n_frames;
    m->stats[1] = pairs;
    if (carry_out != NULL) {
        /* what the next call starts from.  Default: the last frame's final order (the next call
         * continues the same utterance).  SSW_SCORE_CARRY_OUT_REWIND: history slot 1 of the
         * reference's ring, which is what frame 0 of the NEXT utterance -- or of the second pass
         * after acmod_rewind -- copies (src/ptm_mgau.c:425-437): the final order of the last
         * odd-numbered frame of the last utterance that has two frames (in a chain; of the last
         * utterance otherwise), else what that utterance itself started from */
        long long row = (long long)n_frames - 1;
        bool from_start = false; /* no frame wrote the slot: carry_in / the reset order */
        if (flags & SSW_SCORE_CARRY_OUT_REWIND) {
            row = -1;
            for (int u = n_utts - 1; u >= 0 && row < 0; --u) {
                const int T = utt_off[u + 1] - utt_off[u];
                if (T >= 2)
                    row = (long long)utt_off[u] + (T / 2) * 2 - 1;
                else if (!chain) { /* utterances are independent: only the last one counts */
                    from_start = true;
                    for (int i = 0; i < m->n_cbf; ++i)
                        carry_out[i] = (u == 0 && carry_in != NULL) ? carry_in[i] : 0x03020100u;
                    break;
                }
            }
            if (row < 0 && !from_start) {
                from_start = true;
                for (int i = 0; i < m->n_cbf; ++i)
                    carry_out[i] = carry_in != NULL ? carry_in[i] : 0x03020100u;
            }
        }
        if (ms)
            for (int i = 0; i < m->n_cbf; ++i)
                carry_out[i] = 0x03020100u; /* the ms scorer keeps no history */
        else if (!from_start) {
            HIP_OK(hipMemcpyAsync(carry_out, m->d_topn_cw + (size_t)row * m->n_cbf,
                                  sizeof(uint32_t) * (size_t)m->n_cbf, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
        }
    }
    return 0;
}

static int
score_batch_impl(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                 const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream,
                 uint32_t flags, const uint32_t *carry_in, uint32_t *carry_out,
                 const ActiveSets *act, const uint32_t *d_carry_rows, const ssw_compact_plan_s *cp,
                 int frame_base)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    refresh_knobs(m); /* tests: knobs flipped between calls on one model */
    const Knobs &kn = m->kn;
    hipStream_t st = (hipStream_t)stream;
    if (carry_out != NULL && (n_frames == 0 || n_utts == 0)) { /* nothing scored: state unchanged */
        for (int i = 0; i < m->n_cbf; ++i)
            carry_out[i] = carry_in ? carry_in[i] : 0x03020100u;
    }
    if (n_frames == 0 || n_utts == 0)
        return 0;
    if (n_frames < 0 || n_utts < 0 || utt_off == NULL || utt_off[0] != 0
        || utt_off[n_utts] != n_frames) {
        ssw_set_error("bad utterance offsets");
        return -1;
    }
    for (int u = 0; u < n_utts; ++u)
        if (utt_off[u + 1] < utt_off[u]) {
            ssw_set_error("utterance offsets must be non-decreasing");
            return -1;
        }
    if (check_scorer_shape(m, scorer) < 0)
        return -1;
    const bool ms = scorer == SSW_SCORER_MS;
    if (act != NULL && (m->h->cfg.ds != 1 || m->force_exact)) { /* (before anything is launched) */
        ssw_set_error("active-set batches: ds = 1 only");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    if (m->h->continuous) {
        /* no history, no utterance boundaries, none of the PTM scan's workspaces: its own two
         * kernels (ssw_host_cont.inc); flags, carry_in and ds are ignored as for ms */
        if (act != NULL || cp != NULL) {
            ssw_set_error("internal error: active sets or compact rows with a continuous model");
            return -1;
        }
        if (m->timing) {
            HIP_OK(hipEventRecord(m->ev[0], st));
            m->timing_semi = 0;
        }
        if (cont_launch(m, d_feats, n_frames, d_out, st) < 0)
            return -1;
        m->stats[0] = 0;
        m->stats_pending = 0;
        m->last_n_frames = 0; /* (no top-N block: ssw_score_batch_topn has nothing to show) */
        m->stats[1] = (int64_t)n_frames * m->n_cbf;
        for (int i = 0; carry_out != NULL && i < m->n_cbf; ++i)
            carry_out[i] = 0x03020100u; /* the ms scorer keeps no history */
        return 0;
    }
    /* history carried from utterance to utterance (the reference never resets it after
     * start-up, src/acmod.c:367): the batch is one chain, only its first frame is a start.  The
     * chain follows the reference's two-slot ring (src/ptm_mgau.c:425-437): frame numbers restart
     * with every utterance and its frame 0 copies slot 1, so the last frame of an utterance of odd
     * length is off the chain (`skip` bits below; a one-frame utterance entirely) */
    const bool chain = (flags & SSW_SCORE_CARRY_UTTS) != 0 && !ms;
    if (ensure_score_ws(m, n_frames, n_utts) < 0)
        return -1;
    /* a caller that moves from one stream to another: the uploads below are only ordered behind
     * the launches of THIS stream */
    if (m->have_last_score_stream && m->last_score_stream != st)
        HIP_OK(hipDeviceSynchronize()); /* (not the old stream itself: it may be gone) */
    m->last_score_stream = st;
    m->have_last_score_stream = 1;
    const bool want_carry = carry_in != NULL && !ms;
    if (want_carry) {
        for (int i = 0; i < m->n_cbf; ++i)
            for (int k = 0; k < 4; ++k)
                if (((carry_in[i] >> (8 * k)) & 0xffu) >= (uint32_t)m->h->n_density) {
                    ssw_set_error("carry_in[%d] names codeword %u of %d", i,
                                  (carry_in[i] >> (8 * k)) & 0xffu, m->h->n_density);
                    return -1;
                }
        if (devbuf_reserve(m->carry0, sizeof(uint32_t) * (size_t)m->n_cbf * (size_t)n_utts,
                           "ssw_score_batch_ex") < 0)
            return -1;
    }
    /* the offsets rarely change between calls of one job: upload only when they do
     * (cache key: the chain flag, then the offsets) */
    if (m->utt_cache == NULL)
        m->utt_cache = new std::vector<int32_t>();
    const bool new_offsets = m->utt_cache->size() != (size_t)n_utts + 2
        || (*m->utt_cache)[0] != (chain ? 1 : 0)
        || memcmp(m->utt_cache->data() + 1, utt_off, sizeof(int32_t) * ((size_t)n_utts + 1)) != 0;
    if (want_carry || new_offsets) {
        /* one pinned slot for everything this call uploads: [carry rows][offsets][starts][skip] */
        const size_t ncar = want_carry ? (size_t)m->n_cbf * (size_t)n_utts : 0;
        const size_t nw = ((size_t)n_frames + 31) / 32 + 1;
        const size_t b_car = sizeof(uint32_t) * ncar;
        const size_t b_off = new_offsets ? sizeof(int32_t) * ((size_t)n_utts + 1) : 0;
        const size_t b_bits = new_offsets ? sizeof(uint32_t) * nw : 0;
        int slot = 0;
        unsigned char *hs = stage_acquire(m, b_car + sizeof(uint32_t) * m->ws_utts + 2 * b_bits + 64, &slot);
        if (hs == NULL)
            return -1;
        if (want_carry) {
            /* [n_utts][n_cbf]: the first utterance starts from carry_in, the others from the
             * reset history (the chain kernel reads a row per utterance, the scans only row 0) */
            uint32_t *car = reinterpret_cast<uint32_t *>(hs);
            for (size_t i = 0; i < ncar; ++i)
                car[i] = 0x03020100u;
            memcpy(car, carry_in, sizeof(uint32_t) * (size_t)m->n_cbf);
            HIP_OK(hipMemcpyAsync(m->carry0.as<uint32_t>(), car, b_car, hipMemcpyHostToDevice, st));
        }
        if (new_offsets) {
            m->utt_cache->assign(1, chain ? 1 : 0);
            m->utt_cache->insert(m->utt_cache->end(), utt_off, utt_off + n_utts + 1);
            /* staged as it lies on the device: offsets (ws_utts words), start bits, skip bits */
            int32_t *hoff = reinterpret_cast<int32_t *>(hs + b_car);
            uint32_t *starts = reinterpret_cast<uint32_t *>(hoff + m->ws_utts);
            uint32_t *skip = starts + nw;
            memcpy(hoff, utt_off, b_off);
            memset(starts, 0, 2 * b_bits);
            if (chain)
                starts[0] = 1u;
            for (int u = 0; u < n_utts; ++u) {
                if (!chain && utt_off[u] < n_frames)
                    starts[(size_t)utt_off[u] >> 5] |= 1u << (utt_off[u] & 31);
                if (chain && ((utt_off[u + 1] - utt_off[u]) & 1)) {
                    const int t = utt_off[u + 1] - 1;
                    skip[(size_t)t >> 5] |= 1u << (t & 31);
                }
            }
            m->meta_nw = nw;
            HIP_OK(hipMemcpyAsync(m->d_utt_off, hoff, sizeof(uint32_t) * (m->ws_utts + 2 * nw),
                                  hipMemcpyHostToDevice, st));
        }
        if (stage_release(m, slot, st) < 0)
            return -1;
    }
    const ssw_host_model_t *h = m->h;
    ChainParams P;
    fill_chain_params(m, P, d_feats);
    P.n_utts = n_utts;
    P.n_frames = n_frames;
    P.chain_utts = chain ? 1 : 0;
    /* a call that continues an utterance (a piece of ssw_score_batch_host's cut): the in-utterance
     * number of its frame 0, which decides the frames a ds > 1 model re-scans on */
    P.frame_base = frame_base;
    P.carry_pk = (carry_in != NULL && !ms) ? m->carry0.as<uint32_t>() : NULL;
    if (d_carry_rows != NULL && !ms) /* a row per utterance, already on the device */
        P.carry_pk = d_carry_rows;
    const int64_t pairs = (int64_t)n_frames * m->n_cbf;
    bool pieced = false;
    /* compallsen = no: the senone kernel of frames [lo, hi) (ssw_host_active.inc filled the
     * segment tables; four frames per workgroup, a wave each) */
    auto launch_active = [&](int lo, int hi) -> hipError_t {
        if (act->a2 == NULL) {
            SenoneListedParams L = *act->ls;
            L.topn_cw = m->d_topn_cw + (size_t)lo * m->n_cbf;
            L.topn_sc = m->d_topn_sc + (size_t)lo * m->n_cbf;
            L.mixw = ms ? m->d_ms_pdf : m->d_mixw;
            L.logadd8 = m->d_logadd8;
            L.sen2cb = m->d_sen2cb;
            L.sen_slot = m->d_sen_slot;
            L.n_frames = hi - lo;
            L.frame_base = lo;
            L.n_cb = h->n_cb;
            L.n_feat = h->n_feat;
            L.n_density = h->n_density;
            L.n_sen = h->n_sen;
            L.slot_stride = m->slot_stride;
            L.nw32 = (h->n_sen + 31) / 32;
            L.zero = h->zero8;
            L.aw = h->cfg.aw;
            if (L.cap <= 0 || L.cap > h->n_sen)
                L.cap = h->n_sen; /* (the caller's bound on a frame's listed entries) */
            const size_t per_wave = ((ms ? 0 : 8 * (size_t)m->n_cbf) + 4 * (size_t)((L.cap + 1) & ~1)
                                     + 16 + 15) & ~(size_t)15;
            const size_t lds = 4 * per_wave;
            const dim3 grid((unsigned)((hi - lo + 3) / 4));
            if (lds > 48 * 1024) {
                const hipError_t ea = hipFuncSetAttribute(
                    ms ? (const void *)senone_listed_kernel<true> : (const void *)senone_listed_kernel<false>,
                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (ea != hipSuccess)
                    return ea;
            }
            if (ms)
                hipLaunchKernelGGL(senone_listed_kernel<true>, grid, dim3(256), lds, st, L);
            else
                hipLaunchKernelGGL(senone_listed_kernel<false>, grid, dim3(256), lds, st, L);
            return hipGetLastError();
        }
        SenoneActive2Params A = *act->a2;
        A.zero = h->zero8;
        A.aw = h->cfg.aw;
        A.topn_cw = m->d_topn_cw + (size_t)lo * m->n_cbf;
        A.topn_sc = m->d_topn_sc + (size_t)lo * m->n_cbf;
        A.mixw = ms ? m->d_ms_pdf : m->d_mixw;
        A.logadd8 = m->d_logadd8;
        A.n_frames = hi - lo;
        A.frame_base = lo;
        A.n_cb = h->n_cb;
        A.n_feat = h->n_feat;
        A.n_density = h->n_density;
        A.n_sen = h->n_sen;
        A.slot_stride = m->slot_stride;
        const size_t per_wave = (ms ? 0 : 8 * (size_t)m->n_cbf) + 2 * (size_t)((A.cap + 1) & ~1)
            + (A.out_full != NULL ? 2 * (size_t)((h->n_sen + 1) & ~1) : 0);
        const size_t lds = 4 * ((per_wave + 15) & ~(size_t)15);
        const dim3 grid((unsigned)((hi - lo + 3) / 4));
        if (ms)
            hipLaunchKernelGGL(senone_active2_kernel<true>, grid, dim3(256), lds, st, A);
        else
            hipLaunchKernelGGL(senone_active2_kernel<false>, grid, dim3(256), lds, st, A);
        return hipGetLastError();
    };
    if (m->timing) {
        HIP_OK(hipEventRecord(m->ev[0], st));
        m->timing_semi = scorer == SSW_SCORER_S2_SEMI;
    }
    if (scorer == SSW_SCORER_S2_SEMI) {
        /* the same batch, history and carry semantics; its own three kernels (ssw_host_semi.inc) */
        if (act != NULL || cp != NULL) {
            ssw_set_error("internal error: active sets or compact rows with the s2_semi scorer");
            return -1;
        }
        if (semi_launch(m, P, d_out, st) < 0)
            return -1;
        m->stats[0] = 0;
        m->stats_pending = 0;
        return score_batch_finish(m, false, n_frames, utt_off, n_utts, st, flags, carry_in, carry_out);
    }
    if (!ms && (h->cfg.ds != 1 || m->force_exact)) {
        /* frame down-sampling makes every frame depend on its predecessor: exact chains */
        int n_chain = (chain ? 1 : n_utts) * m->n_cbf;
        hipLaunchKernelGGL((ptm_topn_chain_kernel<13, 2, 4>), dim3((n_chain + 3) / 4),
                           dim3(256), 0, st, P);
        HIP_OK(hipGetLastError());
        m->stats[0] = pairs;
        m->stats_pending = 0;
    } else {
        FramesParams F;
        memset(&F, 0, sizeof(F));
        F.topn_cw = m->d_topn_cw;
        F.topn_sc = m->d_topn_sc;
        F.utt_start = m->d_utt_start;
        F.carry0 = (carry_in != NULL && !ms) ? m->carry0.as<uint32_t>() : NULL;
        F.carry_rows = ms ? NULL : d_carry_rows;
        F.utt_off = m->d_utt_off;
        F.n_utts = n_utts;
        F.chain_skip = chain ? m->d_utt_start + m->meta_nw : NULL;
        F.seg_of_frame = act ? act->seg_of_frame : NULL;
        F.seg_cbmask = act ? act->seg_cbmask : NULL;
        F.n_fixed = m->d_nfixed;
        F.n_frames = n_frames;
        F.n_cbf = m->n_cbf;
        F.n_feat = h->n_feat;
        F.featdim = h->veclen_total;
        for (int f = 0; f < h->n_feat; ++f)
            F.featoff[f] = h->featoff[f];
        /* large batches of either scorer: the scan's multiply-adds go to the matrix cores (one
         * wave = 64 frames of one codebook x stream; SSW_SCAN=fma keeps the vector-unit scan) */
        /* (SSW_MFMA_MIN_FRAMES: tuning -- the smallest batch that takes the matrix-core scan;
         * d_wfrag is NULL on a device that failed the load-time self-test, ssw_host_model.inc) */
        const bool mfma = m->d_wfrag != NULL && h->n_feat * 13 == h->veclen_total
            && n_frames >= kn.mfma_min_frames && !kn.scan_fma;
        /* Large batches go through the two kernels in PIECES of ~16 K frames (round 3): measured
         * per frame, scan + senone cost 19.7 ns at 4,096 frames per launch (ramp and tail), 16.3
         * at 16,384, 17.3 at 65,536 and 18.3 at 262,144 -- a piece's top-N block (41 MB) is read
         * back by its senone launch while the memory-side cache still holds it, a whole batch's
         * (660 MB at 262,144 frames) is not.  The scan of a piece takes absolute frame numbers
         * (its exact pass may walk back into the piece before); the senone kernel has no
         * dependency between frames and gets offset pointers.  SSW_SCORE_PIECE = frames per
         * piece (a multiple of 256; 0 = never cut). */
        const int piece = kn.score_piece;
        const bool pieces = mfma && piece > 0 && n_frames >= 2 * piece;
        auto launch_scan = [&](int lo, int hi) {
            /* 64-frame steps per wave: one, or -- from 8,192 frames per launch -- two (half the
             * workgroups and half the LDS fills: +1.2 % at 8,192 frames, +1.3 % at 16,384, +1-2 %
             * at 65,536).  At 4,096 frames (1,008 workgroups for the chip's 1,280 slots) two steps
             * gave +2 % on one of the pool's slower boxes and -0.5 % on the faster ones; below
             * that one step is the faster form (39 against 43 us per call at 2,048 frames).
             * SSW_MFMA_STEPS = "1" / "2" overrides (PTM instance only) */
            const int nstep = ms ? 1
                : kn.mfma_steps != 0 ? kn.mfma_steps
                                     : (hi - lo >= 8192 ? 2 : 1);
            F.frame_lo = lo;
            F.n_frames = hi;
            F.tile_groups = (hi - lo + 256 * nstep - 1) / (256 * nstep);
            /* eight contiguous chunks of (codebook x stream, tile group) pairs, one per XCD,
             * equal in COST: ~1,400 vector instructions per wave and 64-frame step plus ~45 per
             * density its codebook leaves to the exact form (SSW_MFMA_BALANCE=0: equal counts).
             * The cut depends on the number of tile groups only: computed once per shape
             * (round 5: it used to be recomputed on every launch) */
            int max_len = 0;
            {
                const int key = F.tile_groups * 2 + (kn.mfma_balance ? 1 : 0);
                if (m->xcd_cuts == NULL)
                    m->xcd_cuts = new std::map<int, std::array<int, 10>>();
                auto it = m->xcd_cuts->find(key);
                if (it == m->xcd_cuts->end()) {
                    const bool by_cost = kn.mfma_balance;
                    const int n_pairs = m->n_cbf * F.tile_groups;
                    std::array<int, 10> cut;
                    double total = 0.0;
                    for (int c = 0; c < m->n_cbf; ++c)
                        total += (1400.0 + (by_cost ? 45.0 * h->exlistm[(size_t)c * SSW_EXLIST_STRIDE] : 0.0))
                            * F.tile_groups;
                    double acc = 0.0;
                    int x = 1;
                    cut[0] = 0;
                    for (int c = 0; c < m->n_cbf; ++c) {
                        const double w = 1400.0
                            + (by_cost ? 45.0 * h->exlistm[(size_t)c * SSW_EXLIST_STRIDE] : 0.0);
                        for (int g = 0; g < F.tile_groups; ++g) {
                            /* the pair goes to the chunk its middle falls into */
                            while (x < 8 && acc + 0.5 * w >= total * x / 8.0)
                                cut[x++] = c * F.tile_groups + g;
                            acc += w;
                        }
                    }
                    while (x <= 8)
                        cut[x++] = n_pairs;
                    cut[9] = 0;
                    for (int k = 0; k < 8; ++k)
                        if (cut[k + 1] - cut[k] > cut[9])
                            cut[9] = cut[k + 1] - cut[k];
                    if (m->xcd_cuts->size() > 64)
                        m->xcd_cuts->clear();
                    it = m->xcd_cuts->emplace(key, cut).first;
                }
                for (int k = 0; k < 9; ++k)
                    F.xcd_lo[k] = it->second[k];
                max_len = it->second[9];
            }
            dim3 mgrid((unsigned)(8 * max_len));
            /* tuning aid: extra (unused) LDS per workgroup caps the workgroups per CU: the kernel
             * holds 32 KB and 94 VGPRs, i.e. five workgroups per CU; 8192 makes it four */
            const size_t dyn = (size_t)(kn.mfma_lds_pad > 0 ? kn.mfma_lds_pad : 0);
            /* SSW_SCAN_AUDIT=k: the AUDIT instances redo every frame of every k-th wave exactly
             * and count the pairs where a PROVEN scan result differs (ssw_scan_audit_stats) */
            F.audit_k = kn.scan_audit;
            /* masked batches (compallsen = no): the instances whose exact pass steps over the frames
             * a codebook is not scanned in (ssw_k1a_frames.inc, carried_order_masked) */
            const bool masked = act != NULL && !ms && kn.scan_audit <= 0;
#define SSW_MFMA_LAUNCH(MSV, NS)                                                             \
    if (masked)                                                                              \
        hipLaunchKernelGGL((ptm_topn_mfma_kernel<13, false, NS, false, true>), mgrid, dim3(256), dyn, st, \
                           m->d_rec28, m->d_wfrag, m->d_recmax, m->d_exlistm, d_feats, F);   \
    else if (kn.scan_audit > 0)                                                              \
        hipLaunchKernelGGL((ptm_topn_mfma_kernel<13, MSV, NS, true>), mgrid, dim3(256), dyn, st, \
                           m->d_rec28, m->d_wfrag, m->d_recmax, m->d_exlistm, d_feats, F);   \
    else                                                                                     \
        hipLaunchKernelGGL((ptm_topn_mfma_kernel<13, MSV, NS, false>), mgrid, dim3(256), dyn, st, \
                           m->d_rec28, m->d_wfrag, m->d_recmax, m->d_exlistm, d_feats, F)
            if (nstep == 2) {
                SSW_MFMA_LAUNCH(false, 2);
            } else if (ms) {
                SSW_MFMA_LAUNCH(true, 1);
            } else {
                SSW_MFMA_LAUNCH(false, 1);
            }
#undef SSW_MFMA_LAUNCH
            return hipGetLastError();
        };
        if (pieces) {
            const int n_pieces = (n_frames + piece / 2) / piece; /* the remainder joins a piece */
            const int len = ((n_frames + n_pieces - 1) / n_pieces + 255) / 256 * 256;
            for (int lo = 0; lo < n_frames; lo += len) {
                const int hi = lo + len < n_frames ? lo + len : n_frames;
                HIP_OK(launch_scan(lo, hi));
                if (act != NULL) {
                    HIP_OK(launch_active(lo, hi));
                } else if (launch_senone(m, scorer, hi - lo, m->d_topn_cw + (size_t)lo * m->n_cbf,
                                  m->d_topn_sc + (size_t)lo * m->n_cbf,
                                  cp != NULL ? d_out : d_out + (size_t)lo * h->n_sen,
                                  hi == n_frames, st, (flags & SSW_SCORE_SHARE_DEVICE) != 0, cp,
                                  lo) < 0)
                    return -1;
            }
            F.n_frames = n_frames;
            pieced = true;
        } else if (mfma)
            HIP_OK(launch_scan(0, n_frames));
        F.frame_lo = 0;
        F.n_frames = n_frames;
        /* two frames per lane once that still fills the chip with >= 4 waves per SIMD */
        const bool two = (int64_t)((n_frames + 127) / 128) * m->n_cbf >= 2048;
        const int fpl = two ? 2 : 1;
        const int tiles = (n_frames + 64 * fpl - 1) / (64 * fpl);
        F.tile_groups = (tiles + 3) / 4;
        dim3 grid((unsigned)((((int64_t)F.tile_groups * m->n_cbf + 7) / 8) * 8));
        if (mfma)
            ;
        else if (two && ms)
            hipLaunchKernelGGL((ptm_topn_frames_kernel<13, 2, true>), grid, dim3(256), 0, st,
                               m->d_rec, m->d_recq, m->d_recmax, m->d_exlist, d_feats, F);
        else if (two && act != NULL)
            hipLaunchKernelGGL((ptm_topn_frames_kernel<13, 2, false, true>), grid, dim3(256), 0, st,
                               m->d_rec, m->d_recq, m->d_recmax, m->d_exlist, d_feats, F);
        else if (two)
            hipLaunchKernelGGL((ptm_topn_frames_kernel<13, 2, false>), grid, dim3(256), 0, st,
                               m->d_rec, m->d_recq, m->d_recmax, m->d_exlist, d_feats, F);
        else if (ms)
            hipLaunchKernelGGL((ptm_topn_frames_kernel<13, 1, true>), grid, dim3(256), 0, st,
                               m->d_rec, m->d_recq, m->d_recmax, m->d_exlist, d_feats, F);
        else if (act != NULL)
            hipLaunchKernelGGL((ptm_topn_frames_kernel<13, 1, false, true>), grid, dim3(256), 0, st,
                               m->d_rec, m->d_recq, m->d_recmax, m->d_exlist, d_feats, F);
        else
            hipLaunchKernelGGL((ptm_topn_frames_kernel<13, 1, false>), grid, dim3(256), 0, st,
                               m->d_rec, m->d_recq, m->d_recmax, m->d_exlist, d_feats, F);
        HIP_OK(hipGetLastError());
        m->stats_pending = 1;
    }
    if (m->timing && !pieced)
        HIP_OK(hipEventRecord(m->ev[1], st));
    if (pieced)
        ; /* scan and senone launches of every piece are on the stream */
    else if (act != NULL) {
        if (cp != NULL) {
            ssw_set_error("internal error: compact rows with an active set");
            return -1;
        }
        HIP_OK(launch_active(0, n_frames));
    } else if (launch_senone(m, scorer, n_frames, m->d_topn_cw, m->d_topn_sc, d_out,
                             m->stats_pending != 0, st, (flags & SSW_SCORE_SHARE_DEVICE) != 0,
                             cp, 0) < 0)
        return -1;
    if (m->timing && pieced) /* scan and senone launches alternate: no split, ms[0] = the call */
        HIP_OK(hipEventRecord(m->ev[1], st));
    if (m->timing) {
        HIP_OK(hipEventRecord(m->ev[2], st));
        m->timing_pieced = pieced ? 1 : 0;
    }
#if defined(SSW_TIMELINE) || defined(SSW_TIMELINE_SEN)
    if (getenv("SSW_TIMELINE_OUT")) {
        std::vector<unsigned long long> tl(16384 * 6);
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(g_timeline), tl.size() * 8));
        FILE *fp = fopen(getenv("SSW_TIMELINE_OUT"), "wb");
        if (fp) {
            fwrite(tl.data(), 8, tl.size(), fp);
#ifdef SSW_TIMELINE
            std::vector<unsigned long long> tl2(8192 * 8);
            HIP_OK(hipMemcpyFromSymbol(tl2.data(), HIP_SYMBOL(g_timeline2), tl2.size() * 8));
            fwrite(tl2.data(), 8, tl2.size(), fp);
#endif
            fclose(fp);
        }
    }
#endif
    return score_batch_finish(m, ms, n_frames, utt_off, n_utts, st, flags, carry_in, carry_out);
}

/* Measurement aid (DESIGN.md section 7, the first pass in the default configuration): `reps`
 * back-to-back ssw_score_batch calls on one batch, launched from C without returning to the
 * caller in between -- the scoring cost of a frame-synchronous loop that scores ONE frame of
 * every utterance per step (n_frames = n_utts), free of any binding overhead. */
extern "C" int
ssw_debug_score_loop(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                     const int32_t *utt_off, int32_t n_utts, int16_t *d_out, int32_t reps,
                     void *stream)
{
    for (int r = 0; r < reps; ++r)
        if (score_batch_impl(m, scorer, d_feats, n_frames, utt_off, n_utts, d_out, stream, 0u, NULL,
                             NULL) < 0)
            return -1;
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

/* Host buffers in, host buffers out (what a decoder that keeps nothing on the device sees:
 * acmod_score's interface, src/acmod.c:822-860).  10,252 bytes of scores leave the device per
 * frame against 156 bytes of features going in, so the call is bound by the link, and round 4's
 * form -- one blocking pageable hipMemcpy each way around the kernels -- ran at the runtime's
 * pageable-copy rate (10 GB/s, 1.0 M frames/s; profiles/r04_host_boundary.json).  Round 5: the
 * batch is cut at utterance boundaries into sub-batches of ~1024 frames (SSW_HOST_PIPE_FRAMES)
 * that go through a
 * three-stage pipeline -- (1) features into pinned staging, upload, scoring, on one stream;
 * (2) the rows' download into pinned staging on a second stream, behind an event; (3) the host
 * copy into the caller's buffer, shared by the host thread pool -- with two slots in flight, so
 * that sub-batch k is scored while k - 1 crosses the link and k - 2 lands in the caller's
 * memory.  Utterances start from the reset history (as ssw_score_batch): cutting between them
 * changes nothing. */
struct HostCopyJob {
    unsigned char *dst;
    const unsigned char *src;
    size_t bytes, chunk;
};

static void
host_copy_chunk(void *arg, int k)
{
    const HostCopyJob *j = static_cast<const HostCopyJob *>(arg);
    const size_t at = (size_t)k * j->chunk;
    const size_t n = at + j->chunk <= j->bytes ? j->chunk : j->bytes - at;
    memcpy(j->dst + at, j->src + at, n);
}

/* memcpy shared by the host threads (ssw_parallel_for); small copies stay on the caller */
static void
host_copy_parallel(void *dst, const void *src, size_t bytes)
{
    if (bytes < ((size_t)4 << 20)) {
        memcpy(dst, src, bytes);
        return;
    }
    HostCopyJob j;
    j.dst = static_cast<unsigned char *>(dst);
    j.src = static_cast<const unsigned char *>(src);
    j.bytes = bytes;
    j.chunk = (size_t)2 << 20;
    ssw_parallel_for((int)((bytes + j.chunk - 1) / j.chunk), host_copy_chunk, &j);
}

static int
host_pipe_reserve(ssw_model_s *m, size_t feat_bytes, size_t out_bytes)
{
    if (m->s_copy == NULL) {
        HIP_OK(hipStreamCreateWithFlags(&m->s_copy, hipStreamNonBlocking));
        HIP_OK(hipStreamCreateWithFlags(&m->s_pipe, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIP_OK(hipEventCreateWithFlags(&m->ev_piece[k], hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&m->ev_down[k], hipEventDisableTiming));
        }
    }
    if (feat_bytes > m->pipe_feat_cap || out_bytes > m->pipe_out_cap) {
        HIP_OK(hipDeviceSynchronize());
        for (int k = 0; k < 2; ++k) {
            if (m->h_pipe_feat[k])
                (void)hipHostFree(m->h_pipe_feat[k]);
            if (m->h_pipe_out[k])
                (void)hipHostFree(m->h_pipe_out[k]);
            (void)hipFree(m->d_pipe_feat[k]);
            (void)hipFree(m->d_pipe_out[k]);
            m->h_pipe_feat[k] = m->h_pipe_out[k] = NULL;
            m->d_pipe_feat[k] = NULL;
            m->d_pipe_out[k] = NULL;
        }
        m->pipe_feat_cap = m->pipe_out_cap = 0;
        for (int k = 0; k < 2; ++k) {
            HIP_OK(hipHostMalloc((void **)&m->h_pipe_feat[k], feat_bytes, hipHostMallocDefault));
            HIP_OK(hipHostMalloc((void **)&m->h_pipe_out[k], out_bytes, hipHostMallocDefault));
            HIP_OK(hipMalloc((void **)&m->d_pipe_feat[k], feat_bytes));
            HIP_OK(hipMalloc((void **)&m->d_pipe_out[k], out_bytes));
        }
        m->pipe_feat_cap = feat_bytes;
        m->pipe_out_cap = out_bytes;
    }
    return 0;
}

/* sub-batch size: small enough that a 4096-frame call already overlaps its three stages (four
 * sub-batches), large enough that a scoring launch pair still runs near its best rate */
#define SSW_HOST_PIPE_FRAMES 1024
extern "C" int
ssw_score_batch_host(ssw_model_t *m, int scorer, const float *feats, int32_t n_frames,
                     const int32_t *utt_off, int32_t n_utts, int16_t *out)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const ssw_host_model_t *h = m->h;
    if (n_frames <= 0)
        return 0;
    if (check_scorer_shape(m, scorer) < 0)
        return -1;
    if (feats == NULL || out == NULL || utt_off == NULL || n_utts <= 0 || utt_off[0] != 0
        || utt_off[n_utts] != n_frames) {
        ssw_set_error("ssw_score_batch_host: bad arguments");
        return -1;
    }
    for (int u = 0; u < n_utts; ++u)
        if (utt_off[u + 1] < utt_off[u]) {
            ssw_set_error("utterance offsets must be non-decreasing");
            return -1;
        }
    HIP_OK(hipSetDevice(m->device));
    refresh_knobs(m);
    /* sub-batches: whole utterances, closed once they hold SSW_HOST_PIPE_FRAMES frames; an
     * utterance of more than `cap` frames is cut into pieces of `cap` (even: the parity of its
     * frames is kept) that hand the PTM history on through carry_out / carry_in -- so the pinned
     * staging and the device rows stop growing at 2 x cap rows each (en-us: 2 x 168 MB + 2 x 168
     * MB at the default 16,384) whatever the caller sends (ADVICE r5: one 100 K-frame utterance
     * used to pin 2 x 1 GB of host memory and as much of the device for the model's lifetime) */
    struct Sub {
        int f0, f1, u0, u1; /* frames [f0, f1) of utterances [u0, u1) */
        bool cont, more;    /* continues an utterance / is continued by the next sub-batch */
    };
    std::vector<Sub> subs;
    const int cap = m->kn.host_pipe_cap;
    int longest = 0;
    for (int u = 0, a = 0; u < n_utts; ++u) {
        const int len = utt_off[u + 1] - utt_off[u];
        if (len > cap) {
            if (u > a)
                subs.push_back(Sub{ utt_off[a], utt_off[u], a, u, false, false });
            for (int f = utt_off[u]; f < utt_off[u + 1]; f += cap)
                subs.push_back(Sub{ f, std::min(f + cap, utt_off[u + 1]), u, u + 1, f > utt_off[u],
                                    f + cap < utt_off[u + 1] });
            a = u + 1;
        } else if (utt_off[u + 1] - utt_off[a] >= SSW_HOST_PIPE_FRAMES || u + 1 == n_utts) {
            subs.push_back(Sub{ utt_off[a], utt_off[u + 1], a, u + 1, false, false });
            a = u + 1;
        }
    }
    for (const Sub &S : subs)
        longest = std::max(longest, S.f1 - S.f0);
    const size_t row_in = sizeof(float) * (size_t)h->veclen_total, row_out = sizeof(int16_t) * (size_t)h->n_sen;
    /* (a sub-batch is closed by the utterance that takes it past SSW_HOST_PIPE_FRAMES: on a
     * ragged stream the longest one changes from call to call, and growing the pinned staging
     * is a device synchronisation + four allocations -- so it starts at two sub-batches' worth
     * and doubles) */
    size_t rows_cap = m->pipe_out_cap / row_out;
    if ((size_t)longest > rows_cap) {
        rows_cap = std::max(rows_cap, (size_t)2 * SSW_HOST_PIPE_FRAMES);
        while (rows_cap < (size_t)longest)
            rows_cap *= 2;
    }
    if (host_pipe_reserve(m, rows_cap * row_in, rows_cap * row_out) < 0)
        return -1;
    std::vector<uint32_t> carry((size_t)m->n_cbf, 0u);
    const int n_sub = (int)subs.size();
    std::vector<int32_t> off;
    /* the top-N workspace holds the WHOLE call (the debug view ssw_score_batch_topn speaks of
     * the last call): every sub-batch scores into its own stretch of it */
    if (!h->continuous && ensure_score_ws(m, n_frames, n_utts) < 0)
        return -1;
    uint32_t *const topn_cw0 = m->d_topn_cw;
    int4 *const topn_sc0 = m->d_topn_sc;
    struct Restore {
        ssw_model_s *m;
        uint32_t *cw;
        int4 *sc;
        int total;
        ~Restore()
        {
            m->d_topn_cw = cw;
            m->d_topn_sc = sc;
            m->last_n_frames = total;
            m->stats_accumulate = 0; /* (also on the early returns: the next call counts afresh) */
        }
    } restore_{ m, topn_cw0, topn_sc0, n_frames };
    int64_t sum_flagged = 0, sum_pairs = 0; /* ssw_score_batch_stats speaks of the whole call */
    m->stats_accumulate = 0;
    auto land = [&](int k) -> int { /* stage 3 of sub-batch k: pinned staging -> the caller's rows */
        const int slot = k & 1;
        const int f0 = subs[(size_t)k].f0, f1 = subs[(size_t)k].f1;
        HIP_OK(hipEventSynchronize(m->ev_down[slot]));
        host_copy_parallel(out + (size_t)f0 * h->n_sen, m->h_pipe_out[slot], (size_t)(f1 - f0) * row_out);
        return 0;
    };
    for (int k = 0; k < n_sub; ++k) {
        const int slot = k & 1;
        const Sub &S = subs[(size_t)k];
        const int u0 = S.u0, u1 = S.u1;
        const int f0 = S.f0, nf = S.f1 - f0;
        if (nf > 0) {
            off.resize((size_t)(u1 - u0) + 1);
            for (int u = u0; u <= u1; ++u) /* (a piece of a long utterance: [0, nf]) */
                off[(size_t)(u - u0)] = std::min(std::max(utt_off[u], f0), S.f1) - f0;
            /* (the slot's staging is free: sub-batch k - 2 landed in iteration k - 1) */
            memcpy(m->h_pipe_feat[slot], feats + (size_t)f0 * h->veclen_total, (size_t)nf * row_in);
            HIP_OK(hipMemcpyAsync(m->d_pipe_feat[slot], m->h_pipe_feat[slot], (size_t)nf * row_in,
                                  hipMemcpyHostToDevice, m->s_pipe));
            /* the device rows of this slot were downloaded by sub-batch k - 2 */
            HIP_OK(hipStreamWaitEvent(m->s_pipe, m->ev_down[slot], 0));
            if (!h->continuous) {
                m->d_topn_cw = topn_cw0 + (size_t)f0 * m->n_cbf;
                m->d_topn_sc = topn_sc0 + (size_t)f0 * m->n_cbf;
            }
            /* (carry_out makes the piece's call synchronous: a long utterance's pieces do not
             * overlap their scoring with the copies -- they are 16 K frames each) */
            const int rc = score_batch_impl(m, scorer, m->d_pipe_feat[slot], nf, off.data(), u1 - u0,
                                            m->d_pipe_out[slot], m->s_pipe, 0u,
                                            S.cont ? carry.data() : NULL, S.more ? carry.data() : NULL,
                                            NULL, NULL, NULL,
                                            /* a continuing piece keeps its utterance's frame
                                             * numbers (the ds phase); grouped utterances start at 0 */
                                            S.cont ? f0 - utt_off[u0] : 0);
            m->d_topn_cw = topn_cw0;
            m->d_topn_sc = topn_sc0;
            if (rc < 0)
                return -1;
            sum_pairs += m->stats[1];
            sum_flagged += m->stats_pending ? 0 : m->stats[0]; /* (the chain kernel: counted on the host) */
            m->stats_accumulate = 1; /* the next sub-batch's count joins this one's on the device */
            HIP_OK(hipEventRecord(m->ev_piece[slot], m->s_pipe));
            HIP_OK(hipStreamWaitEvent(m->s_copy, m->ev_piece[slot], 0));
            HIP_OK(hipMemcpyAsync(m->h_pipe_out[slot], m->d_pipe_out[slot], (size_t)nf * row_out,
                                  hipMemcpyDeviceToHost, m->s_copy));
        }
        HIP_OK(hipEventRecord(m->ev_down[slot], m->s_copy));
        if (k > 0 && land(k - 1) < 0)
            return -1;
    }
    m->stats_accumulate = 0;
    if (land(n_sub - 1) < 0)
        return -1;
    HIP_OK(hipStreamSynchronize(m->s_pipe));
    m->stats[1] = sum_pairs;
    if (!m->stats_pending)
        m->stats[0] = sum_flagged;
    return 0;
}

extern "C" int
ssw_score_batch_topn(ssw_model_t *m, int32_t n_frames, uint8_t *cw, int32_t *score)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    if (cont_refuse(m, "ssw_score_batch_topn") < 0)
        return -1;
    if (n_frames > m->last_n_frames) {
        ssw_set_error("only %d frames were scored", m->last_n_frames);
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(cw, m->d_topn_cw, (size_t)n_frames * m->n_cbf * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(score, m->d_topn_sc, (size_t)n_frames * m->n_cbf * 16,
                     hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int
ssw_set_kernel_timing(ssw_model_t *m, int enable)
{
    HIP_OK(hipSetDevice(m->device));
    if (enable && !m->timing) {
        for (int i = 0; i < 3; ++i)
            HIP_OK(hipEventCreate(&m->ev[i]));
        HIP_OK(hipEventCreate(&m->ev_sc));
        m->timing = 1;
    } else if (!enable && m->timing) {
        for (int i = 0; i < 3; ++i)
            (void)hipEventDestroy(m->ev[i]);
        (void)hipEventDestroy(m->ev_sc);
        m->timing = 0;
    }
    return 0;
}

extern "C" int
ssw_get_kernel_timing(ssw_model_t *m, float *ms, int n)
{
    if (!m->timing) {
        ssw_set_error("kernel timing is off");
        return -1;
    }
    HIP_OK(hipEventSynchronize(m->ev[2]));
    if (m->timing_pieced) { /* one number: the whole call (scan and senone launches alternate) */
        if (n >= 1)
            HIP_OK(hipEventElapsedTime(&ms[0], m->ev[0], m->ev[2]));
        if (n >= 2)
            ms[1] = 0.0f;
        return n >= 1 ? 1 : 0;
    }
    int k = 0;
    for (; k < 2 && k < n; ++k)
        HIP_OK(hipEventElapsedTime(&ms[k], m->ev[k], m->ev[k + 1]));
    if (m->timing_semi && n >= 3) { /* the s2_semi scorer: the chain kernel's share of ms[0] */
        HIP_OK(hipEventElapsedTime(&ms[2], m->ev_sc, m->ev[1]));
        k = 3;
    }
    return k;
}

extern "C" int
ssw_score_batch_stats(ssw_model_t *m, int64_t stats[2])
{
    if (m->stats_pending) {
        unsigned long long n = 0;
        HIP_OK(hipSetDevice(m->device));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(&n, m->d_nfixed + 1, sizeof(n), hipMemcpyDeviceToHost));
        m->stats[0] = (int64_t)n; /* moved there by the last batch's senone kernel */
        m->stats_pending = 0;
    }
    stats[0] = m->stats[0];
    stats[1] = m->stats[1];
    return 0;
}

/* SSW_SCAN_AUDIT=k (round 5): [0] = (codebook x stream, frame) pairs the matrix-core scan had
 * PROVEN and an audited wave redid exactly all the same, [1] = of those, pairs whose exact
 * result (codeword order or scores) differs from what the scan wrote -- 0 unless the scan's
 * bound does not hold on this device.  Running totals since the model was loaded. */
extern "C" int
ssw_scan_audit_stats(ssw_model_t *m, int64_t stats[2])
{
    stats[0] = stats[1] = 0;
    if (m->device == SSW_DEVICE_NONE || m->d_nfixed == NULL)
        return 0;
    unsigned long long n[2] = { 0, 0 };
    HIP_OK(hipSetDevice(m->device));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(n, m->d_nfixed + 2, sizeof(n), hipMemcpyDeviceToHost));
    stats[0] = (int64_t)n[0];
    stats[1] = (int64_t)n[1];
    return 0;
}

extern "C" int
ssw_debug_scan_keys(ssw_model_t *m, const float *d_feats, int32_t n_frames, int32_t cbf,
                    float *keys)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const ssw_host_model_t *h = m->h;
    if (cont_refuse(m, "ssw_debug_scan_keys") < 0)
        return -1;
    if (m->device == SSW_DEVICE_NONE || m->d_wfrag == NULL) {
        ssw_set_error("no matrix-core scan tables for this model (or no device)");
        return -1;
    }
    if (n_frames <= 0 || cbf < 0 || cbf >= m->n_cbf || d_feats == NULL || keys == NULL) {
        ssw_set_error("ssw_debug_scan_keys: bad arguments");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    float *d_out = NULL;
    HIP_OK(hipMalloc((void **)&d_out, sizeof(float) * 128 * (size_t)n_frames));
    hipLaunchKernelGGL((ptm_mfma_keys_kernel<13>), dim3((n_frames + 127) / 128), dim3(64), 0, 0,
                       m->d_wfrag, m->d_recmax, d_feats, n_frames, h->veclen_total,
                       h->featoff[cbf % h->n_feat], cbf, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpy(keys, d_out, sizeof(float) * 128 * (size_t)n_frames, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    HIP_OK(e);
    return 0;
}

/* The scan's selection on caller-supplied keys (host pointers): keys [n_frames][128] by density;
 * idx and top [n_frames][5] = the densities of the five best keys of every frame, best first, and
 * those keys with the 7 label bits cleared (ptm_scan_top5_debug_kernel).  Needs a device, no
 * particular model: tests/test_gpu_scan_top5.py. */
extern "C" int
ssw_debug_scan_top5(ssw_model_t *m, const float *keys, int32_t n_frames, int32_t *idx, float *top)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    if (cont_refuse(m, "ssw_debug_scan_top5") < 0)
        return -1;
    if (m->device == SSW_DEVICE_NONE || n_frames <= 0 || !keys || !idx || !top) {
        ssw_set_error("ssw_debug_scan_top5: no device or bad arguments");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    const size_t nk = sizeof(float) * 128 * (size_t)n_frames, no = 4 * 5 * (size_t)n_frames;
    unsigned char *d = NULL;
    HIP_OK(hipMalloc((void **)&d, nk + 2 * no));
    hipError_t e = hipMemcpy(d, keys, nk, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ptm_scan_top5_debug_kernel, dim3((unsigned)((n_frames + 63) / 64)),
                           dim3(64), 0, 0, reinterpret_cast<const float *>(d), n_frames,
                           reinterpret_cast<int32_t *>(d + nk), reinterpret_cast<float *>(d + nk + no));
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpy(idx, d + nk, no, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(top, d + nk + no, no, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_OK(e);
    return 0;
}

/* D = A B + C on the matrix cores, one v_mfma_f32_32x32x16_f16 per tile (host pointers; A and B
 * are binary16 bit patterns): tests/test_gpu_mfma_bound.py measures the instruction's
 * accumulation error with it against the eps the scan's bound assumes (ssw_model.c). */
extern "C" int
ssw_debug_mfma_f16_tiles(ssw_model_t *m, const uint16_t *A, const uint16_t *B, const float *C,
                         float *D, int32_t n_tiles)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    if (m->device == SSW_DEVICE_NONE || n_tiles <= 0 || !A || !B || !C || !D) {
        ssw_set_error("ssw_debug_mfma_f16_tiles: no device or bad arguments");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    const size_t na = (size_t)n_tiles * 32 * 16 * 2, nc = (size_t)n_tiles * 32 * 32 * 4;
    unsigned char *d = NULL;
    HIP_OK(hipMalloc((void **)&d, 2 * na + 2 * nc));
    hipError_t e = hipMemcpy(d, A, na, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(d + na, B, na, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(d + 2 * na, C, nc, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mfma_f16_tile_kernel, dim3((unsigned)n_tiles), dim3(64), 0, 0,
                           reinterpret_cast<const _Float16 *>(d),
                           reinterpret_cast<const _Float16 *>(d + na),
                           reinterpret_cast<const float *>(d + 2 * na),
                           reinterpret_cast<float *>(d + 2 * na + nc));
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpy(D, d + 2 * na + nc, nc, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_OK(e);
    return 0;
}
