/* ssw_host_score.inc -- host: batched scoring entry points.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* The scoring workspace for `rows` rows of the top-N block and a batch of n_utts utterances in
 * them.  Grow-only: the top-N pair of exactly `rows` rows, the meta buffer of the largest
 * utterance count and bit count seen (the *_hint maxima).  Refuses a block whose index does not
 * fit 32 bits before anything is allocated; forgets the cached offsets when the meta buffer moves. */
static int
ensure_score_ws(ssw_model_s *m, size_t rows, int n_utts)
{
    ScoreWs &w = m->sw;
    const uint64_t pairs = (uint64_t)rows * (uint64_t)m->n_cbf;
    if (pairs > 0xffffffffull) {
        ssw_set_error("batch of %d frames is too large (frames x codebooks x streams must fit 32 bits)",
                      (int)rows);
        return -1;
    }
    if (devbuf_reserve(w.topn_cw, sizeof(uint32_t) * (size_t)pairs, "ssw_score_batch") < 0
        || devbuf_reserve(w.topn_sc, sizeof(int4) * (size_t)pairs, "ssw_score_batch") < 0)
        return -1;
    if (w.d_nfixed == NULL) {
        if (dev_alloc(&w.d_nfixed, 4) < 0)
            return -1;
        HIP_OK(hipMemset(w.d_nfixed, 0, 4 * sizeof(unsigned long long)));
    }
    const size_t need_bits = 2 * ((rows + 31) / 32 + 2);
    if ((size_t)n_utts + 1 > w.ws_utts || need_bits > w.ws_bits) {
        const size_t wu = std::max((size_t)n_utts + 1, w.ws_utts_hint), wb = std::max(need_bits, w.ws_bits_hint);
        bool moved = false; /* (always, here: wu + wb is more than the buffer holds) */
        w.ws_utts = w.ws_bits = 0;
        const int rc = devbuf_reserve(w.meta, sizeof(uint32_t) * (wu + wb), "ssw_score_batch", 0, &moved);
        if (moved && w.utt_cache)
            w.utt_cache->clear(); /* everything has to be uploaded again */
        if (rc < 0)
            return -1;
        w.ws_utts = w.ws_utts_hint = wu;
        w.ws_bits = w.ws_bits_hint = wb;
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
    /* the reference's add table has more than 256 entries below a base of about 1.000018, and
     * its fast_logmath_add reads them all (tied_mgau_common.h:100-117); the kernels hold 256 and
     * take 0 beyond */
    if (h->logadd8_size != 256) {
        ssw_set_error("PTM scorer: unsupported log-add table (%d entries, the kernels hold 256)",
                      h->logadd8_size);
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

/* the model's part of a chain kernel's parameters; the caller names the top-N rows it writes */
static void
fill_chain_params(const ssw_model_s *m, ChainParams &P, const float *d_feats)
{
    const ssw_host_model_t *h = m->h;
    memset(&P, 0, sizeof(P));
    P.rec = m->d_rec;
    P.feats = d_feats;
    P.utt_off = m->sw.utt_off();
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
    return h->cfg.aw == 1 && !m->ms_raw && n_frames >= 4 * 512 && h->n_cb <= 64
        && 255 + 640 + 6 * m->logadd_max < SSW_LOGADD_MIRROR && m->fold_hb[1] <= 255
        && !m->kn.ms_senone_old;
}

/* per-frame active sets of a compallsen = no batch (device pointers; ssw_host_active.inc) */
struct ActiveSets {
    const int32_t *seg_of_frame;
    const unsigned long long *seg_cbmask;
    SenoneActive2Params *a2; /* filled by the caller but for the top-N block and the model's tables */
    /* or (a2 == NULL): a listed set per frame as a bitmap, ssw_k7_fpactive.inc -- listed, cbmask,
     * out, full, cap are the caller's, the rest is filled here */
    const SenoneListedParams *ls;
    /* a continuous model (ls: listed, out, full, cap, yes are read): NULL, or the bitmap row of
     * every frame of the call where frames share rows (cont_align_active) */
    const int32_t *row_of_frame;
};

/* One scoring call.  `ScoreReq R{}` is all zeros; a caller names what it sets. */
struct ScoreReq {
    int scorer;
    const float *d_feats;    /* device, [n_frames][veclen_total] */
    int32_t n_frames;
    const int32_t *utt_off;  /* host, [n_utts + 1] */
    int32_t n_utts;
    int16_t *d_out;          /* device rows, [n_frames][n_sen]; with cp: the compact buffer */
    void *stream;
    uint32_t flags;          /* SSW_SCORE_* */
    const uint32_t *carry_in; /* host [n_cbf] or NULL: the history the first utterance starts from */
    uint32_t *carry_out;      /* host [n_cbf] or NULL: read back, which makes the call synchronous */
    const ActiveSets *act;    /* compallsen = no: score the active sets only */
    const uint32_t *d_carry_rows; /* device [n_utts][n_cbf]: a history row per utterance */
    /* compact rows (ssw_host_compact.inc): only for launches that take the persistent senone
     * kernel (the caller checks senone_compact_ok) */
    const ssw_compact_plan_s *cp;
    /* a call that continues an utterance (a piece of ssw_score_batch_host's cut): the in-utterance
     * number of its frame 0, which decides the frames a ds > 1 model re-scans on */
    int frame_base;
    /* the row of the model's top-N workspace that frame 0 writes: 0, but in the pieces of
     * ssw_score_batch_host, whose workspace holds the whole call */
    int topn_row0;
};

/* What the steps of one call share: the request and what score_batch_impl derives from it once. */
struct ScoreCall {
    ssw_model_s *m;
    const ScoreReq &R;
    hipStream_t st;
    bool ms;      /* the ms scorer: no history, no chain */
    /* history carried from utterance to utterance (the reference never resets it after
     * start-up, src/acmod.c:367): the batch is one chain, only its first frame is a start.  The
     * chain follows the reference's two-slot ring (src/ptm_mgau.c:425-437): frame numbers restart
     * with every utterance and its frame 0 copies slot 1, so the last frame of an utterance of odd
     * length is off the chain (`skip` bits in score_upload_meta; a one-frame utterance entirely) */
    bool chain;
    uint32_t *cw; /* the top-N rows of frame 0: the workspace's + topn_row0 rows */
    int4 *sc;
};

/* The senone kernel of frames [lo, hi) of the call, from their top-N rows.  With R.cp the rows
 * are compact: d_out is the compact buffer and lo goes to the kernel as the batch frame number of
 * the launch's first frame.  move_stats: the launch moves the exact pass's count to d_nfixed[1]. */
static int
launch_senone(const ScoreCall &C, int lo, int hi, bool move_stats)
{
    ssw_model_s *m = C.m;
    const ssw_host_model_t *h = m->h;
    const int scorer = C.R.scorer, n_frames = hi - lo;
    const ssw_compact_plan_s *cp = C.R.cp;
    hipStream_t st = C.st;
    SenoneParams S;
    memset(&S, 0, sizeof(S));
    S.topn_cw = C.cw + (size_t)lo * m->n_cbf;
    S.topn_sc = C.sc + (size_t)lo * m->n_cbf;
    S.mixw = scorer == SSW_SCORER_MS ? m->d_ms_pdf : m->d_mixw;
    S.aw = h->cfg.aw;
    S.zero = h->zero8;
    S.raw = m->ms_raw;
    S.quad_cb = m->d_quad_cb;
    S.quad_info = m->d_quad_info;
    S.slot_sen = m->d_slot_sen;
    S.logadd8 = m->d_logadd8;
    S.logadd_mirror = m->d_logadd_mirror + (scorer == SSW_SCORER_MS ? SSW_LOGADD_MIRROR : 0);
    S.nfixed = move_stats ? m->sw.d_nfixed : NULL;
    S.nfixed_acc = m->sw.stats_accumulate;
    S.out = cp != NULL ? C.R.d_out : C.R.d_out + (size_t)lo * h->n_sen;
    if (cp != NULL) {
        S.utt_of_frame = cp->d_utt_of_frame;
        S.cutt_off = cp->d_frame_off;
        S.cstride = cp->d_cstride;
        S.crow_off = cp->d_crow_off;
        S.cpos = cp->d_cpos;
        S.frame_base = lo;
    }
    S.n_frames = n_frames;
    S.n_cb = h->n_cb;
    S.n_feat = h->n_feat;
    S.n_density = h->n_density;
    S.n_sen = h->n_sen;
    S.slot_stride = m->slot_stride;
    S.n_quads = m->n_quads;
    S.tab_max = m->logadd_max;
    S.hb = m->fold_hb[scorer == SSW_SCORER_MS ? 1 : 0];
    /* the PTM kernel indexes its folded table with 512 + x - y, x >= -3 tab_max, y <= 255 + 96,
     * and the table's entries are bytes only up to Hb = 255 (ssw_senone_lds.inc) */
    if (scorer != SSW_SCORER_MS
        && (255 + SSW_MAX_NEG_ASCR + 3 * S.tab_max >= SSW_LOGADD_LDS || S.hb > 255)) {
        ssw_set_error("unsupported log-add table (largest entry %d, folded height %d)", S.tab_max,
                      S.hb);
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
    const bool ms_packed = !ptm && ms_takes_packed_kernel(m, n_frames);
    if (cp != NULL && !ptm && !ms_packed) {
        ssw_set_error("internal error: compact rows asked of the un-packed ms senone kernel");
        return -1;
    }
    /* (about seven waves per group at two frames; at least 256 threads: the prologue copies the
     * 256-entry table with the first 256 -- senone_shape, ssw_slot_layout.inc, which the choice of
     * the slot layout evaluates as well) */
    const SenoneShape shape = senone_shape(m->n_quads, fpb, ptm || ms_packed, kn.sen_r,
                                           SEN_MAX_THREADS);
    const int R = shape.R, threads = shape.threads;
    if (threads > SEN_MAX_THREADS || (scorer == SSW_SCORER_MS && threads < m->n_cbf)) {
        ssw_set_error("unsupported senone/codebook shape (%d quads, %d codebook x stream)",
                      m->n_quads, m->n_cbf);
        return -1;
    }
    if (scorer == SSW_SCORER_MS && !ms_packed) {
        lds = MsSenoneCarve(m->n_cbf).bytes();
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
    lds = SenoneCarve(fpb, m->n_cbf, h->n_cb, ms_packed).bytes();
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
    if ((C.R.flags & SSW_SCORE_SHARE_DEVICE) != 0 && groups < (n_units + 7) / 8)
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

/* what SenoneListedParams and SenoneActive2Params share: the top-N rows of frames [lo, hi) and
 * the model's tables */
template <typename Params>
static void
fill_active_common(const ScoreCall &C, Params &A, int lo, int hi)
{
    const ssw_model_s *m = C.m;
    const ssw_host_model_t *h = m->h;
    A.topn_cw = C.cw + (size_t)lo * m->n_cbf;
    A.topn_sc = C.sc + (size_t)lo * m->n_cbf;
    A.mixw = C.ms ? m->d_ms_pdf : m->d_mixw;
    A.logadd8 = m->d_logadd8;
    A.n_frames = hi - lo;
    A.frame_base = lo;
    A.n_cb = h->n_cb;
    A.n_feat = h->n_feat;
    A.n_density = h->n_density;
    A.n_sen = h->n_sen;
    A.slot_stride = m->slot_stride;
    A.zero = h->zero8;
    A.aw = h->cfg.aw;
}

/* compallsen = no: the senone kernel of frames [lo, hi) over R.act's sets (ssw_host_active.inc /
 * ssw_host_fpactive.inc filled the segment tables; four frames per workgroup, a wave each).
 * Reads the frames' top-N rows; the kernels write where the caller's parameter block says. */
static hipError_t
launch_active(const ScoreCall &C, int lo, int hi)
{
    const ssw_model_s *m = C.m;
    const ssw_host_model_t *h = m->h;
    const ActiveSets *act = C.R.act;
    const bool ms = C.ms;
    hipStream_t st = C.st;
    const dim3 grid((unsigned)((hi - lo + 3) / 4));
    if (act->a2 == NULL) {
        SenoneListedParams L = *act->ls;
        fill_active_common(C, L, lo, hi);
        L.sen2cb = m->d_sen2cb;
        L.sen_slot = m->d_sen_slot;
        L.nw32 = (h->n_sen + 31) / 32;
        if (L.cap <= 0 || L.cap > h->n_sen)
            L.cap = h->n_sen; /* (the caller's bound on a frame's listed entries) */
        const size_t lds = ListedCarve(ms, m->n_cbf, L.cap).bytes();
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
    fill_active_common(C, A, lo, hi);
    const size_t lds = Active2Carve(ms, m->n_cbf, A.cap, h->n_sen, A.out_full != NULL).bytes();
    if (ms)
        hipLaunchKernelGGL(senone_active2_kernel<true>, grid, dim3(256), lds, st, A);
    else
        hipLaunchKernelGGL(senone_active2_kernel<false>, grid, dim3(256), lds, st, A);
    return hipGetLastError();
}

/* The sequential top-N scan: frame down-sampling (and SSW_PTM_EXACT) makes every frame depend on
 * its predecessor, so a wave walks each chain exactly.  Writes the call's top-N rows. */
static hipError_t
launch_scan_chain(const ScoreCall &C, const ChainParams &P)
{
    const int n_chain = (C.chain ? 1 : C.R.n_utts) * C.m->n_cbf;
    hipLaunchKernelGGL((ptm_topn_chain_kernel<13, 2, 4>), dim3((n_chain + 3) / 4), dim3(256), 0, C.st, P);
    return hipGetLastError();
}

/* what both frame-parallel scans read: the call's top-N rows, the uploaded offsets and bits, the
 * carried rows; frame_lo, n_frames and tile_groups are the launch's */
static void
fill_frames_params(const ScoreCall &C, FramesParams &F)
{
    const ssw_model_s *m = C.m;
    const ssw_host_model_t *h = m->h;
    const ScoreReq &R = C.R;
    memset(&F, 0, sizeof(F));
    F.topn_cw = C.cw;
    F.topn_sc = C.sc;
    F.utt_start = m->sw.utt_start();
    F.carry0 = (R.carry_in != NULL && !C.ms) ? m->carry0.as<uint32_t>() : NULL;
    F.carry_rows = C.ms ? NULL : R.d_carry_rows;
    F.utt_off = m->sw.utt_off();
    F.n_utts = R.n_utts;
    F.chain_skip = C.chain ? m->sw.utt_start() + m->sw.meta_nw : NULL;
    F.seg_of_frame = R.act ? R.act->seg_of_frame : NULL;
    F.seg_cbmask = R.act ? R.act->seg_cbmask : NULL;
    F.n_fixed = m->sw.d_nfixed;
    F.n_frames = R.n_frames;
    F.n_cbf = m->n_cbf;
    F.n_feat = h->n_feat;
    F.featdim = h->veclen_total;
    for (int f = 0; f < h->n_feat; ++f)
        F.featoff[f] = h->featoff[f];
}

/* The matrix-core scan of frames [lo, hi) (one wave = 64 frames of one codebook x stream).  The
 * scan of a piece takes absolute frame numbers (its exact pass may walk back into the piece
 * before).  Sets F's frame_lo, n_frames, tile_groups, xcd_lo and audit_k. */
static hipError_t
launch_scan_mfma(const ScoreCall &C, FramesParams &F, int lo, int hi)
{
    ssw_model_s *m = C.m;
    const Knobs &kn = m->kn;
    const bool ms = C.ms;
    const float *d_feats = C.R.d_feats;
    hipStream_t st = C.st;
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
    /* the cut into one chunk per XCD (xcd_cut, ssw_xcd_cut.inc) depends on the number of tile
     * groups only: computed once per shape (round 5: it used to be recomputed on every launch) */
    const int key = F.tile_groups * 2 + (kn.mfma_balance ? 1 : 0);
    if (m->sw.xcd_cuts == NULL)
        m->sw.xcd_cuts = new std::map<int, std::array<int, 10>>();
    auto it = m->sw.xcd_cuts->find(key);
    if (it == m->sw.xcd_cuts->end()) {
        if (m->sw.xcd_cuts->size() > 64)
            m->sw.xcd_cuts->clear();
        it = m->sw.xcd_cuts->emplace(key, xcd_cut(m->n_cbf, F.tile_groups, m->h->exlistm,
                                                  SSW_EXLIST_STRIDE, kn.mfma_balance)).first;
    }
    for (int k = 0; k < 9; ++k)
        F.xcd_lo[k] = it->second[k];
    const int max_len = it->second[9];
    dim3 mgrid((unsigned)(8 * max_len));
    /* tuning aid: extra (unused) LDS per workgroup caps the workgroups per CU: the kernel
     * holds 32 KB and 94 VGPRs, i.e. five workgroups per CU; 8192 makes it four */
    const size_t dyn = (size_t)(kn.mfma_lds_pad > 0 ? kn.mfma_lds_pad : 0);
    /* SSW_SCAN_AUDIT=k: the AUDIT instances redo every frame of every k-th wave exactly
     * and count the pairs where a PROVEN scan result differs (ssw_scan_audit_stats) */
    F.audit_k = kn.scan_audit;
    /* masked batches (compallsen = no): the instances whose exact pass steps over the frames
     * a codebook is not scanned in (ssw_scan_common.inc, carried_order_masked) */
    const bool masked = C.R.act != NULL && !ms && kn.scan_audit <= 0;
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
}

/* The vector-unit scan of the whole call (SSW_SCAN=fma, a device that failed the matrix-core
 * self-test, streams that are not 13-dimensional).  Sets F's frame_lo, n_frames, tile_groups. */
static hipError_t
launch_scan_frames(const ScoreCall &C, FramesParams &F)
{
    const ssw_model_s *m = C.m;
    const int n_frames = C.R.n_frames;
    const bool ms = C.ms, act = C.R.act != NULL;
    const float *d_feats = C.R.d_feats;
    hipStream_t st = C.st;
    F.frame_lo = 0;
    F.n_frames = n_frames;
    /* two frames per lane once that still fills the chip with >= 4 waves per SIMD */
    const bool two = (int64_t)((n_frames + 127) / 128) * m->n_cbf >= 2048;
    const int fpl = two ? 2 : 1;
    const int tiles = (n_frames + 64 * fpl - 1) / (64 * fpl);
    F.tile_groups = (tiles + 3) / 4;
    dim3 grid((unsigned)((((int64_t)F.tile_groups * m->n_cbf + 7) / 8) * 8));
#define SSW_FRAMES_LAUNCH(...)                                                               \
    hipLaunchKernelGGL((ptm_topn_frames_kernel<13, __VA_ARGS__>), grid, dim3(256), 0, st,    \
                       m->d_rec, m->d_recq, m->d_recmax, m->d_exlist, d_feats, F)
    if (two && ms)
        SSW_FRAMES_LAUNCH(2, true);
    else if (two && act)
        SSW_FRAMES_LAUNCH(2, false, true);
    else if (two)
        SSW_FRAMES_LAUNCH(2, false);
    else if (ms)
        SSW_FRAMES_LAUNCH(1, true);
    else if (act)
        SSW_FRAMES_LAUNCH(1, false, true);
    else
        SSW_FRAMES_LAUNCH(1, false);
#undef SSW_FRAMES_LAUNCH
    return hipGetLastError();
}

/* batches from this many frames take the matrix-core scan.  Rounds 2-3: 2,049, where the bf16
 * form caught up with the vector-unit scan; the binary16 form of round 4 is ahead at every
 * size measured -- 256 frames: 15.7 against 27.6 us, 1,024: 17.9 against 30.4, 2,048: 23.2
 * against 44.4 (DESIGN.md section 5) -- so every batch takes it; SSW_SCAN=fma or a larger
 * SSW_MFMA_MIN_FRAMES keep the vector-unit scan (tests, A/B) */
#define SSW_MFMA_MIN_FRAMES_DEFAULT 1

/* The offsets of a batch: utt_off[0 .. n_utts] runs from 0 to n_frames and never falls.  `bad` is
 * the caller's message for anything but a falling offset.  Reads host memory only. */
static int
score_check_batch(const int32_t *utt_off, int32_t n_utts, int32_t n_frames, const char *bad)
{
    if (n_frames < 0 || n_utts < 0 || utt_off == NULL || !utt_off_spans(utt_off, n_utts, n_frames)) {
        ssw_set_error("%s", bad);
        return -1;
    }
    for (int u = 0; u < n_utts; ++u)
        if (utt_off[u + 1] < utt_off[u]) {
            ssw_set_error("utterance offsets must be non-decreasing");
            return -1;
        }
    return 0;
}

/* carry_in names codewords of the model, and the device has room for a row per utterance
 * (m->carry0, which score_upload_meta fills) */
static int
score_check_carry(const ScoreCall &C)
{
    ssw_model_s *m = C.m;
    const uint32_t *carry_in = C.R.carry_in;
    for (int i = 0; i < m->n_cbf; ++i)
        for (int k = 0; k < 4; ++k)
            if (((carry_in[i] >> (8 * k)) & 0xffu) >= (uint32_t)m->h->n_density) {
                ssw_set_error("carry_in[%d] names codeword %u of %d", i,
                              (carry_in[i] >> (8 * k)) & 0xffu, m->h->n_density);
                return -1;
            }
    return devbuf_reserve(m->carry0, sizeof(uint32_t) * (size_t)m->n_cbf * (size_t)C.R.n_utts,
                          "ssw_score_batch_ex");
}

/* What the call uploads, on its stream: the carried rows (want_carry: m->carry0, a row per
 * utterance) and -- when they differ from the last call's -- the offsets, start bits and skip
 * bits (the meta buffer; m->sw.utt_cache and meta_nw then describe it).  One pinned slot, at most
 * two copies, the slot's event behind them. */
static int
score_upload_meta(const ScoreCall &C, bool want_carry)
{
    ssw_model_s *m = C.m;
    ScoreWs &w = m->sw;
    const int32_t *utt_off = C.R.utt_off;
    const int n_utts = C.R.n_utts, n_frames = C.R.n_frames;
    const bool chain = C.chain;
    /* the offsets rarely change between calls of one job: upload only when they do
     * (cache key: the chain flag, then the offsets) */
    if (w.utt_cache == NULL)
        w.utt_cache = new std::vector<int32_t>();
    const bool new_offsets = w.utt_cache->size() != (size_t)n_utts + 2
        || (*w.utt_cache)[0] != (chain ? 1 : 0)
        || memcmp(w.utt_cache->data() + 1, utt_off, sizeof(int32_t) * ((size_t)n_utts + 1)) != 0;
    if (!want_carry && !new_offsets)
        return 0;
    /* one pinned slot for everything this call uploads: [carry rows][offsets][starts][skip] */
    const size_t ncar = want_carry ? (size_t)m->n_cbf * (size_t)n_utts : 0;
    const size_t nw = ((size_t)n_frames + 31) / 32 + 1;
    const size_t b_car = sizeof(uint32_t) * ncar;
    const size_t b_off = new_offsets ? sizeof(int32_t) * ((size_t)n_utts + 1) : 0;
    const size_t b_bits = new_offsets ? sizeof(uint32_t) * nw : 0;
    int slot = 0;
    unsigned char *hs = stage_acquire(m, b_car + sizeof(uint32_t) * w.ws_utts + 2 * b_bits + 64, &slot);
    if (hs == NULL)
        return -1;
    if (want_carry) {
        /* [n_utts][n_cbf]: the first utterance starts from carry_in, the others from the
         * reset history (the chain kernel reads a row per utterance, the scans only row 0) */
        uint32_t *car = reinterpret_cast<uint32_t *>(hs);
        for (size_t i = 0; i < ncar; ++i)
            car[i] = SSW_ORDER_RESET;
        memcpy(car, C.R.carry_in, sizeof(uint32_t) * (size_t)m->n_cbf);
        HIP_OK(hipMemcpyAsync(m->carry0.as<uint32_t>(), car, b_car, hipMemcpyHostToDevice, C.st));
    }
    if (new_offsets) {
        w.utt_cache->assign(1, chain ? 1 : 0);
        w.utt_cache->insert(w.utt_cache->end(), utt_off, utt_off + n_utts + 1);
        /* staged as it lies on the device: offsets (ws_utts words), start bits, skip bits */
        int32_t *hoff = reinterpret_cast<int32_t *>(hs + b_car);
        uint32_t *starts = reinterpret_cast<uint32_t *>(hoff + w.ws_utts);
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
        w.meta_nw = nw;
        HIP_OK(hipMemcpyAsync(w.utt_off(), hoff, sizeof(uint32_t) * (w.ws_utts + 2 * nw),
                              hipMemcpyHostToDevice, C.st));
    }
    return stage_release(m, slot, C.st);
}

/* the senone kernel of frames [lo, hi): over the active sets, or all senones */
static int
launch_senone_or_active(const ScoreCall &C, int lo, int hi, bool move_stats)
{
    if (C.R.act == NULL)
        return launch_senone(C, lo, hi, move_stats);
    HIP_OK(launch_active(C, lo, hi));
    return 0;
}

/* Large batches go through the two kernels in PIECES of ~16 K frames (round 3): measured
 * per frame, scan + senone cost 19.7 ns at 4,096 frames per launch (ramp and tail), 16.3
 * at 16,384, 17.3 at 65,536 and 18.3 at 262,144 -- a piece's top-N block (41 MB) is read
 * back by its senone launch while the memory-side cache still holds it, a whole batch's
 * (660 MB at 262,144 frames) is not.  The scan of a piece takes absolute frame numbers
 * (its exact pass may walk back into the piece before); the senone kernel has no
 * dependency between frames and gets offset pointers.  `piece` = SSW_SCORE_PIECE = frames per
 * piece (a multiple of 256).  Leaves scan and senone launches of every piece on the stream; the
 * last piece's senone launch moves the exact pass's count. */
static int
score_pieces(const ScoreCall &C, FramesParams &F, int piece)
{
    const int n_frames = C.R.n_frames;
    const int n_pieces = (n_frames + piece / 2) / piece; /* the remainder joins a piece */
    const int len = ((n_frames + n_pieces - 1) / n_pieces + 255) / 256 * 256;
    for (int lo = 0; lo < n_frames; lo += len) {
        const int hi = lo + len < n_frames ? lo + len : n_frames;
        HIP_OK(launch_scan_mfma(C, F, lo, hi));
        if (launch_senone_or_active(C, lo, hi, hi == n_frames) < 0)
            return -1;
    }
    return 0;
}

/* development builds (make timeline): the kernels' time stamps to the file SSW_TIMELINE_OUT names;
 * synchronises the stream */
static int
score_timeline_dump(hipStream_t st)
{
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
#else
    (void)st;
#endif
    return 0;
}

/* What every scoring call ends in, for every scorer family: the counters, what the debug view
 * may show, and carry_out.
 *   exact_pairs: the (frame, codebook x stream) pairs the exact form took, counted on the host
 *     (0, or all of them under the chain kernel); < 0: the scans counted them on the device and
 *     the senone launch moved the count (ssw_score_batch_stats fetches it)
 *   history: the family keeps one (PTM, s2_semi); the others hand back the reset order
 *   topn: the call left a top-N block for ssw_score_batch_topn (all but continuous models)
 * Reads carry_out from the top-N rows, which makes such a call synchronous. */
static int
score_batch_finish(const ScoreCall &C, int64_t exact_pairs, bool history, bool topn)
{
    ssw_model_s *m = C.m;
    const ScoreReq &R = C.R;
    const int32_t n_frames = R.n_frames, n_utts = R.n_utts;
    const int32_t *utt_off = R.utt_off;
    const uint32_t *carry_in = R.carry_in;
    uint32_t *carry_out = R.carry_out;
    if (exact_pairs >= 0)
        m->sw.stats[0] = exact_pairs;
    m->sw.stats_pending = exact_pairs < 0;
    m->sw.last_n_frames = topn ? n_frames : 0;
    m->sw.stats[1] = (int64_t)n_frames * m->n_cbf;
    if (carry_out == NULL)
        return 0;
    if (!history) {
        for (int i = 0; i < m->n_cbf; ++i)
            carry_out[i] = SSW_ORDER_RESET; /* the ms scorer keeps no history */
        return 0;
    }
    /* what the next call starts from.  Default: the last frame's final order (the next call
     * continues the same utterance).  SSW_SCORE_CARRY_OUT_REWIND: history slot 1 of the
     * reference's ring, which is what frame 0 of the NEXT utterance -- or of the second pass
     * after acmod_rewind -- copies (src/ptm_mgau.c:425-437): the final order of the last
     * odd-numbered frame of the last utterance that has two frames (in a chain; of the last
     * utterance otherwise), else what that utterance itself started from */
    long long row = (long long)n_frames - 1;
    bool from_start = false; /* no frame wrote the slot: carry_in / the reset order */
    if (R.flags & SSW_SCORE_CARRY_OUT_REWIND) {
        row = -1;
        for (int u = n_utts - 1; u >= 0 && row < 0; --u) {
            const int T = utt_off[u + 1] - utt_off[u];
            if (T >= 2)
                row = (long long)utt_off[u] + (T / 2) * 2 - 1;
            else if (!C.chain) { /* utterances are independent: only the last one counts */
                from_start = true;
                for (int i = 0; i < m->n_cbf; ++i)
                    carry_out[i] = (u == 0 && carry_in != NULL) ? carry_in[i] : SSW_ORDER_RESET;
                break;
            }
        }
        if (row < 0 && !from_start) {
            from_start = true;
            for (int i = 0; i < m->n_cbf; ++i)
                carry_out[i] = carry_in != NULL ? carry_in[i] : SSW_ORDER_RESET;
        }
    }
    if (from_start)
        return 0;
    HIP_OK(hipMemcpyAsync(carry_out, C.cw + (size_t)row * m->n_cbf,
                          sizeof(uint32_t) * (size_t)m->n_cbf, hipMemcpyDeviceToHost, C.st));
    HIP_OK(hipStreamSynchronize(C.st));
    return 0;
}

/* The PTM and ms scorers: a top-N scan (the chain kernel, or the matrix-core or vector-unit scan)
 * and the senone kernel, as one launch pair or in pieces, with the timing events around them.
 * P: the batch as fill_chain_params and score_batch_impl describe it. */
static int
score_ptm_ms(const ScoreCall &C, const ChainParams &P)
{
    ssw_model_s *m = C.m;
    const ssw_host_model_t *h = m->h;
    const ScoreReq &R = C.R;
    const Knobs &kn = m->kn;
    const int n_frames = R.n_frames;
    const bool exact = !C.ms && (h->cfg.ds != 1 || m->force_exact);
    bool pieced = false;
    if (exact) {
        HIP_OK(launch_scan_chain(C, P));
    } else {
        FramesParams F;
        fill_frames_params(C, F);
        /* large batches of either scorer: the scan's multiply-adds go to the matrix cores (one
         * wave = 64 frames of one codebook x stream; SSW_SCAN=fma keeps the vector-unit scan) */
        /* (SSW_MFMA_MIN_FRAMES: tuning -- the smallest batch that takes the matrix-core scan;
         * d_wfrag is NULL on a device that failed the load-time self-test, ssw_host_model.inc) */
        const bool mfma = m->d_wfrag != NULL && h->n_feat * 13 == h->veclen_total
            && n_frames >= kn.mfma_min_frames && !kn.scan_fma;
        /* (SSW_SCORE_PIECE = 0: never cut) */
        pieced = mfma && kn.score_piece > 0 && n_frames >= 2 * kn.score_piece;
        if (pieced) {
            if (score_pieces(C, F, kn.score_piece) < 0)
                return -1;
        } else if (mfma)
            HIP_OK(launch_scan_mfma(C, F, 0, n_frames));
        else
            HIP_OK(launch_scan_frames(C, F));
    }
    if (m->sw.timing && !pieced)
        HIP_OK(hipEventRecord(m->sw.ev[1], C.st));
    if (!pieced) { /* (else scan and senone launches of every piece are on the stream) */
        if (R.act != NULL && R.cp != NULL) {
            ssw_set_error("internal error: compact rows with an active set");
            return -1;
        }
        if (launch_senone_or_active(C, 0, n_frames, !exact) < 0)
            return -1;
    }
    if (m->sw.timing && pieced) /* scan and senone launches alternate: no split, ms[0] = the call */
        HIP_OK(hipEventRecord(m->sw.ev[1], C.st));
    if (m->sw.timing) {
        HIP_OK(hipEventRecord(m->sw.ev[2], C.st));
        m->sw.timing_pieced = pieced ? 1 : 0;
    }
    if (score_timeline_dump(C.st) < 0)
        return -1;
    return score_batch_finish(C, exact ? (int64_t)n_frames * m->n_cbf : -1, !C.ms, true);
}

/* Every scoring entry point ends here: check, pick the scorer family, call its steps, finish. */
static int
score_batch_impl(ssw_model_t *m, const ScoreReq &R)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    refresh_knobs(m); /* tests: knobs flipped between calls on one model */
    if (R.carry_out != NULL && (R.n_frames == 0 || R.n_utts == 0)) { /* nothing scored: state unchanged */
        for (int i = 0; i < m->n_cbf; ++i)
            R.carry_out[i] = R.carry_in ? R.carry_in[i] : SSW_ORDER_RESET;
    }
    if (R.n_frames == 0 || R.n_utts == 0)
        return 0;
    if (score_check_batch(R.utt_off, R.n_utts, R.n_frames, "bad utterance offsets") < 0
        || check_scorer_shape(m, R.scorer) < 0)
        return -1;
    if (R.act != NULL && (m->h->cfg.ds != 1 || m->force_exact)) { /* (before anything is launched) */
        ssw_set_error("active-set batches: ds = 1 only");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    const bool ms = R.scorer == SSW_SCORER_MS;
    ScoreCall C{ m, R, (hipStream_t)R.stream, ms, (R.flags & SSW_SCORE_CARRY_UTTS) != 0 && !ms, NULL, NULL };
    if (m->h->continuous) {
        /* no history, no utterance boundaries, none of the PTM scan's workspaces: its own two
         * kernels (ssw_host_cont.inc); flags, carry_in and ds are ignored as for ms */
        if (R.cp != NULL || (R.act != NULL && (R.act->a2 != NULL || R.act->ls == NULL))) {
            ssw_set_error("internal error: segment lists or compact rows with a continuous model");
            return -1;
        }
        if (R.act != NULL && cont_refuse_active(m, "active-set scoring") < 0)
            return -1;
        if (m->sw.timing) {
            HIP_OK(hipEventRecord(m->sw.ev[0], C.st));
            m->sw.timing_semi = 0;
        }
        if (R.act != NULL) { /* compallsen = no: the listed senones of every frame alone */
            const SenoneListedParams &ls = *R.act->ls;
            ContListedReq Q{ R.d_feats, R.n_frames, ls.listed, R.act->row_of_frame, ls.out, ls.yes,
                             ls.cap,    ls.full };
            if (cont_listed_launch(m, Q, C.st) < 0)
                return -1;
            return score_batch_finish(C, 0, false, false);
        }
        if (cont_launch(m, R.d_feats, R.n_frames, R.d_out, C.st) < 0)
            return -1;
        /* (no top-N block: ssw_score_batch_topn has nothing to show) */
        return score_batch_finish(C, 0, false, false);
    }
    if (ensure_score_ws(m, (size_t)R.topn_row0 + (size_t)R.n_frames, R.n_utts) < 0)
        return -1;
    C.cw = m->sw.cw() + (size_t)R.topn_row0 * m->n_cbf;
    C.sc = m->sw.sc() + (size_t)R.topn_row0 * m->n_cbf;
    /* a caller that moves from one stream to another: the uploads below are only ordered behind
     * the launches of THIS stream */
    if (m->sw.have_last_stream && m->sw.last_stream != C.st)
        HIP_OK(hipDeviceSynchronize()); /* (not the old stream itself: it may be gone) */
    m->sw.last_stream = C.st;
    m->sw.have_last_stream = 1;
    const bool want_carry = R.carry_in != NULL && !ms;
    if (want_carry && score_check_carry(C) < 0)
        return -1;
    if (score_upload_meta(C, want_carry) < 0)
        return -1;
    ChainParams P;
    fill_chain_params(m, P, R.d_feats);
    P.topn_cw = C.cw;
    P.topn_sc = C.sc;
    P.n_utts = R.n_utts;
    P.n_frames = R.n_frames;
    P.chain_utts = C.chain ? 1 : 0;
    P.frame_base = R.frame_base;
    P.carry_pk = want_carry ? m->carry0.as<uint32_t>() : NULL;
    if (R.d_carry_rows != NULL && !ms) /* a row per utterance, already on the device */
        P.carry_pk = R.d_carry_rows;
    if (m->sw.timing) {
        HIP_OK(hipEventRecord(m->sw.ev[0], C.st));
        m->sw.timing_semi = R.scorer == SSW_SCORER_S2_SEMI;
    }
    if (R.scorer != SSW_SCORER_S2_SEMI)
        return score_ptm_ms(C, P);
    /* the same batch, history and carry semantics; its own three kernels (ssw_host_semi.inc) */
    if (R.act != NULL || R.cp != NULL) {
        ssw_set_error("internal error: active sets or compact rows with the s2_semi scorer");
        return -1;
    }
    if (semi_launch(m, P, R.d_out, C.st) < 0)
        return -1;
    return score_batch_finish(C, 0, true, true);
}

extern "C" int
ssw_score_batch(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream)
{
    return ssw_score_batch_ex(m, scorer, d_feats, n_frames, utt_off, n_utts, d_out, stream, 0u, NULL,
                              NULL);
}

extern "C" int
ssw_score_batch_ex(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                   const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream,
                   uint32_t flags, const uint32_t *carry_in, uint32_t *carry_out)
{
    ScoreReq R{};
    R.scorer = scorer;
    R.d_feats = d_feats;
    R.n_frames = n_frames;
    R.utt_off = utt_off;
    R.n_utts = n_utts;
    R.d_out = d_out;
    R.stream = stream;
    R.flags = flags;
    R.carry_in = carry_in;
    R.carry_out = carry_out;
    return score_batch_impl(m, R);
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
        if (ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, d_out, stream) < 0)
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
    if (feats == NULL || out == NULL || n_utts <= 0) {
        ssw_set_error("ssw_score_batch_host: bad arguments");
        return -1;
    }
    if (score_check_batch(utt_off, n_utts, n_frames, "ssw_score_batch_host: bad arguments") < 0)
        return -1;
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
     * the last call): every sub-batch scores into its own stretch of it (ScoreReq::topn_row0),
     * reserved here, so that no sub-batch grows it */
    if (!h->continuous && ensure_score_ws(m, (size_t)n_frames, n_utts) < 0)
        return -1;
    struct Restore {
        ssw_model_s *m;
        int total;
        ~Restore()
        {
            m->sw.last_n_frames = total;
            m->sw.stats_accumulate = 0; /* (also on the early returns: the next call counts afresh) */
        }
    } restore_{ m, n_frames };
    int64_t sum_flagged = 0, sum_pairs = 0; /* ssw_score_batch_stats speaks of the whole call */
    m->sw.stats_accumulate = 0;
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
            ScoreReq R{};
            R.scorer = scorer;
            R.d_feats = m->d_pipe_feat[slot];
            R.n_frames = nf;
            R.utt_off = off.data();
            R.n_utts = u1 - u0;
            R.d_out = m->d_pipe_out[slot];
            R.stream = m->s_pipe;
            /* (carry_out makes the piece's call synchronous: a long utterance's pieces do not
             * overlap their scoring with the copies -- they are 16 K frames each) */
            R.carry_in = S.cont ? carry.data() : NULL;
            R.carry_out = S.more ? carry.data() : NULL;
            /* a continuing piece keeps its utterance's frame numbers (the ds phase); grouped
             * utterances start at 0 */
            R.frame_base = S.cont ? f0 - utt_off[u0] : 0;
            R.topn_row0 = f0;
            if (score_batch_impl(m, R) < 0)
                return -1;
            sum_pairs += m->sw.stats[1];
            sum_flagged += m->sw.stats_pending ? 0 : m->sw.stats[0]; /* (the chain kernel: counted on the host) */
            m->sw.stats_accumulate = 1; /* the next sub-batch's count joins this one's on the device */
            HIP_OK(hipEventRecord(m->ev_piece[slot], m->s_pipe));
            HIP_OK(hipStreamWaitEvent(m->s_copy, m->ev_piece[slot], 0));
            HIP_OK(hipMemcpyAsync(m->h_pipe_out[slot], m->d_pipe_out[slot], (size_t)nf * row_out,
                                  hipMemcpyDeviceToHost, m->s_copy));
        }
        HIP_OK(hipEventRecord(m->ev_down[slot], m->s_copy));
        if (k > 0 && land(k - 1) < 0)
            return -1;
    }
    m->sw.stats_accumulate = 0;
    if (land(n_sub - 1) < 0)
        return -1;
    HIP_OK(hipStreamSynchronize(m->s_pipe));
    m->sw.stats[1] = sum_pairs;
    if (!m->sw.stats_pending)
        m->sw.stats[0] = sum_flagged;
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
    if (n_frames > m->sw.last_n_frames) {
        ssw_set_error("only %d frames were scored", m->sw.last_n_frames);
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(cw, m->sw.cw(), (size_t)n_frames * m->n_cbf * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(score, m->sw.sc(), (size_t)n_frames * m->n_cbf * 16,
                     hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int
ssw_set_kernel_timing(ssw_model_t *m, int enable)
{
    HIP_OK(hipSetDevice(m->device));
    if (enable && !m->sw.timing) {
        for (int i = 0; i < 3; ++i)
            HIP_OK(hipEventCreate(&m->sw.ev[i]));
        HIP_OK(hipEventCreate(&m->sw.ev_sc));
        m->sw.timing = 1;
    } else if (!enable && m->sw.timing) {
        for (int i = 0; i < 3; ++i)
            (void)hipEventDestroy(m->sw.ev[i]);
        (void)hipEventDestroy(m->sw.ev_sc);
        m->sw.timing = 0;
    }
    return 0;
}

extern "C" int
ssw_get_kernel_timing(ssw_model_t *m, float *ms, int n)
{
    if (!m->sw.timing) {
        ssw_set_error("kernel timing is off");
        return -1;
    }
    HIP_OK(hipEventSynchronize(m->sw.ev[2]));
    if (m->sw.timing_pieced) { /* one number: the whole call (scan and senone launches alternate) */
        if (n >= 1)
            HIP_OK(hipEventElapsedTime(&ms[0], m->sw.ev[0], m->sw.ev[2]));
        if (n >= 2)
            ms[1] = 0.0f;
        return n >= 1 ? 1 : 0;
    }
    int k = 0;
    for (; k < 2 && k < n; ++k)
        HIP_OK(hipEventElapsedTime(&ms[k], m->sw.ev[k], m->sw.ev[k + 1]));
    if (m->sw.timing_semi && n >= 3) { /* the s2_semi scorer: the chain kernel's share of ms[0] */
        HIP_OK(hipEventElapsedTime(&ms[2], m->sw.ev_sc, m->sw.ev[1]));
        k = 3;
    }
    return k;
}

extern "C" int
ssw_score_batch_stats(ssw_model_t *m, int64_t stats[2])
{
    if (m->sw.stats_pending) {
        unsigned long long n = 0;
        HIP_OK(hipSetDevice(m->device));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(&n, m->sw.d_nfixed + 1, sizeof(n), hipMemcpyDeviceToHost));
        m->sw.stats[0] = (int64_t)n; /* moved there by the last batch's senone kernel */
        m->sw.stats_pending = 0;
    }
    stats[0] = m->sw.stats[0];
    stats[1] = m->sw.stats[1];
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
    if (m->device == SSW_DEVICE_NONE || m->sw.d_nfixed == NULL)
        return 0;
    unsigned long long n[2] = { 0, 0 };
    HIP_OK(hipSetDevice(m->device));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(n, m->sw.d_nfixed + 2, sizeof(n), hipMemcpyDeviceToHost));
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
