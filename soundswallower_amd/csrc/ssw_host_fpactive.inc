/* ssw_host_fpactive.inc -- host: the first pass (and decoder_alignment) in the reference's DEFAULT
 * configuration, compallsen = no, for a batch: ssw_first_pass_batch_active,
 * ssw_align_text_batch_active.  Kernels and the argument why this is exact: ssw_k7_fpactive.inc.
 * One call of the loop is an FpaReq (ssw_host_firstpass.inc) through fpa_run's steps; its sizes
 * and the policy of its rounds are ssw_fpa_shape.inc's.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */

/* What the loop of speculation and proof (fpa_run) needs of the search it drives.  Two kinds:
 * the first pass of forced alignment, one phone-tree graph per utterance (first_pass_kernel
 * <.., EXPORT> and the long-text kernels), and recognition against a grammar plan, where the
 * HMMs are those of grammar fsg_of_utt[u] and many utterances share them (grammar_search_kernel
 * <.., EXPORT>, ssw_host_grammar.inc).  Everything else -- plan, scoring, comparison, rounds --
 * is the same. */
struct fpa_graph_t {
    const char *who;              /* the entry point, for messages */
    int n_nodes;                  /* rows of senid */
    const uint16_t *senid;        /* host [n_nodes][4] */
    std::vector<int> node_base;   /* [n_utts]: the utterance's first row of senid */
    std::vector<int> node_cnt;    /* [n_utts]: its phone-tree HMMs */
    int max_nodes;                /* at least the largest node_cnt: what the per-frame kernels'
                                     LDS is sized and checked for (a plan's largest grammar) */
    /* one run of the search over `rows`, the sets of active HMMs exported to `mask` (cleared
     * here where the kernel does not write every word); `only`: empty, or the utterances to
     * search; d_node_cnt: node_cnt on the device */
    int (*search)(void *arg, const int16_t *rows, const std::vector<int> &only,
                  unsigned long long *mask, const long long *d_act_off, const int *d_node_cnt);
    void *arg;
};

/* the first pass's: first_pass_run with an FpExport; `only` as it takes it */
struct fpa_fp_search_t {
    ssw_model_t *m;
    ssw_fp_graphs_t *g;
    const int32_t *utt_off;
    int32_t n_utts, max_seg;
    int32_t *n_seg;
    ssw_word_seg_t *seg;
    void *stream;
};

static int
fpa_fp_search(void *arg, const int16_t *rows, const std::vector<int> &only,
              unsigned long long *mask, const long long *d_act_off, const int *d_node_cnt)
{
    const fpa_fp_search_t &a = *static_cast<const fpa_fp_search_t *>(arg);
    FpReq R{};
    R.g = a.g;
    R.d_senscr = rows;
    R.utt_off = a.utt_off;
    R.n_utts = a.n_utts;
    R.max_seg = a.max_seg;
    R.n_seg = a.n_seg;
    R.seg = a.seg;
    R.stream = a.stream;
    R.t0 = now_ms();
    R.subset = &only;
    R.exp = FpExport{ mask, d_act_off, d_node_cnt };
    /* (through the levels of the long-text kernels, as ssw_first_pass_batch goes) */
    return first_pass_run(a.m, R);
}

/* what the loop serves: refused with a message before anything is uploaded or launched.  Every
 * path to fpa_run asks once: the grammar entries ahead of their run's begin, the first pass's in
 * first_pass_active_run. */
static int
fpa_check_limits(ssw_model_t *m, const char *who, int scorer)
{
    const ssw_host_model_t *h = m->h;
    if (check_scorer_shape(m, scorer) < 0)
        return -1;
    /* (the bound on the codebooks is the PTM codebook mask's: a continuous model has none) */
    if ((h->n_cb > 64 && !h->continuous) || h->n_emit_state != 3) {
        ssw_set_error("%s: built for <= 64 codebooks and 3-state HMMs", who);
        return -1;
    }
    if (scorer == SSW_SCORER_PTM && (h->cfg.ds != 1 || m->force_exact)) {
        ssw_set_error("%s: frame down-sampling (ds != 1) is served by "
                      "the per-frame calls only", who);
        return -1;
    }
    return 0;
}

/* one call's state: its shape, the workspace's tables (named once, in fpa_layout_upload) and
 * the rounds' bookkeeping */
struct FpaState {
    FpaShape S;
    unsigned long long *mask_x, *mask_y; /* the sets assumed, the sets the search then took */
    const long long *d_act_off;
    const int *d_utt_off, *d_node_base, *d_node_cnt;
    const uint16_t *d_senid;
    uint32_t *d_listed;
    unsigned long long *d_cbm;
    int32_t *d_iota;
    uint32_t *d_seed;
    int32_t *d_diff, *d_only;
    int16_t *d_yes;    /* one utterance's compallsen = yes rows (the rounds over few utterances) */
    uint32_t *d_start; /* two-pass history: the whole batch's utterance-start bits */
    std::vector<int> only; /* empty = every utterance */
    std::vector<int32_t> rounds, diff;
    int n_round;
};

static FpaModelSizes
fpa_model_sizes(const ssw_model_t *m, int scorer)
{
    const ssw_host_model_t *h = m->h;
    FpaModelSizes M;
    M.kind = h->continuous ? FPA_CONT : scorer == SSW_SCORER_MS ? FPA_MS : FPA_PTM;
    M.n_sen = h->n_sen;
    M.n_cbf = m->n_cbf;
    M.featdim = h->veclen_total;
    return M;
}

/* step 2: the workspace laid out, reserved, its tables uploaded in one copy (act_off | utt_off |
 * node base, count | senid) and every pointer of T resolved */
static int
fpa_layout_upload(ssw_model_t *m, const fpa_graph_t &G, const FpaReq &R, FpaState &T)
{
    const FpaShape &S = T.S;
    const size_t nf = (size_t)std::max(R.n_frames, 1), nU = (size_t)R.n_utts, nw32 = (size_t)S.nw32;
    const size_t mask_bytes = sizeof(unsigned long long) * (size_t)std::max(S.mask_words, 1ll);
    WsLayout L;
    L.out(&T.mask_x, mask_bytes);
    L.out(&T.mask_y, mask_bytes);
    const size_t o_up = L.mark();
    L.in(&T.d_act_off, S.act_off.data(), sizeof(long long) * nU);
    L.in(&T.d_utt_off, R.utt_off, sizeof(int) * (nU + 1));
    L.in(&T.d_node_base, G.node_base.data(), sizeof(int) * nU);
    L.in(&T.d_node_cnt, G.node_cnt.data(), sizeof(int) * nU);
    L.in(&T.d_senid, G.senid, sizeof(uint16_t) * 4 * (size_t)G.n_nodes, 1);
    L.out(&T.d_listed, sizeof(uint32_t) * nf * nw32);
    L.out(&T.d_cbm, sizeof(unsigned long long) * nf);
    L.out(&T.d_iota, sizeof(int32_t) * nf);
    L.out(&T.d_seed, sizeof(uint32_t) * nU * nw32);
    L.out(&T.d_diff, sizeof(int32_t) * nU);
    L.out(&T.d_only, sizeof(int32_t) * nU);
    L.out(&T.d_yes, sizeof(int16_t) * (size_t)std::max(S.max_len, 1) * (size_t)m->h->n_sen);
    L.out(&T.d_start, S.start_bytes);
    if (devbuf_reserve(m->fpa_ws, L.size(), G.who) < 0)
        return -1;
    L.resolve(m->fpa_ws.p);
    return stage_upload(m, m->fpa_ws.p + o_up, L.in_bytes() - o_up, (hipStream_t)R.stream,
                        [&](unsigned char *hs) { L.fill(hs, o_up); });
}

/* step 3, the assumption: the trajectory of the search over the compallsen = yes scores, its
 * sets into mask_x */
static int
fpa_assume(ssw_model_t *m, const fpa_graph_t &G, const FpaReq &R, FpaState &T)
{
    HIP_OK(hipMemsetAsync(T.d_seed, 0, sizeof(uint32_t) * (size_t)R.n_utts * (size_t)T.S.nw32,
                          (hipStream_t)R.stream));
    if (R.n_frames > 0
        && ssw_score_batch(m, R.scorer, R.d_feats, R.n_frames, R.utt_off, R.n_utts, R.d_rows, R.stream) < 0)
        return -1;
    return G.search(G.arg, R.d_rows, T.only, T.mask_x, T.d_act_off, T.d_node_cnt);
}

/* frames [lo, hi) = utterances [u_lo, u_hi), planned from mask_x (the sets assumed -> listed
 * senones and active codebooks per frame) and scored into d_rows (the scores the reference would
 * compute for them).  full: senone_listed_kernel's. */
static int
fpa_plan_and_score(ssw_model_t *m, const FpaReq &R, FpaState &T, int lo, int hi, int u_lo, int u_hi,
                   int full)
{
    const ssw_host_model_t *h = m->h;
    hipStream_t st = (hipStream_t)R.stream;
    if (hi <= lo)
        return 0;
    FpaPlanParams Q;
    Q.act_mask = T.mask_x;
    Q.act_off = T.d_act_off;
    Q.utt_off = T.d_utt_off;
    Q.node_base = T.d_node_base;
    Q.node_cnt = T.d_node_cnt;
    Q.senid = T.d_senid;
    Q.sen2cb = m->d_sen2cb;
    Q.listed = T.d_listed;
    Q.cbmask = T.d_cbm;
    Q.iota = T.d_iota;
    Q.seed = T.d_seed;
    Q.n_listed = NULL;
    Q.n_utts = R.n_utts;
    Q.n_frames = R.n_frames;
    Q.n_sen = h->n_sen;
    Q.nw32 = T.S.nw32;
    Q.frame_lo = lo;
    Q.frame_hi = hi;
    if (T.S.plan_lds > 48 * 1024)
        HIP_OK(hipFuncSetAttribute((const void *)fpa_plan_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)T.S.plan_lds));
    hipLaunchKernelGGL(fpa_plan_kernel, dim3((unsigned)((hi - lo + 3) / 4)), dim3(256), T.S.plan_lds,
                       st, Q, T.S.cap);
    HIP_OK(hipGetLastError());
    SenoneListedParams L;
    memset(&L, 0, sizeof(L));
    L.listed = T.d_listed + (size_t)lo * T.S.nw32;
    L.cbmask = T.d_cbm + lo;
    L.out = R.d_rows + (size_t)lo * h->n_sen;
    L.full = full;
    L.yes = T.d_yes; /* (full == 2: one utterance, its yes rows from frame 0) */
    L.cap = T.S.cap;
    ActiveSets act;
    /* (0 .. : the identity, whatever the sub-batch.  iota must hold 0 .. n for any sub-batch: the
     * whole batch's plan writes iota[t] = t once; a sub-batch's plan writes the same values at
     * the same places) */
    act.seg_of_frame = T.d_iota;
    act.seg_cbmask = T.d_cbm + lo;
    act.a2 = NULL;
    act.ls = &L;
    act.row_of_frame = NULL;
    std::vector<int32_t> sub;
    const int32_t *uo = R.utt_off;
    if (lo != 0 || hi != R.n_frames) {
        for (int u = u_lo; u <= u_hi; ++u)
            sub.push_back(R.utt_off[u] - lo);
        uo = sub.data();
    }
    ScoreReq Sc{};
    Sc.scorer = R.scorer;
    Sc.d_feats = R.d_feats + (size_t)lo * h->veclen_total;
    Sc.n_frames = hi - lo;
    Sc.utt_off = uo;
    Sc.n_utts = u_hi - u_lo;
    Sc.d_out = R.d_rows;
    Sc.stream = R.stream;
    Sc.act = &act;
    return score_batch_impl(m, Sc);
}

/* a round's plan and scoring (steps 2 + 3 of ssw_k7_fpactive.inc).  Few unproven utterances left
 * (fpa_one_by_one): they are scored one by one; else the whole batch again (the proven ones' rows
 * come out as they are: their sets have not changed) */
static int
fpa_score_round(ssw_model_t *m, const FpaReq &R, FpaState &T)
{
    if (!fpa_one_by_one(T.only.size(), R.n_utts, m->kn.fpa_sub))
        return fpa_plan_and_score(m, R, T, 0, R.n_frames, 0, R.n_utts, 0);
    /* each of them with its unlisted entries refreshed from its compallsen = yes scores
     * (senone_listed_kernel, full == 2): what such an utterance still gets wrong is the
     * fate of HMMs that enter outside the assumed sets, judged on whatever the row held */
    for (int u : T.only) {
        const int a = R.utt_off[u], b = R.utt_off[u + 1];
        if (b <= a)
            continue;
        const int32_t uo[2] = { 0, b - a };
        if (ssw_score_batch(m, R.scorer, R.d_feats + (size_t)a * m->h->veclen_total, b - a, uo, 1,
                            T.d_yes, R.stream) < 0)
            return -1;
        if (fpa_plan_and_score(m, R, T, a, b, u, u + 1, 2) < 0)
            return -1;
    }
    return 0;
}

/* step 5 of a round: an utterance is proven where the sets the search took (mask_y) are the
 * assumed ones (mask_x).  The round's utterances get its number; `again`: the ones not yet
 * proven, ascending.  Ends in the round's synchronisation of the stream. */
static int
fpa_compare(ssw_model_t *m, const FpaReq &R, FpaState &T, std::vector<int> &again)
{
    hipStream_t st = (hipStream_t)R.stream;
    const std::vector<int> &only = T.only;
    const int n_cmp = only.empty() ? R.n_utts : (int)only.size();
    if (!only.empty()
        && stage_upload(m, T.d_only, sizeof(int32_t) * only.size(), st, [&](unsigned char *hs) {
               memcpy(hs, only.data(), sizeof(int32_t) * only.size());
           }) < 0)
        return -1;
    HIP_OK(hipMemsetAsync(T.d_diff, 0x7f, sizeof(int32_t) * (size_t)R.n_utts, st));
    hipLaunchKernelGGL(fpa_compare_kernel, dim3((unsigned)n_cmp, fpa_compare_slices(T.S.mask_words, n_cmp)),
                       dim3(256), 0, st, T.mask_x, T.mask_y, T.d_act_off, T.d_utt_off, T.d_node_cnt,
                       only.empty() ? (const int *)NULL : T.d_only, T.d_diff);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(T.diff.data(), T.d_diff, sizeof(int32_t) * (size_t)R.n_utts,
                          hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 0; i < n_cmp; ++i) {
        const int u = only.empty() ? i : only[(size_t)i];
        T.rounds[(size_t)u] = T.n_round;
        if (T.diff[(size_t)u] != FPA_NO_DIFF)
            again.push_back(u);
    }
    return 0;
}

/* step 6, two_pass_history: history slot 1 as every utterance's first pass leaves it
 * (fpa_carry_rows_kernel), from the features and the proven codebook masks -- d_cbm holds, for
 * every utterance, those of the last plan of its frames */
static int
fpa_carry_rows(ssw_model_t *m, const FpaReq &R, FpaState &T)
{
    const ssw_host_model_t *h = m->h;
    hipStream_t st = (hipStream_t)R.stream;
    if (R.d_carry_out == NULL || R.scorer != SSW_SCORER_PTM)
        return 0;
    if (m->d_rec28 == NULL) {
        ssw_set_error("two_pass_history in the default configuration needs codebooks of 128 densities");
        return -1;
    }
    if (R.n_frames <= 0)
        return 0;
    const size_t n_words = T.S.n_start_words;
    if (stage_upload(m, T.d_start, sizeof(uint32_t) * n_words, st, [&](unsigned char *hs) {
            uint32_t *bits = reinterpret_cast<uint32_t *>(hs);
            memset(bits, 0, sizeof(uint32_t) * n_words);
            for (int u = 0; u < R.n_utts; ++u)
                if (R.utt_off[u] < R.n_frames)
                    bits[(size_t)R.utt_off[u] >> 5] |= 1u << (R.utt_off[u] & 31);
        }) < 0)
        return -1;
    FramesParams F;
    memset(&F, 0, sizeof(F));
    F.utt_start = T.d_start;
    F.utt_off = T.d_utt_off;
    F.n_utts = R.n_utts;
    F.seg_of_frame = T.d_iota;
    F.seg_cbmask = T.d_cbm;
    F.n_frames = R.n_frames;
    F.n_cbf = m->n_cbf;
    F.n_feat = h->n_feat;
    F.featdim = h->veclen_total;
    for (int f = 0; f < h->n_feat; ++f)
        F.featoff[f] = h->featoff[f];
    hipLaunchKernelGGL(fpa_carry_rows_kernel, dim3((unsigned)((size_t)R.n_utts * m->n_cbf)), dim3(64), 0,
                       st, F, m->d_rec28, R.d_feats, T.d_utt_off, R.d_carry_out);
    HIP_OK(hipGetLastError());
    return 0;
}

/* step 7: what the caller asked for, on the host when this returns */
static int
fpa_copy_out(const FpaReq &R, const FpaState &T)
{
    hipStream_t st = (hipStream_t)R.stream;
    const size_t nw32 = (size_t)T.S.nw32;
    if (R.listed_out != NULL && R.n_frames > 0)
        HIP_OK(hipMemcpyAsync(R.listed_out, T.d_listed, sizeof(uint32_t) * (size_t)R.n_frames * nw32,
                              hipMemcpyDeviceToHost, st));
    if (R.seed_out != NULL)
        HIP_OK(hipMemcpyAsync(R.seed_out, T.d_seed, sizeof(uint32_t) * (size_t)R.n_utts * nw32,
                              hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (R.rounds_out != NULL)
        memcpy(R.rounds_out, T.rounds.data(), sizeof(int32_t) * (size_t)R.n_utts);
    return 0;
}

/* step 8: the counters of ssw_first_pass_active_stats / ssw_grammar_active_stats */
static void
fpa_add_stats(const FpaReq &R, const FpaState &T)
{
    int more = 0;
    long long sum = 0;
    for (int u = 0; u < R.n_utts; ++u) {
        sum += T.rounds[(size_t)u];
        more += T.rounds[(size_t)u] > 1 ? 1 : 0;
    }
    R.stats[0] += R.n_utts;
    R.stats[1] += sum;
    R.stats[2] = T.n_round;
    R.stats[3] += more;
}

/* The loop of speculation and proof for one request.  The caller holds the model (ModelBusy) and
 * has asked fpa_check_limits. */
static int
fpa_run(ssw_model_t *m, const fpa_graph_t &G, const FpaReq &R)
{
    hipStream_t st = (hipStream_t)R.stream;
    if (R.n_utts <= 0)
        return 0;
    HIP_OK(hipSetDevice(m->device));
    refresh_knobs(m);
    const bool timing = m->kn.align_timing;
    const double t_in = now_ms();
    FpaState T;
    /* 1: the shape */
    if (fpa_shape(G.who, fpa_model_sizes(m, R.scorer), G.node_cnt.data(), G.max_nodes, R.utt_off,
                  R.n_utts, R.n_frames, R.d_carry_out != NULL, T.S) < 0) {
        ssw_set_error("%s", T.S.err);
        return -1;
    }
    T.rounds.assign((size_t)R.n_utts, 0);
    T.diff.assign((size_t)R.n_utts, 0);
    T.n_round = 0;
    /* 2: layout and upload; 3: the assumption */
    if (fpa_layout_upload(m, G, R, T) < 0 || fpa_assume(m, G, R, T) < 0)
        return -1;
    const double t_spec = now_ms();
    /* 4: rounds until every utterance's sets are proven */
    for (;;) {
        ++T.n_round;
        const double r0 = now_ms();
        if (fpa_score_round(m, R, T) < 0)
            return -1;
        if (timing)
            HIP_OK(hipStreamSynchronize(st));
        const double r1 = now_ms();
        /* the search over those scores, its sets into mask_y */
        if (G.search(G.arg, R.d_rows, T.only, T.mask_y, T.d_act_off, T.d_node_cnt) < 0)
            return -1;
        const double r2 = now_ms();
        const int n_cmp = T.only.empty() ? R.n_utts : (int)T.only.size();
        std::vector<int> again;
        if (fpa_compare(m, R, T, again) < 0)
            return -1;
        if (timing)
            fprintf(stderr, "%s: round %d, %d searched, %zu not yet proven "
                            "(plan + scoring %.2f ms, search %.2f, comparison %.2f)\n",
                    G.who, T.n_round, n_cmp, again.size(), r1 - r0, r2 - r1, now_ms() - r2);
        if (again.empty())
            break;
        /* every round proves at least one more frame of each of them (the first differing
         * frame's set in mask_y is the reference's), so this ends; the cap is a guard against
         * a defect, not a budget */
        if (T.n_round > 4 * 16384) {
            ssw_set_error("%s: utterance %d not proven after %d rounds", G.who, again[0], T.n_round);
            return -1;
        }
        std::swap(T.mask_x, T.mask_y); /* (the proven utterances' sets are the same in both) */
        fpa_next_only(T.only, again, R.n_utts, m->kn.fpa_sub);
    }
    /* mask_x now holds every utterance's proven sets (for the ones of the last round mask_y is
     * equal to it), and every utterance's seed row was written by the last plan of its frames,
     * the one whose sets were then proven.
     * 5: on request the rows as acmod's buffer would hold them, from one more plan (+ scoring
     * with the unlisted entries written); 6: the carried orders; 7: the copies out; 8: stats */
    if (R.full_rows && fpa_plan_and_score(m, R, T, 0, R.n_frames, 0, R.n_utts, 1) < 0)
        return -1;
    if (fpa_carry_rows(m, R, T) < 0 || fpa_copy_out(R, T) < 0)
        return -1;
    fpa_add_stats(R, T);
    if (timing)
        fprintf(stderr, "%s: assumption (compallsen = yes scoring + search) "
                        "%.2f ms, %d round(s) %.2f ms\n", G.who, t_spec - t_in, T.n_round, now_ms() - t_spec);
    return 0;
}

/* the first pass's graphs: every utterance its own */
static int
first_pass_active_run(ssw_model_t *m, const FpaReq &R, ssw_fp_graphs_t *g, int32_t max_seg,
                      int32_t *n_seg, ssw_word_seg_t *seg)
{
    fpa_fp_search_t a = { m, g, R.utt_off, R.n_utts, max_seg, n_seg, seg, R.stream };
    fpa_graph_t G;
    G.who = "ssw_first_pass_batch_active";
    if (R.n_utts <= 0)
        return 0;
    if (fpa_check_limits(m, G.who, R.scorer) < 0)
        return -1;
    G.n_nodes = g->n_nodes;
    G.senid = g->senid;
    G.max_nodes = 0;
    for (int u = 0; u < R.n_utts; ++u) {
        G.node_base.push_back(g->node_off[u]);
        G.node_cnt.push_back(g->node_off[u + 1] - g->node_off[u]);
    }
    G.search = fpa_fp_search;
    G.arg = &a;
    return fpa_run(m, G, R);
}

/* The s2_semi scorer in the *_active calls.  s2_semi_mgau_frame_eval evaluates every Gaussian and
 * normalises per stream by its best density whatever the active set is (src/s2_semi_mgau.c:
 * 841-872): compallsen = no only restricts which senones are summed, and the search reads the
 * listed ones alone.  The default configuration's search therefore reads the very scores of the
 * compallsen = yes rows, and these calls take that route: one search, nothing to prove.  The
 * stats report one round per utterance and every first assumption accepted; the sets of listed
 * senones are not made (`sets`, the entry's seed_active or listed named sets_name, is refused),
 * d_senscr receives whole rows.  yes(): the entry's compallsen = yes call, 0 or -1. */
template <typename Yes>
static int
semi_active_route(const char *who, const void *sets, const char *sets_name, int64_t stats[4],
                  int32_t n_utts, int32_t *rounds, Yes yes)
{
    if (sets != NULL) {
        ssw_set_error("%s: the s2_semi scorer makes no sets of listed senones (%s)", who, sets_name);
        return -1;
    }
    if (yes() < 0)
        return -1;
    stats[0] += n_utts;
    stats[1] += n_utts;
    stats[2] = 1;
    for (int u = 0; rounds != NULL && u < n_utts; ++u)
        rounds[u] = 1;
    return 0;
}

/* the rows a call scores into: the caller's, or the model's own (ssw_align_text_batch's
 * workspace) after text_rows_reserve; NULL with the error set.  The device is current. */
static int16_t *
active_rows(ssw_model_t *m, int16_t *d_senscr, int32_t n_frames, const char *who)
{
    if (d_senscr != NULL)
        return d_senscr;
    if (text_rows_reserve(m, n_frames, who) < 0)
        return NULL;
    return m->text_scr.as<int16_t>();
}

extern "C" int
ssw_first_pass_batch_active(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                            int scorer, const float *d_feats, int32_t n_frames,
                            const int32_t *utt_off, int32_t n_utts, const int32_t *word_off,
                            const char *const *words, int32_t max_seg, int32_t *n_seg,
                            ssw_word_seg_t *seg, uint32_t *seed_active, int16_t *d_senscr,
                            int32_t *rounds, void *stream)
{
    const char *who = "ssw_first_pass_batch_active";
    if (n_utts == 0)
        return 0;
    if (check_has_device(m) < 0)
        return -1;
    if (n_utts < 0 || n_frames < 0 || max_seg < 1 || !utt_off || !word_off || !words || !n_seg
        || !seg || !d || !utt_off_spans(utt_off, n_utts, n_frames)
        || (n_frames > 0 && d_feats == NULL)) {
        ssw_set_error("bad arguments to ssw_first_pass_batch_active");
        return -1;
    }
    if (cont_refuse_active(m, who) < 0)
        return -1;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    HIP_OK(hipSetDevice(m->device));
    int16_t *rows = active_rows(m, d_senscr, n_frames, who);
    if (rows == NULL)
        return -1;
    if (scorer == SSW_SCORER_S2_SEMI)
        return semi_active_route(who, seed_active, "seed_active", m->fpa_stats, n_utts, rounds, [&] {
            if (n_frames > 0
                && ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, rows, stream) < 0)
                return -1;
            return ssw_first_pass_batch(m, d, cfg, rows, n_frames, utt_off, n_utts, word_off, words,
                                        max_seg, n_seg, seg, stream);
        });
    ssw_fp_graphs_t *g = ssw_fp_graphs_build(m, d, cfg, n_utts, word_off, words);
    if (g == NULL)
        return -1;
    FpaReq R{};
    R.scorer = scorer;
    R.d_feats = d_feats;
    R.n_frames = n_frames;
    R.utt_off = utt_off;
    R.n_utts = n_utts;
    R.d_rows = rows;
    R.full_rows = d_senscr != NULL;
    R.seed_out = seed_active;
    R.rounds_out = rounds;
    R.stats = m->fpa_stats;
    R.stream = stream;
    const int rc = first_pass_active_run(m, R, g, max_seg, n_seg, seg);
    ssw_fp_graphs_free(g);
    return rc;
}

/* [0] utterances searched by ssw_first_pass_batch_active / ssw_align_text_batch_active since the
 * model was loaded, [1] their verify rounds summed, [2] rounds of the last call, [3] utterances
 * whose first assumption (the compallsen = yes trajectory) was not the reference's */
extern "C" int
ssw_first_pass_active_stats(ssw_model_t *m, int64_t stats[4])
{
    for (int i = 0; i < 4; ++i)
        stats[i] = m->fpa_stats[i];
    return 0;
}

/* decoder_alignment in the default configuration for a batch, from features: the first pass
 * above, alignment_populate with its word windows, then the second pass as
 * ssw_align_batch_active_ex does it -- acmod's set starts from what the first pass's last frame
 * left and only grows (src/state_align_search.c:186-189) -- and alignment_propagate. */
extern "C" ssw_alignment_set_t *
ssw_align_text_batch_active(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                            int scorer, const float *d_feats, int32_t n_frames,
                            const int32_t *utt_off, int32_t n_utts, const int32_t *word_off,
                            const char *const *words, void *stream)
{
    const char *who = "ssw_align_text_batch_active";
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    if (check_has_device(m) < 0)
        return NULL;
    if (n_utts < 0 || n_frames < 0 || (n_frames > 0 && d_feats == NULL) || !utt_off || !word_off
        || !words || !d || !utt_off_spans(utt_off, n_utts, n_frames)) {
        ssw_set_error("bad arguments to ssw_align_text_batch_active");
        return NULL;
    }
    if (cont_refuse_active(m, who) < 0)
        return NULL;
    ssw_alignment_set_t *a = NULL;
    if (scorer == SSW_SCORER_S2_SEMI) {
        semi_active_route(who, NULL, NULL, m->fpa_stats, n_utts, NULL, [&] {
            a = ssw_align_text_batch(m, d, cfg, scorer, d_feats, n_frames, utt_off, n_utts, word_off,
                                     words, stream);
            return a != NULL ? 0 : -1;
        });
        return a;
    }
    if (hipSetDevice(m->device) != hipSuccess)
        return NULL;
    int16_t *rows = active_rows(m, NULL, n_frames, who);
    if (rows == NULL)
        return NULL;
    checked_texts_t c;
    check_texts(d, n_utts, word_off, words, c);
    ssw_first_pass_plan_t *plan = c.any
        ? ssw_first_pass_prepare(m, d, cfg, n_utts, c.word_off.data(), c.words.data())
        : ssw_first_pass_prepare(m, d, cfg, n_utts, word_off, words);
    if (plan == NULL)
        return NULL;
    fpa_mode_t mode = { scorer, d_feats, cfg != NULL && cfg->two_pass_history != 0 };
    ForcedAlignReq F{};
    F.d = d;
    F.plan = plan;
    F.d_senscr = rows;
    F.n_frames = n_frames;
    F.utt_off = utt_off;
    F.n_utts = plan->n_utts;
    F.stream = stream;
    F.reject = c.any ? &c.reject : NULL;
    F.fpa = &mode;
    a = forced_align_core(m, F);
    ssw_first_pass_plan_free(plan);
    return a;
}

/* Debug / parity view: the orders the last ssw_align_text_batch_active call with
 * two_pass_history handed from every utterance's first pass to its second -- host uint32
 * [n_utts][n_cb * n_feat], 4 codewords packed best first (history slot 1 of the reference's
 * ring after the first pass, src/ptm_mgau.c:425-437). */
extern "C" int
ssw_first_pass_active_carry(ssw_model_t *m, int32_t n_utts, uint32_t *rows)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const size_t n = (size_t)n_utts * (size_t)m->n_cbf;
    if (n_utts < 0 || rows == NULL || m->carry_rows.p == NULL || sizeof(uint32_t) * n > m->carry_rows.cap) {
        ssw_set_error("ssw_first_pass_active_carry: no carried orders of %d utterances", n_utts);
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    HIP_OK(hipMemcpy(rows, m->carry_rows.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}
