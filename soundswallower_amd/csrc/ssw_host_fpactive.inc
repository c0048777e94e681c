/* ssw_host_fpactive.inc -- host: the first pass (and decoder_alignment) in the reference's DEFAULT
 * configuration, compallsen = no, for a batch: ssw_first_pass_batch_active,
 * ssw_align_text_batch_active.  Kernels and the argument why this is exact: ssw_k7_fpactive.inc.
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

/* what the loop serves: refused with a message before anything is uploaded or launched */
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

/* d_rows: int16 [n_frames][n_sen] device rows the call scores into (workspace and, with
 * full_rows, output).  seed_out: NULL or host [n_utts][(n_sen + 31) / 32].  rounds_out: NULL or
 * host [n_utts]: searches of the utterance over default-configuration scores until its sets
 * were proven (1 = the assumed trajectory was already the right one).
 * listed_out: NULL or host [n_frames][(n_sen + 31) / 32]: the proven listed senones of every
 * frame, bridges included.  stats: the caller's four counters. */
static int
fpa_run(ssw_model_t *m, const fpa_graph_t &G, int scorer, const float *d_feats, int32_t n_frames,
        const int32_t *utt_off, int32_t n_utts, int16_t *d_rows, bool full_rows, uint32_t *seed_out,
        int32_t *rounds_out, uint32_t *listed_out, int64_t *stats, void *stream,
        uint32_t *d_carry_out)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const ssw_host_model_t *h = m->h;
    hipStream_t st = (hipStream_t)stream;
    if (n_utts <= 0)
        return 0;
    if (fpa_check_limits(m, G.who, scorer) < 0)
        return -1;
    HIP_OK(hipSetDevice(m->device));
    refresh_knobs(m);
    const bool timing = m->kn.align_timing;
    const double t_in = now_ms();
    const int nw32 = (h->n_sen + 31) / 32;
    /* the exported sets: [n_frames_u][ceil(N_u / 64)] 64-bit words per utterance */
    std::vector<long long> act_off((size_t)n_utts);
    long long mask_words = 0;
    int max_nodes = G.max_nodes;
    for (int u = 0; u < n_utts; ++u) {
        const int nn = G.node_cnt[(size_t)u];
        act_off[(size_t)u] = mask_words;
        mask_words += (long long)(utt_off[u + 1] - utt_off[u]) * ((nn + 63) / 64);
        max_nodes = std::max(max_nodes, nn);
    }
    /* a frame lists at most three senones per HMM plus the bridges between them */
    /* (even: the plan kernel's LDS words behind the list stay 4-byte aligned) */
    const int cap = ((int)std::min<long long>(h->n_sen, 3ll * max_nodes + h->n_sen / 255 + 2) + 1) & ~1;
    {
        /* what the two per-frame kernels keep in LDS per wave (four waves a workgroup) */
        const size_t plan_lds = 4 * ((4 * (size_t)nw32 + 2 * (size_t)cap + 8 + 15) & ~(size_t)15);
        const size_t sen_lds = h->continuous
            ? cont_listed_lds(m, cap)
            : 4 * (((scorer == SSW_SCORER_MS ? 0 : 8 * (size_t)m->n_cbf)
                    + 4 * (size_t)((cap + 1) & ~1) + 16 + 15) & ~(size_t)15);
        if (std::max(plan_lds, sen_lds) > 156 * 1024) {
            ssw_set_error("%s: %d senones x texts of up to %d phone-tree "
                          "HMMs need %zu KB of LDS per workgroup (160 KB a CU)", G.who, h->n_sen, max_nodes,
                          std::max(plan_lds, sen_lds) / 1024);
            return -1;
        }
    }
    const size_t nf = (size_t)std::max(n_frames, 1), nU = (size_t)n_utts;
    WsLayout L;
    const size_t o_ma = L.out(sizeof(unsigned long long) * (size_t)std::max(mask_words, 1ll));
    const size_t o_mb = L.out(sizeof(unsigned long long) * (size_t)std::max(mask_words, 1ll));
    const size_t o_up = L.mark(); /* uploaded in one copy: act_off | utt_off | node base, count | senid */
    const size_t o_ao = L.in(act_off.data(), sizeof(long long) * nU);
    const size_t o_uo = L.in(utt_off, sizeof(int) * (nU + 1));
    const size_t o_nb = L.in(G.node_base.data(), sizeof(int) * nU);
    const size_t o_nc = L.in(G.node_cnt.data(), sizeof(int) * nU);
    const size_t o_sid = L.in(G.senid, sizeof(uint16_t) * 4 * (size_t)G.n_nodes, 1);
    const size_t o_listed = L.out(sizeof(uint32_t) * nf * (size_t)nw32);
    const size_t o_cbm = L.out(sizeof(unsigned long long) * nf);
    const size_t o_iota = L.out(sizeof(int32_t) * nf);
    const size_t o_seed = L.out(sizeof(uint32_t) * nU * (size_t)nw32);
    const size_t o_diff = L.out(sizeof(int32_t) * nU);
    const size_t o_only = L.out(sizeof(int32_t) * nU);
    int max_len = 0;
    for (int u = 0; u < n_utts; ++u)
        max_len = std::max(max_len, utt_off[u + 1] - utt_off[u]);
    /* one utterance's compallsen = yes rows (the rounds over few utterances, below) */
    const size_t o_yes = L.out(sizeof(int16_t) * (size_t)std::max(max_len, 1) * (size_t)h->n_sen);
    /* (two-pass history: the whole batch's utterance-start bits, for fpa_carry_rows_kernel) */
    const size_t n_start_words = nf / 32 + 2;
    const size_t o_start = L.out(d_carry_out != NULL ? sizeof(uint32_t) * n_start_words : 0);
    if (devbuf_reserve(m->fpa_ws, L.size(), G.who) < 0)
        return -1;
    unsigned char *ws = m->fpa_ws.p;
    if (stage_upload(m, ws + o_up, L.in_bytes() - o_up, st,
                     [&](unsigned char *hs) { L.fill(hs, o_up); }) < 0)
        return -1;
    unsigned long long *mask_x = reinterpret_cast<unsigned long long *>(ws + o_ma);
    unsigned long long *mask_y = reinterpret_cast<unsigned long long *>(ws + o_mb);
    const long long *d_act_off = reinterpret_cast<const long long *>(ws + o_ao);
    const int *d_utt_off = reinterpret_cast<const int *>(ws + o_uo);
    const int *d_node_base = reinterpret_cast<const int *>(ws + o_nb);
    const int *d_node_cnt = reinterpret_cast<const int *>(ws + o_nc);
    uint32_t *d_listed = reinterpret_cast<uint32_t *>(ws + o_listed);
    unsigned long long *d_cbm = reinterpret_cast<unsigned long long *>(ws + o_cbm);
    int32_t *d_iota = reinterpret_cast<int32_t *>(ws + o_iota);
    uint32_t *d_seed = reinterpret_cast<uint32_t *>(ws + o_seed);
    int32_t *d_diff = reinterpret_cast<int32_t *>(ws + o_diff);
    int32_t *d_only = reinterpret_cast<int32_t *>(ws + o_only);
    int16_t *d_yes = reinterpret_cast<int16_t *>(ws + o_yes);

    HIP_OK(hipMemsetAsync(d_seed, 0, sizeof(uint32_t) * (size_t)n_utts * (size_t)nw32, st));
    /* 0: the assumption -- the trajectory of the search over the compallsen = yes scores */
    std::vector<int> only; /* empty = every utterance */
    if (n_frames > 0
        && ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, d_rows, stream) < 0)
        return -1;
    if (G.search(G.arg, d_rows, only, mask_x, d_act_off, d_node_cnt) < 0)
        return -1;
    const double t_spec = now_ms();
    std::vector<int32_t> rounds((size_t)n_utts, 0), diff((size_t)n_utts);
    auto plan_and_score = [&](int lo, int hi, int u_lo, int u_hi, int full) -> int {
        /* frames [lo, hi) = utterances [u_lo, u_hi), planned from mask_x and scored into d_rows */
        if (hi <= lo)
            return 0;
        FpaPlanParams Q;
        Q.act_mask = mask_x;
        Q.act_off = d_act_off;
        Q.utt_off = d_utt_off;
        Q.node_base = d_node_base;
        Q.node_cnt = d_node_cnt;
        Q.senid = reinterpret_cast<const uint16_t *>(ws + o_sid);
        Q.sen2cb = m->d_sen2cb;
        Q.listed = d_listed;
        Q.cbmask = d_cbm;
        Q.iota = d_iota;
        Q.seed = d_seed;
        Q.n_listed = NULL;
        Q.n_utts = n_utts;
        Q.n_frames = n_frames;
        Q.n_sen = h->n_sen;
        Q.nw32 = nw32;
        Q.frame_lo = lo;
        Q.frame_hi = hi;
        const size_t per_wave = (4 * (size_t)nw32 + 2 * (size_t)cap + 8 + 15) & ~(size_t)15;
        if (4 * per_wave > 48 * 1024)
            HIP_OK(hipFuncSetAttribute((const void *)fpa_plan_kernel,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * per_wave)));
        hipLaunchKernelGGL(fpa_plan_kernel, dim3((unsigned)((hi - lo + 3) / 4)), dim3(256),
                           4 * per_wave, st, Q, cap);
        HIP_OK(hipGetLastError());
        SenoneListedParams L;
        memset(&L, 0, sizeof(L));
        L.listed = d_listed + (size_t)lo * nw32;
        L.cbmask = d_cbm + lo;
        L.out = d_rows + (size_t)lo * h->n_sen;
        L.full = full;
        L.yes = d_yes; /* (full == 2: one utterance, its yes rows from frame 0) */
        L.cap = cap;
        ActiveSets act;
        act.seg_of_frame = d_iota; /* (0 .. : the identity, whatever the sub-batch) */
        act.seg_cbmask = d_cbm + lo;
        act.a2 = NULL;
        act.ls = &L;
        act.row_of_frame = NULL;
        std::vector<int32_t> sub;
        const int32_t *uo = utt_off;
        if (lo != 0 || hi != n_frames) {
            for (int u = u_lo; u <= u_hi; ++u)
                sub.push_back(utt_off[u] - lo);
            uo = sub.data();
        }
        ScoreReq R{};
        R.scorer = scorer;
        R.d_feats = d_feats + (size_t)lo * h->veclen_total;
        R.n_frames = hi - lo;
        R.utt_off = uo;
        R.n_utts = u_hi - u_lo;
        R.d_out = d_rows;
        R.stream = stream;
        R.act = &act;
        return score_batch_impl(m, R);
    };
    /* (iota must hold 0 .. n for any sub-batch: the whole batch's plan writes iota[t] = t once;
     * a sub-batch's plan writes the same values at the same places) */
    int n_round = 0;
    for (;;) {
        ++n_round;
        const double r0 = now_ms();
        /* 2 + 3: the sets assumed (mask_x) -> listed senones and active codebooks per frame ->
         * the scores the reference would compute for them.  Few unproven utterances left: they
         * are scored one by one; else the whole batch again (the proven ones' rows come out as
         * they are: their sets have not changed) */
        /* (at most four, or a quarter of the batch: a batch of one long utterance is "few") */
        const bool one_by_one = !only.empty()
            && (m->kn.fpa_sub == 1
                || (m->kn.fpa_sub != 0 && (int)only.size() <= std::max(4, n_utts / 4)));
        if (!one_by_one) {
            if (plan_and_score(0, n_frames, 0, n_utts, 0) < 0)
                return -1;
        } else {
            /* each of them with its unlisted entries refreshed from its compallsen = yes scores
             * (senone_listed_kernel, full == 2): what such an utterance still gets wrong is the
             * fate of HMMs that enter outside the assumed sets, judged on whatever the row held */
            for (int u : only) {
                const int a = utt_off[u], b = utt_off[u + 1];
                if (b <= a)
                    continue;
                const int32_t uo[2] = { 0, b - a };
                if (ssw_score_batch(m, scorer, d_feats + (size_t)a * h->veclen_total, b - a, uo, 1,
                                    d_yes, stream) < 0)
                    return -1;
                if (plan_and_score(a, b, u, u + 1, 2) < 0)
                    return -1;
            }
        }
        if (timing)
            HIP_OK(hipStreamSynchronize(st));
        const double r1 = now_ms();
        /* 4: the search over those scores, its sets into mask_y */
        if (G.search(G.arg, d_rows, only, mask_y, d_act_off, d_node_cnt) < 0)
            return -1;
        const double r2 = now_ms();
        /* 5: proven where the sets are the assumed ones */
        const int n_cmp = only.empty() ? n_utts : (int)only.size();
        if (!only.empty()
            && stage_upload(m, d_only, sizeof(int32_t) * only.size(), st, [&](unsigned char *hs) {
                   memcpy(hs, only.data(), sizeof(int32_t) * only.size());
               }) < 0)
            return -1;
        HIP_OK(hipMemsetAsync(d_diff, 0x7f, sizeof(int32_t) * (size_t)n_utts, st));
        /* (slices: enough workgroups for a single long utterance, few for a batch of short ones) */
        const unsigned slices = (unsigned)std::min<long long>(
            64, std::max<long long>(1, mask_words / std::max(1, n_cmp) / (256 * 16)));
        hipLaunchKernelGGL(fpa_compare_kernel, dim3((unsigned)n_cmp, slices), dim3(256), 0, st, mask_x, mask_y,
                           d_act_off, d_utt_off, d_node_cnt, only.empty() ? (const int *)NULL : d_only,
                           d_diff);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(diff.data(), d_diff, sizeof(int32_t) * (size_t)n_utts,
                              hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        std::vector<int> again;
        if (only.empty()) {
            for (int u = 0; u < n_utts; ++u) {
                rounds[(size_t)u] = n_round;
                if (diff[(size_t)u] != FPA_NO_DIFF)
                    again.push_back(u);
            }
        } else {
            for (int u : only) {
                rounds[(size_t)u] = n_round;
                if (diff[(size_t)u] != FPA_NO_DIFF)
                    again.push_back(u);
            }
        }
        if (timing)
            fprintf(stderr, "%s: round %d, %d searched, %zu not yet proven "
                            "(plan + scoring %.2f ms, search %.2f, comparison %.2f)\n",
                    G.who, n_round, n_cmp, again.size(), r1 - r0, r2 - r1, now_ms() - r2);
        if (again.empty())
            break;
        /* every round proves at least one more frame of each of them (the first differing
         * frame's set in mask_y is the reference's), so this ends; the cap is a guard against
         * a defect, not a budget */
        if (n_round > 4 * 16384) {
            ssw_set_error("%s: utterance %d not proven after %d rounds", G.who, again[0],
                          n_round);
            return -1;
        }
        std::swap(mask_x, mask_y); /* (the proven utterances' sets are the same in both) */
        only.swap(again);
        if ((int)only.size() == n_utts && n_utts > 4 && m->kn.fpa_sub != 1)
            only.clear(); /* every one of them: the whole batch as a whole */
    }
    /* mask_x now holds every utterance's proven sets (for the ones of the last round mask_y is
     * equal to it).  The seed of the second pass and, on request, the rows as acmod's buffer
     * would hold them come from one more plan (+ scoring with the unlisted entries written) */
    /* (every utterance's seed row was written by the last plan of its frames, the one whose sets
     * were then proven) */
    if (full_rows && plan_and_score(0, n_frames, 0, n_utts, 1) < 0)
        return -1;
    if (d_carry_out != NULL && scorer == SSW_SCORER_PTM && m->d_rec28 == NULL) {
        ssw_set_error("two_pass_history in the default configuration needs codebooks of 128 densities");
        return -1;
    }
    if (d_carry_out != NULL && scorer == SSW_SCORER_PTM && n_frames > 0) {
        /* history slot 1 as every utterance's first pass leaves it (fpa_carry_rows_kernel): from
         * the features and the proven codebook masks -- d_cbm holds, for every utterance, those of
         * the last plan of its frames */
        uint32_t *d_start = ws_at<uint32_t>(ws, o_start);
        if (stage_upload(m, d_start, sizeof(uint32_t) * n_start_words, st, [&](unsigned char *hs) {
                uint32_t *bits = reinterpret_cast<uint32_t *>(hs);
                memset(bits, 0, sizeof(uint32_t) * n_start_words);
                for (int u = 0; u < n_utts; ++u)
                    if (utt_off[u] < n_frames)
                        bits[(size_t)utt_off[u] >> 5] |= 1u << (utt_off[u] & 31);
            }) < 0)
            return -1;
        FramesParams F;
        memset(&F, 0, sizeof(F));
        F.utt_start = d_start;
        F.utt_off = d_utt_off;
        F.n_utts = n_utts;
        F.seg_of_frame = d_iota;
        F.seg_cbmask = d_cbm;
        F.n_frames = n_frames;
        F.n_cbf = m->n_cbf;
        F.n_feat = h->n_feat;
        F.featdim = h->veclen_total;
        for (int f = 0; f < h->n_feat; ++f)
            F.featoff[f] = h->featoff[f];
        hipLaunchKernelGGL(fpa_carry_rows_kernel, dim3((unsigned)((size_t)n_utts * m->n_cbf)), dim3(64), 0,
                           st, F, m->d_rec28, d_feats, d_utt_off, d_carry_out);
        HIP_OK(hipGetLastError());
    }
    if (listed_out != NULL && n_frames > 0)
        HIP_OK(hipMemcpyAsync(listed_out, d_listed, sizeof(uint32_t) * (size_t)n_frames * (size_t)nw32,
                              hipMemcpyDeviceToHost, st));
    if (seed_out != NULL)
        HIP_OK(hipMemcpyAsync(seed_out, d_seed, sizeof(uint32_t) * (size_t)n_utts * (size_t)nw32,
                              hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    int more = 0;
    long long sum = 0;
    for (int u = 0; u < n_utts; ++u) {
        sum += rounds[(size_t)u];
        more += rounds[(size_t)u] > 1 ? 1 : 0;
    }
    stats[0] += n_utts;
    stats[1] += sum;
    stats[2] = n_round;
    stats[3] += more;
    if (rounds_out != NULL)
        memcpy(rounds_out, rounds.data(), sizeof(int32_t) * (size_t)n_utts);
    if (timing)
        fprintf(stderr, "%s: assumption (compallsen = yes scoring + search) "
                        "%.2f ms, %d round(s) %.2f ms\n", G.who, t_spec - t_in, n_round, now_ms() - t_spec);
    return 0;
}

/* the first pass's graphs: every utterance its own */
static int
first_pass_active_run(ssw_model_t *m, ssw_fp_graphs_t *g, int scorer, const float *d_feats,
                      int32_t n_frames, const int32_t *utt_off, int32_t n_utts, int32_t max_seg,
                      int32_t *n_seg, ssw_word_seg_t *seg, int16_t *d_rows, bool full_rows,
                      uint32_t *seed_out, int32_t *rounds_out, void *stream, uint32_t *d_carry_out)
{
    fpa_fp_search_t a = { m, g, utt_off, n_utts, max_seg, n_seg, seg, stream };
    fpa_graph_t G;
    G.who = "ssw_first_pass_batch_active";
    G.n_nodes = g->n_nodes;
    G.senid = g->senid;
    G.max_nodes = 0;
    for (int u = 0; u < n_utts; ++u) {
        G.node_base.push_back(g->node_off[u]);
        G.node_cnt.push_back(g->node_off[u + 1] - g->node_off[u]);
    }
    G.search = fpa_fp_search;
    G.arg = &a;
    return fpa_run(m, G, scorer, d_feats, n_frames, utt_off, n_utts, d_rows, full_rows, seed_out,
                   rounds_out, NULL, m->fpa_stats, stream, d_carry_out);
}

/* The s2_semi scorer in the *_active calls.  s2_semi_mgau_frame_eval evaluates every Gaussian and
 * normalises per stream by its best density whatever the active set is (src/s2_semi_mgau.c:
 * 841-872): compallsen = no only restricts which senones are summed, and the search reads the
 * listed ones alone.  The default configuration's search therefore reads the very scores of the
 * compallsen = yes rows, and these calls take that route: one search, nothing to prove.  The
 * stats report one round per utterance and every first assumption accepted; the sets of listed
 * senones are not made (seed_active / listed are refused), d_senscr receives whole rows. */
static void
semi_active_done(int64_t stats[4], int32_t n_utts, int32_t *rounds)
{
    stats[0] += n_utts;
    stats[1] += n_utts;
    stats[2] = 1;
    for (int u = 0; rounds != NULL && u < n_utts; ++u)
        rounds[u] = 1;
}

extern "C" int
ssw_first_pass_batch_active(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                            int scorer, const float *d_feats, int32_t n_frames,
                            const int32_t *utt_off, int32_t n_utts, const int32_t *word_off,
                            const char *const *words, int32_t max_seg, int32_t *n_seg,
                            ssw_word_seg_t *seg, uint32_t *seed_active, int16_t *d_senscr,
                            int32_t *rounds, void *stream)
{
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
    if (cont_refuse_active(m, "ssw_first_pass_batch_active") < 0)
        return -1;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    int16_t *rows = d_senscr;
    if (rows == NULL) { /* the model's own rows (ssw_align_text_batch's workspace) */
        HIP_OK(hipSetDevice(m->device));
        if (text_rows_reserve(m, n_frames, "ssw_first_pass_batch_active") < 0)
            return -1;
        rows = m->text_scr.as<int16_t>();
    }
    if (scorer == SSW_SCORER_S2_SEMI) { /* the compallsen = yes route (semi_active_done) */
        if (seed_active != NULL) {
            ssw_set_error("ssw_first_pass_batch_active: the s2_semi scorer makes no sets of listed "
                          "senones (seed_active)");
            return -1;
        }
        if (n_frames > 0
            && ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, rows, stream) < 0)
            return -1;
        if (ssw_first_pass_batch(m, d, cfg, rows, n_frames, utt_off, n_utts, word_off, words, max_seg,
                                 n_seg, seg, stream) < 0)
            return -1;
        semi_active_done(m->fpa_stats, n_utts, rounds);
        return 0;
    }
    ssw_fp_graphs_t *g = ssw_fp_graphs_build(m, d, cfg, n_utts, word_off, words);
    if (g == NULL)
        return -1;
    const int rc = first_pass_active_run(m, g, scorer, d_feats, n_frames, utt_off, n_utts, max_seg,
                                         n_seg, seg, rows, d_senscr != NULL, seed_active, rounds,
                                         stream);
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
    if (cont_refuse_active(m, "ssw_align_text_batch_active") < 0)
        return NULL;
    if (scorer == SSW_SCORER_S2_SEMI) { /* the compallsen = yes route (semi_active_done) */
        ssw_alignment_set_t *a = ssw_align_text_batch(m, d, cfg, scorer, d_feats, n_frames, utt_off,
                                                      n_utts, word_off, words, stream);
        if (a != NULL)
            semi_active_done(m->fpa_stats, n_utts, NULL);
        return a;
    }
    if (hipSetDevice(m->device) != hipSuccess)
        return NULL;
    if (text_rows_reserve(m, n_frames, "ssw_align_text_batch_active") < 0)
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
    F.d_senscr = m->text_scr.as<int16_t>();
    F.n_frames = n_frames;
    F.utt_off = utt_off;
    F.n_utts = plan->n_utts;
    F.stream = stream;
    F.reject = c.any ? &c.reject : NULL;
    F.fpa = &mode;
    ssw_alignment_set_t *a = forced_align_core(m, F);
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
