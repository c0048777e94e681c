/* ssw_host_firstpass.inc -- host: ssw_first_pass_batch.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* first pass of forced alignment (SURVEY 8(f) row 4)                                   */
/* ---------------------------------------------------------------------------------- */
/* A plan is the host half of the first pass: the graphs of a batch of texts.  Building it
 * touches no device, so it can be done (on another host thread) while the GPU works on the
 * previous batch. */
struct ssw_first_pass_plan_s {
    ssw_fp_graphs_t *g;
    int32_t n_utts, max_words;
};

extern "C" ssw_first_pass_plan_t *
ssw_first_pass_prepare(const ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                       int32_t n_utts, const int32_t *word_off, const char *const *words)
{
    if (n_utts < 0 || !word_off || !words || !d) {
        ssw_set_error("bad arguments to ssw_first_pass_prepare");
        return NULL;
    }
    ssw_fp_graphs_t *g = ssw_fp_graphs_build(m, d, cfg, n_utts, word_off, words);
    if (g == NULL)
        return NULL;
    ssw_first_pass_plan_t *p = new ssw_first_pass_plan_t();
    p->g = g;
    p->n_utts = n_utts;
    p->max_words = 0;
    for (int u = 0; u < n_utts; ++u)
        p->max_words = std::max(p->max_words, word_off[u + 1] - word_off[u]);
    return p;
}

extern "C" void
ssw_first_pass_plan_free(ssw_first_pass_plan_t *p)
{
    if (p == NULL)
        return;
    ssw_fp_graphs_free(p->g);
    delete p;
}

/* One run of the first pass over a batch's graphs: what every caller fills, by name. */
struct FpExport {
    /* where the kernels write the sets of active HMMs (the default configuration's rounds,
     * ssw_host_fpactive.inc); all NULL: a plain search */
    unsigned long long *mask;
    const long long *act_off;
    const int *node_cnt; /* device [n_utts]: phone-tree HMMs of every utterance's graph */
};
struct FpReq {
    ssw_fp_graphs_t *g;      /* the graphs stay the caller's */
    const int16_t *d_senscr; /* the score rows the search reads */
    const int32_t *utt_off;
    int32_t n_utts, max_seg;
    int32_t *n_seg;
    ssw_word_seg_t *seg;
    void *stream;
    double t0; /* when the caller began (its graphs included), for SSW_ALIGN_TIMING's line */
    /* the utterances to search (the rounds of ssw_first_pass_batch_active), NULL or empty =
     * all; the others keep what they have */
    const std::vector<int> *subset;
    FpExport exp;
};

static int first_pass_run(ssw_model_t *m, const FpReq &R);

extern "C" int
ssw_first_pass_batch(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                     const int16_t *d_senscr, int32_t n_frames, const int32_t *utt_off,
                     int32_t n_utts, const int32_t *word_off, const char *const *words,
                     int32_t max_seg, int32_t *n_seg, ssw_word_seg_t *seg, void *stream)
{
    if (n_utts == 0)
        return 0;
    if (check_has_device(m) < 0)
        return -1;
    if (n_utts < 0 || n_frames < 0 || max_seg < 1 || !utt_off || !word_off || !words || !n_seg
        || !seg || !d || !utt_off_spans(utt_off, n_utts, n_frames)) {
        ssw_set_error("bad arguments to ssw_first_pass_batch");
        return -1;
    }
    FpReq R{};
    R.t0 = now_ms();
    R.g = ssw_fp_graphs_build(m, d, cfg, n_utts, word_off, words);
    if (R.g == NULL)
        return -1;
    R.d_senscr = d_senscr;
    R.utt_off = utt_off;
    R.n_utts = n_utts;
    R.max_seg = max_seg;
    R.n_seg = n_seg;
    R.seg = seg;
    R.stream = stream;
    const int rc = first_pass_run(m, R);
    ssw_fp_graphs_free(R.g);
    return rc;
}

extern "C" int
ssw_first_pass_run(ssw_model_t *m, const ssw_first_pass_plan_t *plan, const int16_t *d_senscr,
                   int32_t n_frames, const int32_t *utt_off, int32_t max_seg, int32_t *n_seg,
                   ssw_word_seg_t *seg, void *stream)
{
    if (plan == NULL || plan->n_utts == 0)
        return 0;
    if (check_has_device(m) < 0)
        return -1;
    if (n_frames < 0 || max_seg < 1 || !utt_off || !n_seg || !seg
        || !utt_off_spans(utt_off, plan->n_utts, n_frames)) {
        ssw_set_error("bad arguments to ssw_first_pass_run");
        return -1;
    }
    FpReq R{};
    R.t0 = now_ms();
    R.g = plan->g;
    R.d_senscr = d_senscr;
    R.utt_off = utt_off;
    R.n_utts = plan->n_utts;
    R.max_seg = max_seg;
    R.n_seg = n_seg;
    R.seg = seg;
    R.stream = stream;
    return first_pass_run(m, R);
}

/* upload the graphs, search, bring the segmentations back; the graphs stay the caller's */
static int first_pass_run_impl(ssw_model_t *m, const FpReq &R, int level, const std::vector<int> &only);

static int
first_pass_run(ssw_model_t *m, const FpReq &R)
{
    /* long texts, three levels.  2: first_pass_win_kernel (HMMs in registers, a sliding window
     * of nodes, banded history table); 1: first_pass_big_kernel<.., true> (node state in HBM,
     * banded node walk and history table); 0: the same with the full [frame][leaf] table.  An
     * utterance that outgrows a level's window or budget says so (-(1 << 30)) and is searched
     * again one level down -- it alone: the others keep what they have (`only`).
     * SSW_FP_BAND=0: level 0 at once; SSW_FP_WIN=0: never 2. */
    refresh_knobs(m);
    int level = !m->kn.fp_band ? 0 : !m->kn.fp_win ? 1 : 2;
    std::vector<int> only; /* empty: all of them */
    if (R.subset != NULL)
        only = *R.subset;
    for (;;) {
        int rc = first_pass_run_impl(m, R, level, only);
        if (rc != 0 || level == 0)
            return rc;
        std::vector<int> left;
        if (only.empty()) {
            for (int u = 0; u < R.n_utts; ++u)
                if (R.n_seg[u] == -(1 << 30))
                    left.push_back(u);
        } else {
            for (int u : only)
                if (R.n_seg[u] == -(1 << 30))
                    left.push_back(u);
        }
        if (left.empty())
            return rc;
        only.swap(left);
        --level;
    }
}

/* The device tables of one launch.  One staging buffer -> one copy (WsLayout).  What changes
 * from call to call comes last among the uploaded tables -- the utterance offsets and hist_off
 * excepted, which lie ahead of the graph's: `o_call` is where the graph's tables end. */
struct FpTables {
    WsLayout L;
    FirstPassParams P;
    WsLayout::Piece resent[2]; /* utt_off, hist_off: ahead of the graph's tables, yet a call's own */
    size_t o_call;

    FpTables() {}
    FpTables(const FpTables &) = delete; /* (L holds the addresses of P's pointers) */
    FpTables &operator=(const FpTables &) = delete;
};

static void
fp_layout(FpTables &T, const ssw_model_t *m, const FpReq &R, const FpShape &S, const std::vector<int> &only)
{
    const ssw_fp_graphs_t *g = R.g;
    const size_t nU = (size_t)R.n_utts, nN = (size_t)g->n_nodes, nL = (size_t)g->n_leaves;
    WsLayout &L = T.L;
    FirstPassParams &P = T.P;
    L.in(&P.utt_off, R.utt_off, sizeof(int) * (nU + 1));
    T.resent[0] = L.ins.back();
    L.in(&P.node_off, g->node_off, sizeof(int) * (nU + 1));
    L.in(&P.leaf_off, g->leaf_off, sizeof(int) * (nU + 1));
    L.in(&P.state_off, g->state_off, sizeof(int) * (nU + 1));
    L.in(&P.senid, g->senid, sizeof(uint16_t) * 4 * nN);
    L.in(&P.pen, g->pen, sizeof(int) * nN);
    L.in(&P.parent, g->parent, sizeof(int) * nN);
    L.in(&P.info, g->info, sizeof(uint32_t) * nN);
    L.in(&P.ctxt, g->ctxt, sizeof(uint64_t) * nN);
    L.in(&P.leaf_ord, g->leaf_ord, sizeof(int) * nN);
    L.in(&P.leaf_wid, g->leaf_wid, sizeof(int) * nL);
    L.in(&P.leaf_to, g->leaf_to, sizeof(int) * nL);
    L.in(&P.leaf_node, g->leaf_node, sizeof(int) * nL);
    L.in(&P.in_off, g->in_off, sizeof(int) * ((size_t)g->n_states + 1));
    L.in(&P.in_leaf, g->in_leaf, sizeof(int) * (size_t)g->n_in);
    L.in(&P.hist_off, S.hist_off.data(), sizeof(long long) * nU);
    T.resent[1] = L.ins.back();
    L.in(&P.tw, g->tw, sizeof(int) * (size_t)g->n_tw);
    L.in(&P.tw_off, g->tw_off, sizeof(int) * (nU + 1));
    L.in(&P.twin_ref, g->twin_ref, sizeof(int) * nN);
    L.in(&P.tw_rk, g->tw_rk, sizeof(int) * nU);
    T.o_call = L.mark();
    L.in(&P.big_off, S.big_off.data(), sizeof(long long) * nU);
    L.in(&P.only, only.data(), sizeof(int) * only.size()); /* (NULL for all of them, once resolved) */
    L.out(&P.n_seg, sizeof(int) * nU);
    L.out(&P.seg, sizeof(ssw_word_seg_t) * nU * (size_t)R.max_seg);
    L.out(&P.hist, sizeof(int2) * (S.hist_total ? S.hist_total : 1));
    L.out(&P.big_ws, sizeof(int) * S.big_ints);
    P.senscr = R.d_senscr;
    P.tp = (const uint32_t *)m->d_tp;
    P.n_sen = m->h->n_sen;
    P.max_seg = R.max_seg;
    P.beam = g->beam;
    P.pbeam = g->pbeam;
    P.wbeam = g->wbeam;
    P.sil = m->h->sil;
    P.hist_band = S.hist_band;
    P.act_mask = R.exp.mask;
    P.act_off = R.exp.act_off;
}

/* The cached-graphs policy.  The same graphs searched again (the rounds of
 * ssw_first_pass_batch_active, a level's leftovers, a plan run on several recordings): their
 * tables are on the device already, and all that goes up is what changes from call to call --
 * what lies behind `o_call` (big_off, only) and the two small tables ahead of the graph's that a
 * call may change (utt_off: a plan's texts meet new recordings; hist_off).  Keyed by the graphs'
 * uid, not their address, and by `o_call`; a workspace that moved took the cached graphs with
 * it.  The graphs go up on a stream of their own: whatever the caller's stream still has to do
 * (ssw_align_text_batch: the scoring kernels) does not hold the copy back; the search then
 * waits for both.  `stage` must outlive its copy: on the success path the wait on ev_up and the
 * caller's synchronise cover that, after an error failed() does. */
struct FpUpload {
    std::vector<unsigned char> stage;

    /* the workspace, grown if need be; -1 with the error set */
    int reserve(ssw_model_t *m, size_t bytes)
    {
        bool moved = false;
        const int got = devbuf_reserve(m->fp_ws, bytes, "ssw_first_pass_batch", bytes / 4, &moved);
        if (moved)
            m->fp_ws_uid = 0;
        return got;
    }
    hipError_t send(ssw_model_t *m, const ssw_fp_graphs_t *g, const FpTables &T, hipStream_t st)
    {
        const bool cached = m->fp_ws_uid != 0 && m->fp_ws_uid == g->uid
            && m->fp_ws_uid_bytes == T.o_call;
        const size_t up_from = cached ? T.o_call : 0, in_bytes = T.L.in_bytes();
        stage.resize(in_bytes - up_from + 1);
        T.L.fill(stage.data(), up_from);
        hipError_t e = hipSuccess;
        if (m->s_up == NULL) {
            e = hipStreamCreateWithFlags(&m->s_up, hipStreamNonBlocking);
            if (e == hipSuccess)
                e = hipEventCreateWithFlags(&m->ev_up, hipEventDisableTiming);
        }
        if (e == hipSuccess && in_bytes > up_from)
            e = hipMemcpyAsync(m->fp_ws.p + up_from, stage.data(), in_bytes - up_from,
                               hipMemcpyHostToDevice, m->s_up);
        for (int k = 0; k < 2 && e == hipSuccess && cached; ++k)
            e = hipMemcpyAsync(m->fp_ws.p + T.resent[k].off, T.resent[k].src, T.resent[k].bytes,
                               hipMemcpyHostToDevice, m->s_up);
        if (e == hipSuccess) {
            m->fp_ws_uid = g->uid;
            m->fp_ws_uid_bytes = T.o_call;
        } else
            m->fp_ws_uid = 0;
        if (e == hipSuccess)
            e = hipEventRecord(m->ev_up, m->s_up);
        if (e == hipSuccess)
            e = hipStreamWaitEvent(st, m->ev_up, 0);
        return e;
    }
    /* `stage` goes out of scope with this: the upload stream must be done with it first */
    void failed(ssw_model_t *m)
    {
        if (m->s_up != NULL)
            (void)hipStreamSynchronize(m->s_up);
    }
};

/* the shape's kernel instance, over n_run utterances */
static hipError_t
fp_launch(const FpShape &S, const FirstPassParams &P, const FpExport &x, int n_run, hipStream_t st)
{
    const bool exp = x.mask != NULL;
    const int t = S.tpb;
    void (*kern)(FirstPassParams) = first_pass_big_kernel<1024, false>; /* FP_HBM */
    if (S.kind == FP_WIN)
        kern = t == 1024 ? first_pass_win_kernel<1024>
            : t == 512   ? first_pass_win_kernel<512>
                         : first_pass_win_kernel<256>;
    else if (S.kind == FP_HBM_BAND)
        kern = t == 1024 ? first_pass_big_kernel<1024, true>
            : t == 512   ? first_pass_big_kernel<512, true>
                         : first_pass_big_kernel<256, true>;
    else if (S.kind == FP_REG && t == 256)
        kern = exp ? first_pass_kernel<256, true> : first_pass_kernel<256>;
    else if (S.kind == FP_REG && t == 512)
        kern = exp ? first_pass_kernel<512, true> : first_pass_kernel<512>;
    else if (S.kind == FP_REG)
        kern = exp ? first_pass_kernel<1024, true> : first_pass_kernel<1024>;
    hipError_t e = hipSuccess;
    if (S.lds_bytes > 48 * 1024)
        e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)S.lds_bytes);
    if (e == hipSuccess && S.clear_mask) {
        hipLaunchKernelGGL(fpa_clear_kernel, dim3(n_run), dim3(256), 0, st, P.act_mask, P.act_off,
                           P.utt_off, x.node_cnt, P.only);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kern, dim3(n_run), dim3(S.tpb), S.lds_bytes, st, P);
        e = hipGetLastError();
    }
    return e;
}

/* The results, on the host when this returns: all of them, or a level's leftovers -- their rows
 * alone, copied one by one when they are few, picked out of one copy of the whole arrays
 * otherwise (round 6: 256 utterances run again cost 512 small copies, 7 ms) */
static hipError_t
fp_fetch(const FpReq &R, const FirstPassParams &P, const std::vector<int> &only, hipStream_t st)
{
    const size_t nU = (size_t)R.n_utts, row = (size_t)R.max_seg;
    const bool whole = only.empty() || only.size() > 8;
    std::vector<int> all_n;
    std::vector<ssw_word_seg_t> all_seg;
    int32_t *n_to = R.n_seg;
    ssw_word_seg_t *seg_to = R.seg;
    if (!only.empty() && whole) {
        all_n.resize(nU);
        all_seg.resize(nU * row);
        n_to = all_n.data();
        seg_to = all_seg.data();
    }
    hipError_t e = hipSuccess;
    if (whole) {
        e = hipMemcpyAsync(n_to, P.n_seg, sizeof(int) * nU, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(seg_to, P.seg, sizeof(ssw_word_seg_t) * nU * row, hipMemcpyDeviceToHost, st);
    } else
        for (size_t i = 0; i < only.size() && e == hipSuccess; ++i) {
            const size_t u = (size_t)only[i];
            e = hipMemcpyAsync(R.n_seg + u, P.n_seg + u, sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(R.seg + u * row, P.seg + u * row, sizeof(ssw_word_seg_t) * row,
                                   hipMemcpyDeviceToHost, st);
        }
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e == hipSuccess && !all_n.empty())
        for (int u : only) {
            R.n_seg[u] = all_n[(size_t)u];
            memcpy(R.seg + (size_t)u * row, all_seg.data() + (size_t)u * row, sizeof(ssw_word_seg_t) * row);
        }
    return e;
}

static int
first_pass_run_impl(ssw_model_t *m, const FpReq &R, int level, const std::vector<int> &only)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    if (R.n_utts == 0)
        return 0;
    const ssw_fp_graphs_t *g = R.g;
    hipStream_t st = (hipStream_t)R.stream;
    const double t1 = now_ms();
    /* the utterances of this launch: all, or the ones named (their sizes alone pick the kernel
     * and size the workspaces; the others' results stay as they are, on both sides) */
    std::vector<char> runs((size_t)R.n_utts, only.empty() ? 1 : 0);
    for (int u : only)
        runs[(size_t)u] = 1;
    const int n_run = only.empty() ? R.n_utts : (int)only.size();
    const FpGraphSizes sizes = { g->node_off, g->leaf_off, g->state_off, g->tw_off, g->tw_rk };
    const FpKnobs knobs = { !strcmp(m->kn.fp_kernel, "big"), m->kn.fp_hist_band, m->kn.fp_big_tpb,
                            m->kn.fp_win_tpb };
    FpShape S;
    if (fp_shape(sizes, R.utt_off, R.n_utts, runs.data(), level, knobs, R.exp.mask != NULL, S) < 0) {
        ssw_set_error("%s", S.err);
        return -1;
    }
    FpTables T;
    fp_layout(T, m, R, S, only);
    FpUpload up;
    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess && up.reserve(m, T.L.size()) < 0)
        return -1;
    if (e == hipSuccess)
        e = up.send(m, g, T, st);
    if (e == hipSuccess) {
        T.L.resolve(m->fp_ws.p);
        if (only.empty())
            T.P.only = NULL;
        e = fp_launch(S, T.P, R.exp, n_run, st);
    }
    if (e == hipSuccess)
        e = fp_fetch(R, T.P, only, st);
    if (e != hipSuccess) {
        up.failed(m);
        ssw_set_error("ssw_first_pass_batch: %s", hipGetErrorString(e));
    }
    if (m->kn.align_timing)
        fprintf(stderr, "ssw_first_pass_batch: graphs %.2f ms (%d HMMs), upload + search + results "
                        "%.2f ms\n", t1 - R.t0, g->n_nodes, now_ms() - t1);
    return e == hipSuccess ? 0 : -1;
}

/* ---------------------------------------------------------------------------------- */
/* decoder_alignment for a batch (src/decoder.c:737-798)                                */
/* ---------------------------------------------------------------------------------- */
struct ssw_alignment_set_s {
    const ssw_model_t *m;
    const ssw_dict_t *d;
    std::vector<int32_t> n_frames;
    int32_t n_utts;
    std::vector<int32_t> status, word_off, phone_off;
    std::vector<std::string> message; /* per utterance: why its text was rejected (status 3) */
    /* empty, or per utterance decoder_hyp's text as the grammar search built it: the sets of
     * ssw_recognition_set_align and its kin, for ssw_alignment_set_json's top-level "t" */
    std::vector<std::string> hyp;
    std::vector<int32_t> wid, cipid, parent;
    std::vector<uint16_t> senid;
    std::vector<ssw_align_entry_t> word_al, phone_al, state_al;
};

/* the default configuration (ssw_host_fpactive.inc): both passes score for themselves, from the
 * features, what their searches hold active; d_senscr is then the first pass's row workspace */
struct fpa_mode_t {
    int scorer;
    const float *d_feats;
    bool two_pass; /* cfg->two_pass_history: the second pass starts from what the first left */
};
/* One call of the loop of speculation and proof (fpa_run, ssw_host_fpactive.inc), filled by name;
 * what is not set is NULL / 0. */
struct FpaReq {
    int scorer;
    const float *d_feats;
    int32_t n_frames;
    const int32_t *utt_off;
    int32_t n_utts;
    int16_t *d_rows;       /* device int16 [n_frames][n_sen]: the rows the call scores into
                              (workspace and, with full_rows, output) */
    bool full_rows;        /* the rows as acmod's buffer would hold them, unlisted entries written */
    uint32_t *seed_out;    /* NULL or host [n_utts][(n_sen + 31) / 32]: acmod's flags after every
                              utterance's last frame */
    int32_t *rounds_out;   /* NULL or host [n_utts]: searches of the utterance over default-
                              configuration scores until its sets were proven (1 = the assumed
                              trajectory was already the right one) */
    uint32_t *listed_out;  /* NULL or host [n_frames][(n_sen + 31) / 32]: the proven listed senones
                              of every frame, bridges included */
    uint32_t *d_carry_out; /* NULL or device [n_utts][n_cbf]: history slot 1 as every utterance's
                              first pass leaves it (two_pass_history) */
    int64_t *stats;        /* the four counters the call feeds (fpa_stats / gra_stats) */
    void *stream;
};
/* the first pass's: the request, and what is the first pass's own */
static int first_pass_active_run(ssw_model_t *m, const FpaReq &R, ssw_fp_graphs_t *g, int32_t max_seg,
                                 int32_t *n_seg, ssw_word_seg_t *seg);

/* decoder_alignment for a batch of texts: the first pass, then align_word_segments.  The texts
 * come as a plan, or as cfg + word_off + words. */
struct ForcedAlignReq {
    const ssw_dict_t *d;
    const ssw_first_pass_config_t *cfg;
    const ssw_first_pass_plan_t *plan;
    const int16_t *d_senscr;
    int32_t n_frames;
    const int32_t *utt_off;
    int32_t n_utts;
    const int32_t *word_off;
    const char *const *words;
    void *stream;
    const std::vector<std::string> *reject; /* NULL, or per utterance why its text was rejected */
    int (*between)(void *); /* NULL, or called once before the second pass */
    void *between_arg;
    const fpa_mode_t *fpa; /* NULL: both passes read d_senscr */
};
static ssw_alignment_set_t *forced_align_core(ssw_model_t *m, const ForcedAlignReq &F);

/* decoder_alignment from alignment_add_word on (src/decoder.c:765-797), for a batch whose word
 * windows are known: forced_align_core's second half, and what follows a grammar search
 * (ssw_host_grammar.inc). */
struct AlignSegReq {
    const ssw_dict_t *d;
    const int16_t *d_senscr;
    const int32_t *utt_off;
    int32_t n_utts;
    /* utterance u has n_seg[u] words at seg + u * max_seg; n_seg[u] < 0: none, reported with
     * status pre_status[u] (NULL: 1) and (*message)[u] (the strings are taken) */
    const int32_t *n_seg;
    const ssw_word_seg_t *seg;
    int32_t max_seg;
    const int32_t *pre_status;
    std::vector<std::string> *message;
    /* fpa: the default configuration, with `seed` (host [n_utts][(n_sen + 31) / 32]) and d_carry
     * (NULL, or device [n_utts][n_cbf]); else the second pass reads d_senscr */
    const fpa_mode_t *fpa;
    const uint32_t *seed;
    const uint32_t *d_carry;
    int (*between)(void *); /* NULL, or called once before the second pass */
    void *between_arg;
    void *stream;
    double first_ms; /* for SSW_ALIGN_TIMING's line, the time the caller's first pass took */
};
static ssw_alignment_set_t *align_word_segments(ssw_model_t *m, const AlignSegReq &Q);

/* decoder_set_align_text fails for the one utterance whose text has a word the dictionary does
 * not know (src/decoder.c:699-703); in a batch the others must still be aligned.  The texts are
 * checked here; a rejected one is searched as an empty text (its grammar is then one state with
 * the filler loops: always buildable) and reported with status 3 and the reference's message. */
struct checked_texts_t {
    std::vector<int32_t> word_off;
    std::vector<const char *> words;
    std::vector<std::string> reject;
    bool any = false;
};

static void
check_texts(const ssw_dict_t *d, int32_t n_utts, const int32_t *word_off, const char *const *words,
            checked_texts_t &c)
{
    c.reject.assign((size_t)n_utts, std::string());
    for (int u = 0; u < n_utts && !c.any; ++u)
        for (int i = word_off[u]; i < word_off[u + 1]; ++i)
            if (ssw_dict_word_id(d, words[i]) < 0) {
                c.any = true;
                break;
            }
    if (!c.any)
        return;
    c.word_off.assign((size_t)n_utts + 1, 0);
    for (int u = 0; u < n_utts; ++u) {
        for (int i = word_off[u]; i < word_off[u + 1]; ++i)
            if (ssw_dict_word_id(d, words[i]) < 0) {
                c.reject[u] = std::string("Unknown word ") + words[i];
                break;
            }
        if (c.reject[u].empty())
            c.words.insert(c.words.end(), words + word_off[u], words + word_off[u + 1]);
        c.word_off[u + 1] = (int32_t)c.words.size();
    }
    if (c.words.empty())
        c.words.push_back("");
}

extern "C" ssw_alignment_set_t *
ssw_forced_align_batch(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                       const int16_t *d_senscr, int32_t n_frames, const int32_t *utt_off,
                       int32_t n_utts, const int32_t *word_off, const char *const *words,
                       void *stream)
{
    if (n_utts < 0 || !utt_off || !word_off || !words || !d) {
        ssw_set_error("bad arguments to ssw_forced_align_batch");
        return NULL;
    }
    checked_texts_t c;
    check_texts(d, n_utts, word_off, words, c);
    ForcedAlignReq F{};
    F.d = d;
    F.cfg = cfg;
    F.d_senscr = d_senscr;
    F.n_frames = n_frames;
    F.utt_off = utt_off;
    F.n_utts = n_utts;
    F.word_off = c.any ? c.word_off.data() : word_off;
    F.words = c.any ? c.words.data() : words;
    F.stream = stream;
    F.reject = c.any ? &c.reject : NULL;
    return forced_align_core(m, F);
}

extern "C" ssw_alignment_set_t *
ssw_forced_align_planned(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_plan_t *plan,
                         const int16_t *d_senscr, int32_t n_frames, const int32_t *utt_off,
                         void *stream)
{
    if (!plan || !utt_off || !d) {
        ssw_set_error("bad arguments to ssw_forced_align_planned");
        return NULL;
    }
    ForcedAlignReq F{};
    F.d = d;
    F.plan = plan;
    F.d_senscr = d_senscr;
    F.n_frames = n_frames;
    F.utt_off = utt_off;
    F.n_utts = plan->n_utts;
    F.stream = stream;
    return forced_align_core(m, F);
}

/* the first pass of F in the default configuration (F.fpa): the rows are its workspace, the seed
 * of the second pass and, with two_pass_history, the carried orders come out */
static FpaReq
forced_align_fpa_req(ssw_model_t *m, const ForcedAlignReq &F, uint32_t *seed, bool carry2)
{
    FpaReq A{};
    A.scorer = F.fpa->scorer;
    A.d_feats = F.fpa->d_feats;
    A.n_frames = F.n_frames;
    A.utt_off = F.utt_off;
    A.n_utts = F.n_utts;
    A.d_rows = const_cast<int16_t *>(F.d_senscr);
    A.seed_out = seed;
    A.d_carry_out = carry2 ? m->carry_rows.as<uint32_t>() : NULL;
    A.stats = m->fpa_stats;
    A.stream = F.stream;
    return A;
}

static ssw_alignment_set_t *
forced_align_core(ssw_model_t *m, const ForcedAlignReq &F)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    const ssw_host_model_t *h = m->h;
    const ssw_first_pass_plan_t *plan = F.plan;
    const fpa_mode_t *fpa = F.fpa;
    const int n_utts = F.n_utts;
    refresh_knobs(m);
    const double t_a = now_ms();
    int max_words = plan ? plan->max_words : 0;
    for (int u = 0; !plan && u < n_utts; ++u)
        max_words = std::max(max_words, F.word_off[u + 1] - F.word_off[u]);
    /* every word can be followed by fillers and a silence loop can repeat: start with room for
     * that; a backtrace that needs more says how much (n_seg = -(2 + needed)), and the batch is
     * searched again with room for the longest one -- never reported as a failed search, and
     * never dependent on which other utterances share the batch (the result of an utterance does
     * not depend on the buffer size once it fits) */
    int max_seg = 8 * max_words + 32;
    std::vector<int32_t> n_seg((size_t)n_utts);
    std::vector<ssw_word_seg_t> seg;
    ssw_first_pass_plan_t *own_plan = NULL;
    const size_t nw32 = ((size_t)h->n_sen + 31) / 32;
    std::vector<uint32_t> seed; /* default configuration: acmod's set after the first pass */
    if (fpa != NULL)
        seed.assign((size_t)n_utts * nw32, 0u);
    const bool carry2 = fpa != NULL && fpa->two_pass && fpa->scorer == SSW_SCORER_PTM && n_utts > 0;
    if (carry2 && carry_rows_reserve(m, n_utts, "ssw_align_text_batch_active") < 0)
        return NULL;
    for (int attempt = 0; n_utts && attempt < 2; ++attempt) {
        seg.assign((size_t)n_utts * max_seg, ssw_word_seg_t());
        if (!plan && (attempt == 1 || fpa != NULL) && own_plan == NULL) { /* build the graphs once more only in this rare case */
            own_plan = ssw_first_pass_prepare(m, F.d, F.cfg, n_utts, F.word_off, F.words);
            if (own_plan == NULL)
                return NULL;
        }
        const ssw_first_pass_plan_t *use = plan ? plan : own_plan;
        const int rc = fpa != NULL
            ? first_pass_active_run(m, forced_align_fpa_req(m, F, seed.data(), carry2), use->g,
                                    max_seg, n_seg.data(), seg.data())
            : use ? ssw_first_pass_run(m, use, F.d_senscr, F.n_frames, F.utt_off, max_seg,
                                       n_seg.data(), seg.data(), F.stream)
                  : ssw_first_pass_batch(m, F.d, F.cfg, F.d_senscr, F.n_frames, F.utt_off, n_utts,
                                         F.word_off, F.words, max_seg, n_seg.data(), seg.data(),
                                         F.stream);
        if (rc < 0) {
            ssw_first_pass_plan_free(own_plan);
            return NULL;
        }
        int need = 0;
        for (int u = 0; u < n_utts; ++u)
            if (n_seg[u] <= -2)
                need = std::max(need, -n_seg[u] - 2);
        if (need == 0)
            break;
        max_seg = need;
    }
    ssw_first_pass_plan_free(own_plan);
    std::vector<std::string> message((size_t)n_utts);
    std::vector<int32_t> pre_status((size_t)n_utts, 1);
    if (F.reject != NULL) /* these were searched as empty texts: no alignment for them */
        for (int u = 0; u < n_utts; ++u)
            if (!(*F.reject)[u].empty()) {
                message[u] = (*F.reject)[u];
                pre_status[u] = 3;
                n_seg[u] = -1;
            }
    AlignSegReq Q{};
    Q.d = F.d;
    Q.d_senscr = F.d_senscr;
    Q.utt_off = F.utt_off;
    Q.n_utts = n_utts;
    Q.n_seg = n_seg.data();
    Q.seg = seg.data();
    Q.max_seg = max_seg;
    Q.pre_status = pre_status.data();
    Q.message = &message;
    Q.fpa = fpa;
    Q.seed = seed.data();
    Q.d_carry = carry2 ? m->carry_rows.as<uint32_t>() : NULL;
    Q.between = F.between;
    Q.between_arg = F.between_arg;
    Q.stream = F.stream;
    Q.first_ms = now_ms() - t_a;
    return align_word_segments(m, Q);
}

/* fn(u0, u1) over [0, n_utts): utterances are independent, so a few host threads share them --
 * min(ssw_host_threads(), 32, n_utts / 16) of them, the caller alone below two */
template <typename F>
static void
for_utt_ranges(int n_utts, F &fn)
{
    const int n_thr = std::min(std::min(ssw_host_threads(), 32), n_utts / 16);
    if (n_thr < 2) {
        fn(0, n_utts);
        return;
    }
    struct job_t {
        F *fn;
        int n_utts, n_thr;
    } job = { &fn, n_utts, n_thr };
    ssw_parallel_for(n_thr, [](void *arg, int t) {
        const job_t *j = static_cast<const job_t *>(arg);
        (*j->fn)((int)((long long)j->n_utts * t / j->n_thr),
                 (int)((long long)j->n_utts * (t + 1) / j->n_thr));
    }, &job);
}

/* what align_word_segments' steps hand each other */
struct align_piece_t { /* one utterance's phones as alignment_populate left them */
    int np = -1;
    std::vector<int32_t> ssid, tmat, ci, par, st, du;
};
struct align_phones_t { /* the batch's phones, concatenated: what the second pass reads */
    std::vector<int16_t> tmat;
    std::vector<int32_t> sf, ef;
};

/* alignment_add_word + alignment_populate per utterance, with the first pass's windows
 * (populate is 150 triphone look-ups per utterance) */
static void
align_populate_words(const ssw_model_t *m, const AlignSegReq &Q, std::vector<align_piece_t> &piece)
{
    const int max_ph = 0xffff / std::max(1, m->h->n_emit_state);
    auto populate_range = [&](int u0, int u1) {
        std::vector<const char *> wstr;
        std::vector<int32_t> wstart, wdur, t_ssid((size_t)max_ph), t_tmat((size_t)max_ph),
            t_ci((size_t)max_ph), t_par((size_t)max_ph), t_st((size_t)max_ph), t_du((size_t)max_ph);
        for (int u = u0; u < u1; ++u) {
            if (Q.n_seg[u] < 0)
                continue;
            const ssw_word_seg_t *sg = Q.seg + (size_t)u * Q.max_seg;
            wstr.clear();
            wstart.clear();
            wdur.clear();
            for (int i = 0; i < Q.n_seg[u]; ++i) {
                wstr.push_back(ssw_dict_word(Q.d, sg[i].wid));
                wstart.push_back(sg[i].start);
                wdur.push_back(sg[i].duration);
            }
            align_piece_t &pc = piece[u];
            pc.np = ssw_alignment_populate(m, Q.d, Q.n_seg[u], wstr.data(), wstart.data(), wdur.data(),
                                           max_ph, t_ssid.data(), t_tmat.data(), t_ci.data(),
                                           t_par.data(), t_st.data(), t_du.data());
            if (pc.np < 0)
                continue;
            pc.ssid.assign(t_ssid.begin(), t_ssid.begin() + pc.np);
            pc.tmat.assign(t_tmat.begin(), t_tmat.begin() + pc.np);
            pc.ci.assign(t_ci.begin(), t_ci.begin() + pc.np);
            pc.par.assign(t_par.begin(), t_par.begin() + pc.np);
            pc.st.assign(t_st.begin(), t_st.begin() + pc.np);
            pc.du.assign(t_du.begin(), t_du.begin() + pc.np);
        }
    };
    for_utt_ranges(Q.n_utts, populate_range);
}

/* the pieces concatenated into the set, with every utterance's status so far */
static void
align_concat_pieces(const ssw_host_model_t *h, const AlignSegReq &Q, const std::vector<align_piece_t> &piece,
                    ssw_alignment_set_t *a, align_phones_t &ph)
{
    const int n_utts = Q.n_utts;
    std::vector<int32_t> ssid, tmat32, start, dur;
    for (int u = 0; u < n_utts; ++u) {
        a->word_off[u] = (int32_t)a->wid.size();
        a->phone_off[u] = (int32_t)a->cipid.size();
        if (Q.n_seg[u] < 0) {
            a->status[u] = Q.pre_status != NULL ? Q.pre_status[u] : 1;
            continue;
        }
        const align_piece_t &pc = piece[u];
        if (pc.np < 0) {
            a->status[u] = 2;
            continue;
        }
        const ssw_word_seg_t *sg = Q.seg + (size_t)u * Q.max_seg;
        for (int i = 0; i < Q.n_seg[u]; ++i)
            a->wid.push_back(sg[i].wid);
        a->cipid.insert(a->cipid.end(), pc.ci.begin(), pc.ci.end());
        a->parent.insert(a->parent.end(), pc.par.begin(), pc.par.end());
        ssid.insert(ssid.end(), pc.ssid.begin(), pc.ssid.end());
        tmat32.insert(tmat32.end(), pc.tmat.begin(), pc.tmat.end());
        start.insert(start.end(), pc.st.begin(), pc.st.end());
        dur.insert(dur.end(), pc.du.begin(), pc.du.end());
    }
    a->word_off[n_utts] = (int32_t)a->wid.size();
    a->phone_off[n_utts] = (int32_t)a->cipid.size();
    const size_t n_ph = a->cipid.size();
    const int ne = h->n_emit_state;
    a->senid.resize(n_ph * ne);
    a->state_al.assign(n_ph * ne, ssw_align_entry_t{ 0, 0, 0 });
    a->phone_al.assign(n_ph, ssw_align_entry_t{ 0, 0, 0 });
    a->word_al.assign(a->wid.size(), ssw_align_entry_t{ 0, 0, 0 });
    ph.tmat.resize(n_ph);
    ph.sf.resize(n_ph);
    ph.ef.resize(n_ph);
    for (size_t i = 0; i < n_ph; ++i) {
        for (int j = 0; j < ne; ++j) {
            a->senid[i * ne + j] = h->sseq[(size_t)ssid[i] * ne + j];
            /* what alignment_populate leaves in the state entries (src/ps_alignment.c:237-239) */
            a->state_al[i * ne + j].start = start[i];
            a->state_al[i * ne + j].duration = dur[i];
        }
        ph.tmat[i] = (int16_t)tmat32[i];
        ph.sf[i] = start[i] > 0 ? start[i] : 0; /* state_align_search_init, :464-471 */
        ph.ef[i] = dur[i] > 0 ? start[i] + dur[i] : INT_MAX;
    }
}

/* the second pass over every run of consecutive utterances that got through the first */
static int
align_second_pass(ssw_model_t *m, const AlignSegReq &Q, ssw_alignment_set_t *a, const align_phones_t &ph)
{
    const ssw_host_model_t *h = m->h;
    const int n_utts = Q.n_utts, ne = h->n_emit_state;
    const size_t nw32 = ((size_t)h->n_sen + 31) / 32;
    const int32_t *utt_off = Q.utt_off;
    std::vector<int32_t> foff, poff, st;
    for (int u0 = 0; u0 < n_utts;) {
        if (a->status[u0] != 0) {
            ++u0;
            continue;
        }
        int u1 = u0;
        while (u1 < n_utts && a->status[u1] == 0)
            ++u1;
        foff.clear();
        poff.clear();
        for (int u = u0; u <= u1; ++u) {
            foff.push_back(utt_off[u] - utt_off[u0]);
            poff.push_back(a->phone_off[u] - a->phone_off[u0]);
        }
        st.assign((size_t)(u1 - u0), 0);
        const size_t p0 = (size_t)a->phone_off[u0];
        const int rc2 = Q.fpa != NULL
            ? align_batch_active_impl(m, Q.fpa->scorer,
                                      Q.fpa->d_feats + (size_t)utt_off[u0] * h->veclen_total, u1 - u0,
                                      foff.data(), poff.data(), a->senid.data() + p0 * ne,
                                      ph.tmat.data() + p0, ph.sf.data() + p0, ph.ef.data() + p0,
                                      Q.seed + (size_t)u0 * nw32, a->state_al.data() + p0 * ne,
                                      st.data(), NULL, Q.stream,
                                      Q.d_carry != NULL ? Q.d_carry + (size_t)u0 * m->n_cbf : NULL)
            : ssw_align_batch(m, Q.d_senscr + (size_t)utt_off[u0] * h->n_sen, u1 - u0, foff.data(),
                              poff.data(), a->senid.data() + p0 * ne, ph.tmat.data() + p0,
                              ph.sf.data() + p0, ph.ef.data() + p0, a->state_al.data() + p0 * ne,
                              st.data(), Q.stream);
        if (rc2 < 0)
            return -1;
        for (int u = u0; u < u1; ++u)
            if (st[u - u0] != 0)
                a->status[u] = 2;
        u0 = u1;
    }
    return 0;
}

/* alignment_propagate: states -> phones -> words, the utterances shared out over the host
 * threads (one after the other they took 0.28 ms per 256 utterances, as long as a fifth of
 * the second pass's kernel) */
static int
align_propagate(ssw_alignment_set_t *a, int ne)
{
    std::atomic<int> failed{ 0 };
    auto propagate_range = [&](int ua, int ub) {
        std::vector<int32_t> sp;
        for (int u = ua; u < ub; ++u) {
            if (a->status[u] != 0)
                continue;
            const int p0 = a->phone_off[u], np = a->phone_off[u + 1] - p0;
            const int w0 = a->word_off[u], nw = a->word_off[u + 1] - w0;
            sp.resize((size_t)np * ne);
            for (int i = 0, k = 0; i < np; ++i)
                for (int j = 0; j < ne; ++j)
                    sp[k++] = i;
            if (ssw_alignment_propagate(a->state_al.data() + (size_t)p0 * ne, sp.data(), np * ne,
                                        a->phone_al.data() + p0, np) < 0
                || ssw_alignment_propagate(a->phone_al.data() + p0, a->parent.data() + p0, np,
                                           a->word_al.data() + w0, nw) < 0)
                failed.store(1);
        }
    };
    for_utt_ranges(a->n_utts, propagate_range);
    return failed.load() ? -1 : 0;
}

static ssw_alignment_set_t *
align_word_segments(ssw_model_t *m, const AlignSegReq &Q)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    refresh_knobs(m);
    const int n_utts = Q.n_utts;
    const double t_b = now_ms();
    std::unique_ptr<ssw_alignment_set_t> a(new ssw_alignment_set_t());
    a->m = m;
    a->d = Q.d;
    a->n_utts = n_utts;
    for (int u = 0; u < n_utts; ++u)
        a->n_frames.push_back(Q.utt_off[u + 1] - Q.utt_off[u]);
    a->status.assign((size_t)n_utts, 0);
    a->message.swap(*Q.message);
    a->message.resize((size_t)n_utts);
    a->word_off.assign((size_t)n_utts + 1, 0);
    a->phone_off.assign((size_t)n_utts + 1, 0);
    std::vector<align_piece_t> piece((size_t)n_utts);
    align_phones_t ph;
    align_populate_words(m, Q, piece);
    align_concat_pieces(m->h, Q, piece, a.get(), ph);
    const double t_c = now_ms();
    /* (ssw_align_text_batch with two_pass_history: the scores are made again here, from the
     * history the first pass left, before the second pass reads them) */
    if (Q.between != NULL && Q.between(Q.between_arg) < 0)
        return NULL;
    if (align_second_pass(m, Q, a.get(), ph) < 0)
        return NULL;
    const double t_d = now_ms();
    if (align_propagate(a.get(), m->h->n_emit_state) < 0)
        return NULL;
    if (m->kn.align_timing) /* SSW_ALIGN_TIMING: stderr, ms per stage */
        fprintf(stderr, "ssw_forced_align_batch: first pass %.2f ms, populate %.2f, second pass %.2f, "
                        "propagate %.2f\n", Q.first_ms, t_c - t_b, t_d - t_c, now_ms() - t_d);
    return a.release();
}

/* decoder_alignment's history semantics (src/decoder.c:786-793): the second pass scores again
 * after acmod_rewind, from the top-N order the first pass left (src/ptm_mgau.c:425-448; per
 * utterance here, utterances being independent work items; the s2_semi scorer keeps the same
 * ring of two slots, src/s2_semi_mgau.c:845-855).  Two steps, shared by ssw_align_text_batch and
 * the grammar's recognize_align_rows: the last frame's final order of every utterance is set
 * aside while the first scoring's top-N block is still in the workspace ... */
static int
carry_last_orders(ssw_model_t *m, const char *who, int32_t n_utts, void *stream)
{
    if (carry_rows_reserve(m, n_utts, who) < 0)
        return -1;
    hipLaunchKernelGGL(gather_last_orders_kernel, dim3((unsigned)n_utts), dim3(128), 0,
                       (hipStream_t)stream, m->sw.cw(), m->sw.utt_off(), m->n_cbf,
                       (const uint32_t *)NULL, m->carry_rows.as<uint32_t>());
    if (hipGetLastError() != hipSuccess) {
        ssw_set_error("%s: gather_last_orders_kernel failed to launch", who);
        return -1;
    }
    return 0;
}

/* ... and the scores are made again between the two searches, every utterance from its first
 * pass's history (after carry_last_orders: the request holds the carried rows' address) */
struct rescore_t {
    ssw_model_t *m;
    ScoreReq R;
};
static rescore_t
rescore_request(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                const int32_t *utt_off, int32_t n_utts, int16_t *d_out, void *stream)
{
    rescore_t r = { m, ScoreReq{} };
    r.R.scorer = scorer;
    r.R.d_feats = d_feats;
    r.R.n_frames = n_frames;
    r.R.utt_off = utt_off;
    r.R.n_utts = n_utts;
    r.R.d_out = d_out;
    r.R.stream = stream;
    r.R.d_carry_rows = m->carry_rows.as<uint32_t>();
    return r;
}
static int
rescore_run(void *arg)
{
    const rescore_t *r = static_cast<const rescore_t *>(arg);
    return score_batch_impl(r->m, r->R);
}

extern "C" ssw_alignment_set_t *
ssw_align_text_batch(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                     int scorer, const float *d_feats, int32_t n_frames, const int32_t *utt_off,
                     int32_t n_utts, const int32_t *word_off, const char *const *words,
                     void *stream)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    if (check_has_device(m) < 0)
        return NULL;
    if (n_frames < 0 || (n_frames > 0 && d_feats == NULL)) {
        ssw_set_error("bad arguments to ssw_align_text_batch");
        return NULL;
    }
    if (hipSetDevice(m->device) != hipSuccess)
        return NULL;
    if (text_rows_reserve(m, n_frames, "ssw_align_text_batch") < 0)
        return NULL;
    refresh_knobs(m);
    const bool timing = m->kn.align_timing;
    const double t_in = now_ms();
    int16_t *rows = m->text_scr.as<int16_t>();
    if (n_frames > 0 && ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, rows, stream) < 0)
        return NULL;
    const bool two_pass = cfg != NULL && cfg->two_pass_history
        && (scorer == SSW_SCORER_PTM || scorer == SSW_SCORER_S2_SEMI) && n_frames > 0 && n_utts > 0;
    if (two_pass && carry_last_orders(m, "ssw_align_text_batch", n_utts, stream) < 0)
        return NULL;
    rescore_t rs = rescore_request(m, scorer, d_feats, n_frames, utt_off, n_utts, rows, stream);
    /* the scoring kernels are in flight: the host builds the first pass's graphs meanwhile;
     * the searches then run on the same stream, after the scores */
    checked_texts_t c;
    check_texts(d, n_utts, word_off, words, c);
    ssw_first_pass_plan_t *plan = c.any
        ? ssw_first_pass_prepare(m, d, cfg, n_utts, c.word_off.data(), c.words.data())
        : ssw_first_pass_prepare(m, d, cfg, n_utts, word_off, words);
    if (plan == NULL) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        return NULL;
    }
    ForcedAlignReq F{};
    F.d = d;
    F.plan = plan;
    F.d_senscr = rows;
    F.n_frames = n_frames;
    F.utt_off = utt_off;
    F.n_utts = plan->n_utts;
    F.stream = stream;
    F.reject = c.any ? &c.reject : NULL;
    F.between = two_pass ? rescore_run : NULL;
    F.between_arg = &rs;
    ssw_alignment_set_t *a = forced_align_core(m, F);
    ssw_first_pass_plan_free(plan);
    if (timing)
        fprintf(stderr, "ssw_align_text_batch: %.2f ms in the call\n",
                now_ms() - t_in);
    return a;
}


extern "C" int32_t
ssw_alignment_set_status(const ssw_alignment_set_t *a, int32_t utt)
{
    return (utt >= 0 && utt < a->n_utts) ? a->status[utt] : -1;
}

extern "C" const char *
ssw_alignment_set_message(const ssw_alignment_set_t *a, int32_t utt)
{
    return (utt >= 0 && utt < a->n_utts) ? a->message[utt].c_str() : "";
}

extern "C" int32_t
ssw_alignment_set_words(const ssw_alignment_set_t *a, int32_t utt, const int32_t **wid,
                        const ssw_align_entry_t **al)
{
    if (utt < 0 || utt >= a->n_utts)
        return -1;
    if (wid)
        *wid = a->wid.data() + a->word_off[utt];
    if (al)
        *al = a->word_al.data() + a->word_off[utt];
    return a->word_off[utt + 1] - a->word_off[utt];
}

extern "C" int32_t
ssw_alignment_set_phones(const ssw_alignment_set_t *a, int32_t utt, const int32_t **cipid,
                         const int32_t **parent, const ssw_align_entry_t **al)
{
    if (utt < 0 || utt >= a->n_utts)
        return -1;
    if (cipid)
        *cipid = a->cipid.data() + a->phone_off[utt];
    if (parent)
        *parent = a->parent.data() + a->phone_off[utt];
    if (al)
        *al = a->phone_al.data() + a->phone_off[utt];
    return a->phone_off[utt + 1] - a->phone_off[utt];
}

extern "C" int32_t
ssw_alignment_set_states(const ssw_alignment_set_t *a, int32_t utt, const uint16_t **senid,
                         const ssw_align_entry_t **al)
{
    if (utt < 0 || utt >= a->n_utts)
        return -1;
    const int ne = (int)(a->cipid.empty() ? 3 : a->senid.size() / a->cipid.size());
    if (senid)
        *senid = a->senid.data() + (size_t)a->phone_off[utt] * ne;
    if (al)
        *al = a->state_al.data() + (size_t)a->phone_off[utt] * ne;
    return (a->phone_off[utt + 1] - a->phone_off[utt]) * ne;
}

extern "C" int32_t
ssw_alignment_set_json(const ssw_alignment_set_t *a, int32_t utt, double utt_start, int32_t frate,
                       int32_t align_level, char *out, int32_t out_len)
{
    if (utt < 0 || utt >= a->n_utts || a->status[utt] != 0) {
        ssw_set_error("ssw_alignment_set_json: utterance %d has no alignment", utt);
        return -1;
    }
    const int w0 = a->word_off[utt], nw = a->word_off[utt + 1] - w0;
    const int p0 = a->phone_off[utt], np = a->phone_off[utt + 1] - p0;
    const int ne = (int)(a->cipid.empty() ? 3 : a->senid.size() / a->cipid.size());
    std::vector<const char *> wstr((size_t)nw);
    std::string hyp; /* decoder_hyp: base strings of the non-filler words (src/fsg_search.c:985-1026) */
    for (int i = 0; i < nw; ++i) {
        const int wid = a->wid[w0 + i];
        wstr[i] = ssw_dict_word(a->d, wid);
        if (!ssw_dict_is_filler(a->d, wid)) {
            if (!hyp.empty())
                hyp += ' ';
            hyp += ssw_dict_word(a->d, ssw_dict_base_id(a->d, wid));
        }
    }
    if (!a->hyp.empty()) /* (the grammar's filler marking, not the dictionary's) */
        hyp = a->hyp[(size_t)utt];
    return ssw_alignment_json(a->m, hyp.c_str(), 0, utt_start, frate, a->n_frames[utt] + 1, nw,
                              wstr.data(), a->word_al.data() + w0, np, a->cipid.data() + p0,
                              a->parent.data() + p0, a->phone_al.data() + p0,
                              align_level >= 2 ? a->senid.data() + (size_t)p0 * ne : NULL,
                              align_level >= 2 ? a->state_al.data() + (size_t)p0 * ne : NULL, out,
                              out_len);
}

extern "C" void
ssw_alignment_set_free(ssw_alignment_set_t *a)
{
    delete a;
}
