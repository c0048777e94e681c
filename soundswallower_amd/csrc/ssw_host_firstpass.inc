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

static int first_pass_run(ssw_model_t *m, ssw_fp_graphs_t *g, double fp_t0, const int16_t *d_senscr,
                          int32_t n_frames, const int32_t *utt_off, int32_t n_utts, int32_t max_seg,
                          int32_t *n_seg, ssw_word_seg_t *seg, void *stream,
                          const std::vector<int> *subset = NULL);

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
    const double t0 = now_ms();
    ssw_fp_graphs_t *g = ssw_fp_graphs_build(m, d, cfg, n_utts, word_off, words);
    if (g == NULL)
        return -1;
    const int rc = first_pass_run(m, g, t0, d_senscr, n_frames, utt_off, n_utts, max_seg, n_seg, seg,
                                  stream);
    ssw_fp_graphs_free(g);
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
    const double t0 = now_ms();
    return first_pass_run(m, plan->g, t0, d_senscr, n_frames, utt_off, plan->n_utts, max_seg, n_seg,
                          seg, stream);
}

/* upload the graphs, search, bring the segmentations back; the graphs stay the caller's */
static int
first_pass_run_impl(ssw_model_t *m, ssw_fp_graphs_t *g, double fp_t0, const int16_t *d_senscr,
                    int32_t n_frames, const int32_t *utt_off, int32_t n_utts, int32_t max_seg,
                    int32_t *n_seg, ssw_word_seg_t *seg, void *stream, int level,
                    const std::vector<int> &only);

#define SSW_FP_HIST_BAND 512 /* banded history table: word-final HMMs per frame, on average */
static int
first_pass_run(ssw_model_t *m, ssw_fp_graphs_t *g, double fp_t0, const int16_t *d_senscr,
               int32_t n_frames, const int32_t *utt_off, int32_t n_utts, int32_t max_seg,
               int32_t *n_seg, ssw_word_seg_t *seg, void *stream, const std::vector<int> *subset)
{
    /* long texts, three levels.  2: first_pass_win_kernel (HMMs in registers, a sliding window
     * of nodes, banded history table); 1: first_pass_big_kernel<.., true> (node state in HBM,
     * banded node walk and history table); 0: the same with the full [frame][leaf] table.  An
     * utterance that outgrows a level's window or budget says so (-(1 << 30)) and is searched
     * again one level down -- it alone: the others keep what they have (`only`).
     * SSW_FP_BAND=0: level 0 at once; SSW_FP_WIN=0: never 2. */
    refresh_knobs(m);
    int level = !m->kn.fp_band ? 0 : !m->kn.fp_win ? 1 : 2;
    /* `subset` (the rounds of ssw_first_pass_batch_active): the utterances to search, NULL or
     * empty = all; the others keep what they have */
    std::vector<int> only; /* empty: all of them */
    if (subset != NULL)
        only = *subset;
    for (;;) {
        int rc = first_pass_run_impl(m, g, fp_t0, d_senscr, n_frames, utt_off, n_utts, max_seg,
                                     n_seg, seg, stream, level, only);
        if (rc != 0 || level == 0)
            return rc;
        std::vector<int> left;
        if (only.empty()) {
            for (int u = 0; u < n_utts; ++u)
                if (n_seg[u] == -(1 << 30))
                    left.push_back(u);
        } else {
            for (int u : only)
                if (n_seg[u] == -(1 << 30))
                    left.push_back(u);
        }
        if (left.empty())
            return rc;
        only.swap(left);
        --level;
    }
}

static int
first_pass_run_impl(ssw_model_t *m, ssw_fp_graphs_t *g, double fp_t0, const int16_t *d_senscr,
                    int32_t n_frames, const int32_t *utt_off, int32_t n_utts, int32_t max_seg,
                    int32_t *n_seg, ssw_word_seg_t *seg, void *stream, int level,
                    const std::vector<int> &only)
{
    bool band = level >= 1;
    /* the utterances of this launch: all, or the ones named (their sizes alone pick the kernel
     * and size the workspaces; the others' results stay as they are, on both sides) */
    std::vector<char> runs((size_t)n_utts, only.empty() ? 1 : 0);
    for (int u : only)
        runs[(size_t)u] = 1;
    const int n_run = only.empty() ? n_utts : (int)only.size();
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    hipStream_t st = (hipStream_t)stream;
    (void)n_frames;
    if (n_utts == 0)
        return 0;
    const bool fp_timing = m->kn.align_timing;
    const double fp_t1 = now_ms();
    std::vector<long long> hist_off((size_t)n_utts);
    std::vector<long long> big_off((size_t)n_utts);
    size_t hist_total = 0, lds_ints = 0, max_nodes = 0, big_ints = 0;
    bool big = !strcmp(m->kn.fp_kernel, "big"); /* SSW_FP_KERNEL */
    for (int u = 0; u < n_utts; ++u) { /* which kernel: see below */
        if (!runs[(size_t)u])
            continue;
        const size_t nl = (size_t)(g->leaf_off[u + 1] - g->leaf_off[u]);
        const size_t nn = (size_t)(g->node_off[u + 1] - g->node_off[u]);
        const size_t ns = (size_t)(g->state_off[u + 1] - g->state_off[u]);
        const size_t li = 3 * nn + 4 * nl + 2 * ns + (size_t)(g->tw_off[u + 1] - g->tw_off[u])
            + (size_t)g->tw_rk[u];
        /* beyond one HMM per thread of a 1024-thread workgroup the sliding-window kernel is the
         * faster one (32 texts, ms of first pass, registers / window: 970 HMMs 7.8 / 11.7, 1,167
         * 13.9 / 13.7, 1,564 18.7 / 15.3, 1,961 41 / 23, 2,940 69 / 31, 3,918 109 / 40 -- round 5;
         * the 2- and 4-HMMs-per-thread register instances, the ones that spilt, are gone) */
        big = big || li * sizeof(int) > 160 * 1024 - 512 || nn > 1024;
    }
    band = band && big;
    size_t hist_band = SSW_FP_HIST_BAND;
    {
        /* SSW_FP_HIST_BAND (tests): a budget small enough to overflow */
        if (m->kn.fp_hist_band > 0)
            hist_band = (size_t)m->kn.fp_hist_band;
    }
    for (int u = 0; u < n_utts; ++u) {
        hist_off[u] = (long long)hist_total;
        big_off[u] = (long long)big_ints;
        if (!runs[(size_t)u])
            continue;
        const size_t nl = (size_t)(g->leaf_off[u + 1] - g->leaf_off[u]);
        const size_t nn = (size_t)(g->node_off[u + 1] - g->node_off[u]);
        if (nl * (size_t)(utt_off[u + 1] - utt_off[u]) >= (size_t)INT_MAX) { /* entry ids are int32 */
            ssw_set_error("utterance %d: %zu word-final HMMs x %d frames exceed the history "
                          "table's 2^31 entries", u, nl, utt_off[u + 1] - utt_off[u]);
            return -1;
        }
        /* banded: a budget of SSW_FP_HIST_BAND entries per frame (fewer if the text has fewer
         * word-final HMMs) instead of one per (frame, word-final HMM) */
        hist_total += (band ? std::min(nl, hist_band) : nl)
            * (size_t)(utt_off[u + 1] - utt_off[u]);
        const size_t ns = (size_t)(g->state_off[u + 1] - g->state_off[u]);
        lds_ints = std::max(lds_ints, 3 * nn + 4 * nl + 2 * ns
                                          + (size_t)(g->tw_off[u + 1] - g->tw_off[u])
                                          + (size_t)g->tw_rk[u]);
        max_nodes = std::max(max_nodes, nn);
        big_off[u] = (long long)big_ints; /* first_pass_big_kernel's workspace, see there */
        big_ints += 13 * nn + 5 * nl + 2 * ns + (size_t)(g->tw_off[u + 1] - g->tw_off[u])
            + (size_t)g->tw_rk[u] + 64
            + 2 * (ns + 2) + 2 * (size_t)(utt_off[u + 1] - utt_off[u]) + 2; /* SFIRST LFIRST FBASE FLLO */
    }
    const size_t lds_bytes = lds_ints * sizeof(int);
    int rc = -1;
    /* a text beyond what one workgroup holds in registers and LDS (about 400 words) sends the
     * batch through the kernel that keeps the node state in HBM; SSW_FP_KERNEL=big forces it */
    if (!big)
        big_ints = 0;
    /* one staging buffer -> one copy (WsLayout).  What changes from call to call comes last
     * among the uploaded tables -- the utterance offsets and hist_off excepted, which lie ahead
     * of the graph's: `o_call` is where the graph's tables end */
    const size_t nU = (size_t)n_utts, nN = (size_t)g->n_nodes, nL = (size_t)g->n_leaves;
    WsLayout L;
    const size_t o_utt_off = L.in(utt_off, sizeof(int) * (nU + 1));
    const size_t o_node_off = L.in(g->node_off, sizeof(int) * (nU + 1));
    const size_t o_leaf_off = L.in(g->leaf_off, sizeof(int) * (nU + 1));
    const size_t o_state_off = L.in(g->state_off, sizeof(int) * (nU + 1));
    const size_t o_senid = L.in(g->senid, sizeof(uint16_t) * 4 * nN);
    const size_t o_pen = L.in(g->pen, sizeof(int) * nN);
    const size_t o_parent = L.in(g->parent, sizeof(int) * nN);
    const size_t o_info = L.in(g->info, sizeof(uint32_t) * nN);
    const size_t o_ctxt = L.in(g->ctxt, sizeof(uint64_t) * nN);
    const size_t o_leaf_ord = L.in(g->leaf_ord, sizeof(int) * nN);
    const size_t o_leaf_wid = L.in(g->leaf_wid, sizeof(int) * nL);
    const size_t o_leaf_to = L.in(g->leaf_to, sizeof(int) * nL);
    const size_t o_leaf_node = L.in(g->leaf_node, sizeof(int) * nL);
    const size_t o_in_off = L.in(g->in_off, sizeof(int) * ((size_t)g->n_states + 1));
    const size_t o_in_leaf = L.in(g->in_leaf, sizeof(int) * (size_t)g->n_in);
    const size_t b_hist_off = sizeof(long long) * nU;
    const size_t o_hist_off = L.in(hist_off.data(), b_hist_off);
    const size_t o_tw = L.in(g->tw, sizeof(int) * (size_t)g->n_tw);
    const size_t o_tw_off = L.in(g->tw_off, sizeof(int) * (nU + 1));
    const size_t o_twin_ref = L.in(g->twin_ref, sizeof(int) * nN);
    const size_t o_tw_rk = L.in(g->tw_rk, sizeof(int) * nU);
    const size_t o_call = L.mark();
    const size_t o_big_off = L.in(big_off.data(), sizeof(long long) * nU);
    const size_t o_only = L.in(only.data(), sizeof(int) * only.size());
    const size_t in_bytes = L.in_bytes();
    const size_t out_off = L.out(sizeof(int) * nU);
    const size_t seg_off = L.out(sizeof(ssw_word_seg_t) * nU * (size_t)max_seg);
    const size_t hist_at = L.out(sizeof(int2) * (hist_total ? hist_total : 1));
    const size_t big_at = L.out(sizeof(int) * big_ints);

    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess) {
        bool moved = false;
        const int got = devbuf_reserve(m->fp_ws, L.size(), "ssw_first_pass_batch", L.size() / 4, &moved);
        if (moved) /* the cached graphs went with the old buffer */
            m->fp_ws_uid = 0;
        if (got < 0)
            return -1;
    }
    /* The same graphs searched again (the rounds of ssw_first_pass_batch_active, a level's
     * leftovers, a plan run on several recordings): their tables are on the device already --
     * what changes from call to call comes last in the layout (the utterance offsets excepted:
     * a plan's texts meet new recordings) and is all that goes up: utt_off, hist_off, big_off,
     * only.  Keyed by the graphs' uid, not their address. */
    const bool cached = m->fp_ws_uid != 0 && m->fp_ws_uid == g->uid
        && m->fp_ws_uid_bytes == o_call;
    const size_t up_from = cached ? o_call : 0; /* big_off | only */
    std::vector<unsigned char> stage(in_bytes - up_from + 1);
    std::vector<int> all_n;
    std::vector<ssw_word_seg_t> all_seg;
    if (e == hipSuccess) {
        L.fill(stage.data(), up_from);
        /* the graphs go up on a stream of their own: whatever the caller's stream still has
         * to do (ssw_align_text_batch: the scoring kernels) does not hold the copy back; the
         * search then waits for both */
        if (m->s_up == NULL) {
            e = hipStreamCreateWithFlags(&m->s_up, hipStreamNonBlocking);
            if (e == hipSuccess)
                e = hipEventCreateWithFlags(&m->ev_up, hipEventDisableTiming);
        }
        if (e == hipSuccess && in_bytes > up_from)
            e = hipMemcpyAsync(m->fp_ws.p + up_from, stage.data(), in_bytes - up_from,
                               hipMemcpyHostToDevice, m->s_up);
        if (e == hipSuccess && cached) {
            /* the two small tables ahead of the graph's that a call may change */
            e = hipMemcpyAsync(m->fp_ws.p + o_utt_off, utt_off, sizeof(int) * (nU + 1),
                               hipMemcpyHostToDevice, m->s_up);
            if (e == hipSuccess)
                e = hipMemcpyAsync(m->fp_ws.p + o_hist_off, hist_off.data(), b_hist_off,
                                   hipMemcpyHostToDevice, m->s_up);
        }
        if (e == hipSuccess) {
            m->fp_ws_uid = g->uid;
            m->fp_ws_uid_bytes = o_call;
        } else
            m->fp_ws_uid = 0;
        if (e == hipSuccess)
            e = hipEventRecord(m->ev_up, m->s_up);
        if (e == hipSuccess)
            e = hipStreamWaitEvent(st, m->ev_up, 0);
    }
    if (e == hipSuccess) {
        unsigned char *ws = m->fp_ws.p;
        FirstPassParams P;
        P.senscr = d_senscr;
        P.utt_off = ws_at<const int>(ws, o_utt_off);
        P.node_off = ws_at<const int>(ws, o_node_off);
        P.leaf_off = ws_at<const int>(ws, o_leaf_off);
        P.state_off = ws_at<const int>(ws, o_state_off);
        P.senid = ws_at<const uint16_t>(ws, o_senid);
        P.pen = ws_at<const int>(ws, o_pen);
        P.parent = ws_at<const int>(ws, o_parent);
        P.info = ws_at<const uint32_t>(ws, o_info);
        P.ctxt = ws_at<const unsigned long long>(ws, o_ctxt);
        P.leaf_ord = ws_at<const int>(ws, o_leaf_ord);
        P.leaf_wid = ws_at<const int>(ws, o_leaf_wid);
        P.leaf_to = ws_at<const int>(ws, o_leaf_to);
        P.leaf_node = ws_at<const int>(ws, o_leaf_node);
        P.in_off = ws_at<const int>(ws, o_in_off);
        P.in_leaf = ws_at<const int>(ws, o_in_leaf);
        P.hist_off = ws_at<const long long>(ws, o_hist_off);
        P.tw = ws_at<const int>(ws, o_tw);
        P.tw_off = ws_at<const int>(ws, o_tw_off);
        P.twin_ref = ws_at<const int>(ws, o_twin_ref);
        P.tw_rk = ws_at<const int>(ws, o_tw_rk);
        P.big_off = ws_at<const long long>(ws, o_big_off);
        P.only = only.empty() ? NULL : ws_at<const int>(ws, o_only);
        P.big_ws = ws_at<int>(ws, big_at);
        P.tp = (const uint32_t *)m->d_tp;
        P.hist = ws_at<int2>(ws, hist_at);
        P.n_seg = ws_at<int>(ws, out_off);
        P.seg = ws_at<ssw_word_seg_t>(ws, seg_off);
        P.n_sen = m->h->n_sen;
        P.max_seg = max_seg;
        P.beam = g->beam;
        P.pbeam = g->pbeam;
        P.wbeam = g->wbeam;
        P.sil = m->h->sil;
        /* one thread per HMM while a workgroup can hold them (1024 threads), then the long-text kernels */
        void (*kern)(FirstPassParams);
        int tpb;
        size_t lds_launch = lds_bytes;
        P.hist_band = (int)hist_band;
        P.act_mask = m->fpa_mask;
        P.act_off = m->fpa_act_off;
        const bool exp = m->fpa_mask != NULL;
        if (big) {
            /* banded: a frame walks a few hundred nodes, so a small workgroup (cheaper barriers
             * and reductions) is the faster one; SSW_FP_BIG_TPB = 256 / 512 / 1024 (tuning) */
            const int want = m->kn.fp_big_tpb;
            kern = first_pass_big_kernel<1024, false>;
            tpb = 1024;
            if (band && level == 2) {
                /* window of 512 nodes unless told otherwise (256 / 512 / 1024) */
                const int wt = m->kn.fp_win_tpb;
                kern = wt >= 1024 ? first_pass_win_kernel<1024>
                    : wt >= 512   ? first_pass_win_kernel<512>
                                  : first_pass_win_kernel<256>;
                tpb = wt >= 1024 ? 1024 : wt >= 512 ? 512 : 256;
            } else if (band) {
                kern = want == 1024 ? first_pass_big_kernel<1024, true>
                    : want == 512   ? first_pass_big_kernel<512, true>
                                    : first_pass_big_kernel<256, true>;
                tpb = want == 1024 ? 1024 : want == 512 ? 512 : 256;
            }
            lds_launch = 0;
        } else if (max_nodes <= 256) {
            kern = exp ? first_pass_kernel<256, true> : first_pass_kernel<256>;
            tpb = 256;
        } else if (max_nodes <= 512) {
            kern = exp ? first_pass_kernel<512, true> : first_pass_kernel<512>;
            tpb = 512;
        } else { /* (more than 1024 nodes: `big` above) */
            kern = exp ? first_pass_kernel<1024, true> : first_pass_kernel<1024>;
            tpb = 1024;
        }
        if (lds_launch > 48 * 1024)
            e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_launch);
        if (e == hipSuccess && exp && big) {
            /* the long-text kernels export only the words that hold an active HMM */
            hipLaunchKernelGGL(fpa_clear_kernel, dim3(n_run), dim3(256), 0, st, P.act_mask, P.act_off,
                               P.utt_off, m->fpa_node_cnt, P.only);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(kern, dim3(n_run), dim3(tpb), lds_launch, st, P);
            e = hipGetLastError();
        }
        if (e == hipSuccess && only.empty())
            e = hipMemcpyAsync(n_seg, ws + out_off, sizeof(int) * (size_t)n_utts,
                               hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && only.empty())
            e = hipMemcpyAsync(seg, ws + seg_off, sizeof(ssw_word_seg_t) * (size_t)n_utts * max_seg,
                               hipMemcpyDeviceToHost, st);
        /* a level's leftovers: their rows alone come back -- copied one by one when they are
         * few, picked out of one copy of the whole arrays otherwise (round 6: 256 utterances run
         * again cost 512 small copies, 7 ms) */
        if (only.size() > 8 && e == hipSuccess) {
            all_n.resize((size_t)n_utts);
            all_seg.resize((size_t)n_utts * (size_t)max_seg);
            e = hipMemcpyAsync(all_n.data(), ws + out_off, sizeof(int) * (size_t)n_utts,
                               hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(all_seg.data(), ws + seg_off,
                                   sizeof(ssw_word_seg_t) * (size_t)n_utts * max_seg,
                                   hipMemcpyDeviceToHost, st);
        } else
        for (size_t i = 0; i < only.size() && e == hipSuccess; ++i) {
            const size_t u = (size_t)only[i];
            e = hipMemcpyAsync(n_seg + u, ws + out_off + sizeof(int) * u, sizeof(int),
                               hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(seg + u * (size_t)max_seg,
                                   ws + seg_off + sizeof(ssw_word_seg_t) * u * (size_t)max_seg,
                                   sizeof(ssw_word_seg_t) * (size_t)max_seg, hipMemcpyDeviceToHost, st);
        }
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e == hipSuccess && !all_n.empty())
        for (int u : only) {
            n_seg[u] = all_n[(size_t)u];
            memcpy(seg + (size_t)u * max_seg, all_seg.data() + (size_t)u * max_seg,
                   sizeof(ssw_word_seg_t) * (size_t)max_seg);
        }
    if (e != hipSuccess) {
        /* `stage` goes out of scope below: the upload stream must be done with it first (on the
         * success path the wait on ev_up and the synchronise above cover that) */
        if (m->s_up != NULL)
            (void)hipStreamSynchronize(m->s_up);
        ssw_set_error("ssw_first_pass_batch: %s", hipGetErrorString(e));
    } else
        rc = 0;
    if (fp_timing)
        fprintf(stderr, "ssw_first_pass_batch: graphs %.2f ms (%d HMMs), upload + search + results "
                        "%.2f ms\n", fp_t1 - fp_t0, g->n_nodes, now_ms() - fp_t1);
    return rc;
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
static int first_pass_active_run(ssw_model_t *m, ssw_fp_graphs_t *g, int scorer, const float *d_feats,
                                 int32_t n_frames, const int32_t *utt_off, int32_t n_utts,
                                 int32_t max_seg, int32_t *n_seg, ssw_word_seg_t *seg,
                                 int16_t *d_rows, bool full_rows, uint32_t *seed_out,
                                 int32_t *rounds_out, void *stream, uint32_t *d_carry_out = NULL);
static ssw_alignment_set_t *forced_align_core(ssw_model_t *m, const ssw_dict_t *d,
                                              const ssw_first_pass_config_t *cfg,
                                              const ssw_first_pass_plan_t *plan,
                                              const int16_t *d_senscr, int32_t n_frames,
                                              const int32_t *utt_off, int32_t n_utts,
                                              const int32_t *word_off, const char *const *words,
                                              void *stream,
                                              const std::vector<std::string> *reject = NULL,
                                              int (*between)(void *) = NULL, void *between_arg = NULL,
                                              const fpa_mode_t *fpa = NULL);

/* decoder_alignment from alignment_add_word on (src/decoder.c:765-797), for a batch whose word
 * windows are known: forced_align_core's second half, and what follows a grammar search
 * (ssw_host_grammar.inc).  Utterance u has n_seg[u] words at seg + u * max_seg; n_seg[u] < 0: none,
 * reported with status pre_status[u] (NULL: 1) and message[u].  fpa: the default configuration,
 * with `seed` (host [n_utts][(n_sen + 31) / 32]) and d_carry (NULL, or device [n_utts][n_cbf]);
 * else the second pass reads d_senscr.  between: NULL, or called once before the second pass.
 * first_ms: for SSW_ALIGN_TIMING's line, the time the caller's first pass took. */
static ssw_alignment_set_t *align_word_segments(ssw_model_t *m, const ssw_dict_t *d,
                                                const int16_t *d_senscr, const int32_t *utt_off,
                                                int32_t n_utts, const int32_t *n_seg,
                                                const ssw_word_seg_t *seg, int32_t max_seg,
                                                const int32_t *pre_status,
                                                std::vector<std::string> &message,
                                                const fpa_mode_t *fpa, const uint32_t *seed,
                                                const uint32_t *d_carry, int (*between)(void *),
                                                void *between_arg, void *stream, double first_ms);

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
    if (c.any)
        return forced_align_core(m, d, cfg, NULL, d_senscr, n_frames, utt_off, n_utts,
                                 c.word_off.data(), c.words.data(), stream, &c.reject);
    return forced_align_core(m, d, cfg, NULL, d_senscr, n_frames, utt_off, n_utts, word_off, words,
                             stream);
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
    return forced_align_core(m, d, NULL, plan, d_senscr, n_frames, utt_off, plan->n_utts, NULL, NULL,
                             stream);
}

static ssw_alignment_set_t *
forced_align_core(ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                  const ssw_first_pass_plan_t *plan, const int16_t *d_senscr, int32_t n_frames,
                  const int32_t *utt_off, int32_t n_utts, const int32_t *word_off,
                  const char *const *words, void *stream, const std::vector<std::string> *reject,
                  int (*between)(void *), void *between_arg, const fpa_mode_t *fpa)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    const ssw_host_model_t *h = m->h;
    refresh_knobs(m);
    const double t_a = now_ms();
    int max_words = plan ? plan->max_words : 0;
    for (int u = 0; !plan && u < n_utts; ++u)
        max_words = std::max(max_words, word_off[u + 1] - word_off[u]);
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
            own_plan = ssw_first_pass_prepare(m, d, cfg, n_utts, word_off, words);
            if (own_plan == NULL)
                return NULL;
        }
        const ssw_first_pass_plan_t *use = plan ? plan : own_plan;
        const int rc = fpa != NULL
            ? first_pass_active_run(m, use->g, fpa->scorer, fpa->d_feats, n_frames, utt_off, n_utts,
                                    max_seg, n_seg.data(), seg.data(),
                                    const_cast<int16_t *>(d_senscr), false, seed.data(), NULL, stream,
                                    carry2 ? m->carry_rows.as<uint32_t>() : NULL)
            : use ? ssw_first_pass_run(m, use, d_senscr, n_frames, utt_off, max_seg,
                                                n_seg.data(), seg.data(), stream)
                           : ssw_first_pass_batch(m, d, cfg, d_senscr, n_frames, utt_off, n_utts,
                                                  word_off, words, max_seg, n_seg.data(),
                                                  seg.data(), stream);
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
    if (reject != NULL) /* these were searched as empty texts: no alignment for them */
        for (int u = 0; u < n_utts; ++u)
            if (!(*reject)[u].empty()) {
                message[u] = (*reject)[u];
                pre_status[u] = 3;
                n_seg[u] = -1;
            }
    return align_word_segments(m, d, d_senscr, utt_off, n_utts, n_seg.data(), seg.data(), max_seg,
                               pre_status.data(), message, fpa, seed.data(),
                               carry2 ? m->carry_rows.as<uint32_t>() : NULL, between, between_arg,
                               stream, now_ms() - t_a);
}

static ssw_alignment_set_t *
align_word_segments(ssw_model_t *m, const ssw_dict_t *d, const int16_t *d_senscr,
                    const int32_t *utt_off, int32_t n_utts, const int32_t *n_seg,
                    const ssw_word_seg_t *seg, int32_t max_seg, const int32_t *pre_status,
                    std::vector<std::string> &message, const fpa_mode_t *fpa, const uint32_t *seed,
                    const uint32_t *d_carry, int (*between)(void *), void *between_arg, void *stream,
                    double first_ms)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    const ssw_host_model_t *h = m->h;
    refresh_knobs(m);
    const bool timing = m->kn.align_timing; /* SSW_ALIGN_TIMING: stderr, ms per stage */
    const size_t nw32 = ((size_t)h->n_sen + 31) / 32;
    double t_b = now_ms(), t_c, t_d;
    ssw_alignment_set_t *a = new ssw_alignment_set_t();
    a->m = m;
    a->d = d;
    a->n_utts = n_utts;
    for (int u = 0; u < n_utts; ++u)
        a->n_frames.push_back(utt_off[u + 1] - utt_off[u]);
    a->status.assign((size_t)n_utts, 0);
    a->message.swap(message);
    a->message.resize((size_t)n_utts);
    a->word_off.assign((size_t)n_utts + 1, 0);
    a->phone_off.assign((size_t)n_utts + 1, 0);
    /* alignment_add_word + alignment_populate per utterance, with the first pass's windows;
     * utterances are independent, so a few host threads share them (populate is 150 triphone
     * look-ups per utterance) and the pieces are concatenated afterwards */
    std::vector<int32_t> ssid, tmat32, start, dur;
    const int max_ph = 0xffff / std::max(1, h->n_emit_state);
    struct piece_t {
        int np = -1;
        std::vector<int32_t> ssid, tmat, ci, par, st, du;
    };
    std::vector<piece_t> piece((size_t)n_utts);
    auto populate_range = [&](int u0, int u1) {
        std::vector<const char *> wstr;
        std::vector<int32_t> wstart, wdur, t_ssid((size_t)max_ph), t_tmat((size_t)max_ph),
            t_ci((size_t)max_ph), t_par((size_t)max_ph), t_st((size_t)max_ph), t_du((size_t)max_ph);
        for (int u = u0; u < u1; ++u) {
            if (n_seg[u] < 0)
                continue;
            const ssw_word_seg_t *sg = seg + (size_t)u * max_seg;
            wstr.clear();
            wstart.clear();
            wdur.clear();
            for (int i = 0; i < n_seg[u]; ++i) {
                wstr.push_back(ssw_dict_word(d, sg[i].wid));
                wstart.push_back(sg[i].start);
                wdur.push_back(sg[i].duration);
            }
            piece_t &pc = piece[u];
            pc.np = ssw_alignment_populate(m, d, n_seg[u], wstr.data(), wstart.data(), wdur.data(),
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
    {
        const int n_thr = std::min(std::min(ssw_host_threads(), 32), n_utts / 16);
        if (n_thr < 2)
            populate_range(0, n_utts);
        else {
            struct job_t {
                decltype(populate_range) *fn;
                int n_utts, n_thr;
            } job = { &populate_range, n_utts, n_thr };
            ssw_parallel_for(n_thr, [](void *arg, int t) {
                const job_t *j = static_cast<const job_t *>(arg);
                (*j->fn)((int)((long long)j->n_utts * t / j->n_thr),
                         (int)((long long)j->n_utts * (t + 1) / j->n_thr));
            }, &job);
        }
    }
    for (int u = 0; u < n_utts; ++u) {
        a->word_off[u] = (int32_t)a->wid.size();
        a->phone_off[u] = (int32_t)a->cipid.size();
        if (n_seg[u] < 0) {
            a->status[u] = pre_status != NULL ? pre_status[u] : 1;
            continue;
        }
        const piece_t &pc = piece[u];
        if (pc.np < 0) {
            a->status[u] = 2;
            continue;
        }
        const ssw_word_seg_t *sg = seg + (size_t)u * max_seg;
        for (int i = 0; i < n_seg[u]; ++i)
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
    std::vector<int16_t> tmat(n_ph);
    std::vector<int32_t> sf(n_ph), ef(n_ph);
    for (size_t i = 0; i < n_ph; ++i) {
        for (int j = 0; j < ne; ++j) {
            a->senid[i * ne + j] = h->sseq[(size_t)ssid[i] * ne + j];
            /* what alignment_populate leaves in the state entries (src/ps_alignment.c:237-239) */
            a->state_al[i * ne + j].start = start[i];
            a->state_al[i * ne + j].duration = dur[i];
        }
        tmat[i] = (int16_t)tmat32[i];
        sf[i] = start[i] > 0 ? start[i] : 0; /* state_align_search_init, :464-471 */
        ef[i] = dur[i] > 0 ? start[i] + dur[i] : INT_MAX;
    }
    t_c = now_ms();
    /* (ssw_align_text_batch with two_pass_history: the scores are made again here, from the
     * history the first pass left, before the second pass reads them) */
    if (between != NULL && between(between_arg) < 0) {
        delete a;
        return NULL;
    }
    /* the second pass over every run of consecutive utterances that got through the first */
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
        const int rc2 = fpa != NULL
            ? align_batch_active_impl(m, fpa->scorer,
                                      fpa->d_feats + (size_t)utt_off[u0] * h->veclen_total, u1 - u0,
                                      foff.data(), poff.data(), a->senid.data() + p0 * ne,
                                      tmat.data() + p0, sf.data() + p0, ef.data() + p0,
                                      seed + (size_t)u0 * nw32, a->state_al.data() + p0 * ne,
                                      st.data(), NULL, stream,
                                      d_carry != NULL ? d_carry + (size_t)u0 * m->n_cbf : NULL)
            : ssw_align_batch(m, d_senscr + (size_t)utt_off[u0] * h->n_sen, u1 - u0, foff.data(),
                              poff.data(), a->senid.data() + p0 * ne, tmat.data() + p0,
                              sf.data() + p0, ef.data() + p0, a->state_al.data() + p0 * ne,
                              st.data(), stream);
        if (rc2 < 0) {
            delete a;
            return NULL;
        }
        for (int u = u0; u < u1; ++u)
            if (st[u - u0] != 0)
                a->status[u] = 2;
        u0 = u1;
    }
    t_d = now_ms();
    /* alignment_propagate: states -> phones -> words, the utterances shared out over the host
     * threads (one after the other they took 0.28 ms per 256 utterances, as long as a fifth of
     * the second pass's kernel) */
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
        const int n_thr = std::min(std::min(ssw_host_threads(), 32), n_utts / 16);
        if (n_thr < 2)
            propagate_range(0, n_utts);
        else {
            struct job_t {
                decltype(propagate_range) *fn;
                int n_utts, n_thr;
            } job = { &propagate_range, n_utts, n_thr };
            ssw_parallel_for(n_thr, [](void *arg, int t) {
                const job_t *j = static_cast<const job_t *>(arg);
                (*j->fn)((int)((long long)j->n_utts * t / j->n_thr),
                         (int)((long long)j->n_utts * (t + 1) / j->n_thr));
            }, &job);
        }
        if (failed.load()) {
            delete a;
            return NULL;
        }
    }
    if (timing)
        fprintf(stderr, "ssw_forced_align_batch: first pass %.2f ms, populate %.2f, second pass %.2f, "
                        "propagate %.2f\n", first_ms, t_c - t_b, t_d - t_c, now_ms() - t_d);
    return a;
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
    if (n_frames > 0
        && ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, m->text_scr.as<int16_t>(), stream) < 0)
        return NULL;
    /* decoder_alignment's history semantics (src/decoder.c:786-793): the second pass scores
     * again after acmod_rewind, from the top-N order the first pass left (src/ptm_mgau.c:425-448;
     * per utterance here, utterances being independent work items).  The last frame's final
     * order of every utterance is set aside now, while the first pass's top-N block is still in
     * the workspace; the scores are made again between the two searches. */
    struct rescore_t {
        ssw_model_t *m;
        const float *d_feats;
        int32_t n_frames, n_utts;
        const int32_t *utt_off;
        void *stream;
        int scorer;
    } rs = { m, d_feats, n_frames, n_utts, utt_off, stream, scorer };
    /* (the s2_semi scorer keeps the same ring of two slots, src/s2_semi_mgau.c:845-855) */
    const bool two_pass = cfg != NULL && cfg->two_pass_history
        && (scorer == SSW_SCORER_PTM || scorer == SSW_SCORER_S2_SEMI) && n_frames > 0 && n_utts > 0;
    if (two_pass) {
        if (carry_rows_reserve(m, n_utts, "ssw_align_text_batch") < 0)
            return NULL;
        hipLaunchKernelGGL(gather_last_orders_kernel, dim3((unsigned)n_utts), dim3(128), 0,
                           (hipStream_t)stream, m->sw.cw(), m->sw.utt_off(), m->n_cbf,
                           (const uint32_t *)NULL, m->carry_rows.as<uint32_t>());
        if (hipGetLastError() != hipSuccess) {
            ssw_set_error("ssw_align_text_batch: gather_last_orders_kernel failed to launch");
            return NULL;
        }
    }
    auto rescore = [](void *arg) -> int {
        rescore_t *r = static_cast<rescore_t *>(arg);
        ScoreReq R{};
        R.scorer = r->scorer;
        R.d_feats = r->d_feats;
        R.n_frames = r->n_frames;
        R.utt_off = r->utt_off;
        R.n_utts = r->n_utts;
        R.d_out = r->m->text_scr.as<int16_t>();
        R.stream = r->stream;
        R.d_carry_rows = r->m->carry_rows.as<uint32_t>();
        return score_batch_impl(r->m, R);
    };
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
    ssw_alignment_set_t *a = forced_align_core(m, d, NULL, plan, m->text_scr.as<int16_t>(), n_frames, utt_off,
                                               plan->n_utts, NULL, NULL, stream,
                                               c.any ? &c.reject : NULL,
                                               two_pass ? +rescore : NULL, &rs);
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
