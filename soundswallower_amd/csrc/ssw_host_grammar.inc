/* ssw_host_grammar.inc -- host: ssw_grammar_prepare(_large, _large_active), ssw_grammar_search_batch,
 * ssw_recognize_batch, ssw_recognize_batch_active, the recognition set, and decoder_alignment of
 * what was recognised: ssw_recognition_set_align, ssw_recognize_align_batch(_active).
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* recognition against word FSGs (decoder_set_fsg; ssw_k9_grammar.inc)                  */
/* ---------------------------------------------------------------------------------- */
struct ssw_grammar_plan_s {
    ssw_fp_graphs_t *g;
    int32_t n_fsgs;
    size_t lds_ints; /* the largest grammar's exchange arrays */
    int32_t max_nodes;
    /* ssw_grammar_prepare_large: a grammar beyond one workgroup's registers or LDS puts the whole
     * plan on grammar_search_big_kernel; the first such grammar, for the refusals that name it */
    bool big;
    int32_t big_fsg, big_nodes;
    std::string big_name;
    /* ssw_grammar_prepare_large_active: ssw_recognize_batch_active takes the plan when it is big
     * (the exporting instance of grammar_search_big_kernel); nothing else looks at it */
    bool active;
};

/* LDS ints of one grammar's exchange arrays: XS XH FLG [N] | EXJ IL[3] LS[2] per slot | TW |
 * RK | SMAX [2 NS] (grammar_search_kernel) */
static size_t
grammar_lds_ints(const ssw_fp_graphs_t *g, int u)
{
    const size_t nn = (size_t)(g->node_off[u + 1] - g->node_off[u]);
    const size_t ns = (size_t)(g->state_off[u + 1] - g->state_off[u]);
    const size_t ne = (size_t)(g->slot_off[g->state_off[u + 1]] - g->slot_off[g->state_off[u]]);
    return 3 * nn + 6 * ne + 2 * ns + (size_t)(g->tw_off[u + 1] - g->tw_off[u]) + (size_t)g->tw_rk[u];
}

#define SSW_GRAMMAR_LDS_BYTES (160 * 1024 - 512)

/* ints of one utterance's workspace on grammar_search_big_kernel (layout: see there) */
static size_t
grammar_big_ws_ints(const ssw_fp_graphs_t *g, int u)
{
    const size_t nn = (size_t)(g->node_off[u + 1] - g->node_off[u]);
    const size_t ns = (size_t)(g->state_off[u + 1] - g->state_off[u]);
    const size_t ne = (size_t)(g->slot_off[g->state_off[u + 1]] - g->slot_off[g->state_off[u]]);
    const size_t ntw = (size_t)(g->tw_off[u + 1] - g->tw_off[u]);
    return 13 * nn + 9 * ne + ntw + (size_t)g->tw_rk[u] + 2 * ns + ntw / 4 + 1;
}

/* max_hmms < 0: ssw_grammar_prepare, every grammar within one workgroup; `active`:
 * ssw_grammar_prepare_large_active */
static ssw_grammar_plan_t *
grammar_prepare(const ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                int32_t n_fsgs, const ssw_fsg_t *const *fsgs, int32_t max_hmms, bool active)
{
    const bool large = max_hmms >= 0;
    if (m == NULL || d == NULL || n_fsgs < 1 || fsgs == NULL || (large && max_hmms < 1)) {
        ssw_set_error("bad arguments to %s", active ? "ssw_grammar_prepare_large_active"
                      : large ? "ssw_grammar_prepare_large" : "ssw_grammar_prepare");
        return NULL;
    }
    if (large && max_hmms > SSW_GRAMMAR_LARGE_MAX_HMMS) {
        ssw_set_error("max_hmms = %d: the grammar search handles at most %d phone-tree HMMs per "
                      "grammar (the reference narrows its beams beyond its maxhmmpf)", max_hmms,
                      SSW_GRAMMAR_LARGE_MAX_HMMS);
        return NULL;
    }
    /* built on the calling thread, one grammar after the other (a plan's grammars are few next
     * to a batch of texts); no device call: another host thread may prepare the next plan while
     * the GPU searches this one */
    ssw_fp_graphs_t *g = ssw_grammar_graphs_build(m, d, cfg, n_fsgs, fsgs);
    if (g == NULL)
        return NULL;
    size_t lds = 0;
    int32_t max_nodes = 0;
    ssw_grammar_plan_t *p = new ssw_grammar_plan_t();
    p->big = false;
    p->big_fsg = -1;
    p->big_nodes = 0;
    p->active = active;
    for (int u = 0; u < n_fsgs; ++u) {
        const int nn = g->node_off[u + 1] - g->node_off[u];
        const size_t li = grammar_lds_ints(g, u);
        if (large) {
            if (nn > max_hmms) {
                ssw_set_error("grammar %d (%s) has %d phone-tree HMMs: max_hmms allows at most %d",
                              u, ssw_fsg_name(fsgs[u]), nn, max_hmms);
                ssw_fp_graphs_free(g);
                delete p;
                return NULL;
            }
            if (!p->big && (nn > SSW_GRAMMAR_MAX_HMMS || li * sizeof(int) > SSW_GRAMMAR_LDS_BYTES)) {
                p->big = true;
                p->big_fsg = u;
                p->big_nodes = nn;
                p->big_name = ssw_fsg_name(fsgs[u]);
            }
            if (nn <= SSW_GRAMMAR_MAX_HMMS && li * sizeof(int) <= SSW_GRAMMAR_LDS_BYTES) {
                lds = std::max(lds, li);
                max_nodes = std::max(max_nodes, nn);
            }
            continue;
        }
        if (nn > SSW_GRAMMAR_MAX_HMMS) {
            ssw_set_error("grammar %d (%s) has %d phone-tree HMMs: the grammar search holds at "
                          "most %d in one workgroup", u, ssw_fsg_name(fsgs[u]), nn,
                          SSW_GRAMMAR_MAX_HMMS);
            ssw_fp_graphs_free(g);
            delete p;
            return NULL;
        }
        if (li * sizeof(int) > SSW_GRAMMAR_LDS_BYTES) {
            ssw_set_error("grammar %d (%s): %d phone-tree HMMs and %d entering-list entries need "
                          "%zu bytes of exchange arrays: the workgroup's LDS holds at most %d",
                          u, ssw_fsg_name(fsgs[u]), nn,
                          g->slot_off[g->state_off[u + 1]] - g->slot_off[g->state_off[u]],
                          li * sizeof(int), (int)SSW_GRAMMAR_LDS_BYTES);
            ssw_fp_graphs_free(g);
            delete p;
            return NULL;
        }
        lds = std::max(lds, li);
        max_nodes = std::max(max_nodes, nn);
    }
    p->g = g;
    p->n_fsgs = n_fsgs;
    p->lds_ints = lds;
    p->max_nodes = max_nodes;
    return p;
}

extern "C" ssw_grammar_plan_t *
ssw_grammar_prepare(const ssw_model_t *m, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
                    int32_t n_fsgs, const ssw_fsg_t *const *fsgs)
{
    return grammar_prepare(m, d, cfg, n_fsgs, fsgs, -1, false);
}

extern "C" ssw_grammar_plan_t *
ssw_grammar_prepare_large(const ssw_model_t *m, const ssw_dict_t *d,
                          const ssw_first_pass_config_t *cfg, int32_t n_fsgs,
                          const ssw_fsg_t *const *fsgs, int32_t max_hmms)
{
    if (max_hmms < 0)
        max_hmms = 0; /* (refused as a bad argument) */
    return grammar_prepare(m, d, cfg, n_fsgs, fsgs, max_hmms, false);
}

extern "C" ssw_grammar_plan_t *
ssw_grammar_prepare_large_active(const ssw_model_t *m, const ssw_dict_t *d,
                                 const ssw_first_pass_config_t *cfg, int32_t n_fsgs,
                                 const ssw_fsg_t *const *fsgs, int32_t max_hmms)
{
    if (max_hmms < 0)
        max_hmms = 0; /* (refused as a bad argument) */
    return grammar_prepare(m, d, cfg, n_fsgs, fsgs, max_hmms, true);
}

extern "C" int32_t
ssw_grammar_plan_active(const ssw_grammar_plan_t *p)
{
    return p == NULL ? -1 : p->active ? 1 : 0;
}

extern "C" void
ssw_grammar_plan_free(ssw_grammar_plan_t *p)
{
    if (p == NULL)
        return;
    ssw_fp_graphs_free(p->g);
    delete p;
}

extern "C" int32_t
ssw_grammar_plan_hmms(const ssw_grammar_plan_t *p, int32_t fsg)
{
    if (p == NULL || fsg < 0 || fsg >= p->n_fsgs)
        return -1;
    return p->g->node_off[fsg + 1] - p->g->node_off[fsg];
}

struct ssw_recognition_set_s {
    const ssw_model_t *m;
    const ssw_dict_t *d;
    int32_t n_utts;
    std::vector<int32_t> n_frames, status, score, seg_off, n_seg;
    std::vector<std::string> message, hyp;
    std::vector<char> has_hyp;
    std::vector<ssw_fsg_seg_t> seg;
};

static size_t
grammar_hist_budget()
{
    const char *e = getenv("SSW_GRAMMAR_HIST_MB");
    if (e != NULL && atoll(e) > 0)
        return (size_t)atoll(e) << 20;
    return SSW_GRAMMAR_HIST_BYTES;
}

/* The history tables of a call: (frames + 1) rows of one entry per slot, per utterance.
 * hist_off[u]: the utterance's first entry within its group's table; group: the first utterance
 * of every group, then n_utts; *hist_cap: the entries of the largest group.  A plan on the
 * one-workgroup kernels is one group, refused when it exceeds the budget; a plan on
 * grammar_search_big_kernel starts another group where the budget is reached (the groups are
 * searched one after the other in the same table), and refuses an utterance that exceeds it alone. */
static int
grammar_history_layout(const ssw_grammar_plan_t *plan, const int32_t *fsg_of_utt,
                       const int32_t *utt_off, int32_t n_utts, std::vector<long long> &hist_off,
                       std::vector<int> &group, size_t *hist_cap, int *max_seg)
{
    const ssw_fp_graphs_t *g = plan->g;
    const size_t budget = grammar_hist_budget();
    size_t hist_total = 0, sum = 0;
    hist_off.assign((size_t)n_utts + 1, 0);
    group.assign(1, 0);
    *hist_cap = 0;
    *max_seg = 1;
    for (int u = 0; u < n_utts; ++u) {
        const int gi = fsg_of_utt ? fsg_of_utt[u] : 0;
        if (gi < 0 || gi >= plan->n_fsgs) {
            ssw_set_error("utterance %d: grammar %d is not one of the plan's %d", u, gi, plan->n_fsgs);
            return -1;
        }
        const int T = utt_off[u + 1] - utt_off[u];
        if (T < 0) {
            ssw_set_error("bad arguments to ssw_grammar_search_batch");
            return -1;
        }
        const size_t ne = (size_t)(g->slot_off[g->state_off[gi + 1]] - g->slot_off[g->state_off[gi]]);
        const size_t nsn = (size_t)(g->sn_off[gi + 1] - g->sn_off[gi]);
        const size_t row = std::max<size_t>(std::max(ne, nsn), 1);
        if (row * ((size_t)T + 1) >= (size_t)INT_MAX) { /* entry ids are int32 */
            ssw_set_error("utterance %d: %zu entering-list entries x %d frames exceed the history "
                          "table's 2^31 entries", u, row, T);
            return -1;
        }
        const size_t mine = row * ((size_t)T + 1);
        if (plan->big && (hist_total + mine) * sizeof(int2) > budget) {
            if (mine * sizeof(int2) > budget) {
                ssw_set_error("the history table of utterance %d (%zu entries, %zu bytes: frames x "
                              "entering-list entries) exceeds the budget of %zu bytes", u, mine,
                              mine * sizeof(int2), budget);
                return -1;
            }
            group.push_back(u);
            hist_total = 0;
        }
        hist_off[(size_t)u] = (long long)hist_total;
        hist_total += mine;
        sum += mine;
        *hist_cap = std::max(*hist_cap, hist_total);
        /* a path has at most one word exit per frame, each followed by at most one null entry,
         * after at most one null entry of frame -1 */
        *max_seg = std::max(*max_seg, 2 * T + 1);
    }
    group.push_back(n_utts);
    if (!plan->big && sum * sizeof(int2) > budget) {
        ssw_set_error("the history table of this call (%zu entries, %zu bytes: frames x "
                      "entering-list entries, summed over %d utterances) exceeds the budget of "
                      "%zu bytes; search fewer utterances per call", sum, sum * sizeof(int2), n_utts,
                      budget);
        return -1;
    }
    return 0;
}

extern "C" int32_t
ssw_grammar_history_groups(const ssw_grammar_plan_t *plan, const int32_t *fsg_of_utt,
                           const int32_t *utt_off, int32_t n_utts)
{
    std::vector<long long> hist_off;
    std::vector<int> group;
    size_t cap;
    int max_seg;
    if (plan == NULL || utt_off == NULL || n_utts < 0) {
        ssw_set_error("bad arguments to ssw_grammar_history_groups");
        return -1;
    }
    if (grammar_history_layout(plan, fsg_of_utt, utt_off, n_utts, hist_off, group, &cap, &max_seg) < 0)
        return -1;
    return n_utts > 0 ? (int32_t)group.size() - 1 : 0;
}

/* One call's grammar search in three steps, so that the default configuration can launch it
 * once per round (ssw_recognize_batch_active): begin() checks the call, makes the empty set and
 * uploads the tables; launch() runs the kernel over some rows; finish() fetches the results and
 * fills the set.  ssw_grammar_search_batch is begin, one launch, finish. */
struct grammar_run_t {
    ssw_model_t *m;
    const ssw_dict_t *d;
    const ssw_grammar_plan_t *plan;
    const int32_t *fsg_of_utt;
    int32_t n_utts;
    hipStream_t st;
    ssw_recognition_set_t *r;
    GrammarParams P;
    int max_seg;
    int *d_only; /* device [n_utts]: the utterances a round of the default configuration searches */
    std::vector<unsigned char> stage; /* must outlive its copy */
    std::vector<int> only_host;
    std::vector<int> group; /* first utterance of every history group, then n_utts */
    int *big_ws;            /* grammar_search_big_kernel's workspaces and their offsets */
    const long long *big_ws_off;
    bool uploaded;
    const char *who; /* the default configuration's entry point, for the loop's messages */

    grammar_run_t() : m(NULL), d(NULL), plan(NULL), fsg_of_utt(NULL), n_utts(0), st(NULL), r(NULL),
                      max_seg(1), d_only(NULL), big_ws(NULL), big_ws_off(NULL), uploaded(false),
                      who("ssw_recognize_batch_active") {}
    ~grammar_run_t()
    {
        if (uploaded)
            (void)hipStreamSynchronize(st);
        delete r;
    }
    int begin(ssw_model_t *m_, const ssw_dict_t *d_, const ssw_grammar_plan_t *plan_,
              const int32_t *fsg_of_utt_, const int32_t *utt_off, int32_t n_utts_, void *stream);
    hipError_t launch(const int16_t *d_senscr, const std::vector<int> *only, unsigned long long *mask,
                      const long long *d_act_off, const int *d_node_cnt);
    ssw_recognition_set_t *finish();
};

int
grammar_run_t::begin(ssw_model_t *m_, const ssw_dict_t *d_, const ssw_grammar_plan_t *plan_,
                     const int32_t *fsg_of_utt_, const int32_t *utt_off, int32_t n_utts_,
                     void *stream)
{
    m = m_;
    d = d_;
    plan = plan_;
    fsg_of_utt = fsg_of_utt_;
    n_utts = n_utts_;
    const ssw_fp_graphs_t *g = plan->g;
    st = (hipStream_t)stream;
    std::vector<long long> hist_off, ws_off((size_t)n_utts + 1, 0);
    size_t hist_total = 0, ws_ints = 0;
    if (grammar_history_layout(plan, fsg_of_utt, utt_off, n_utts, hist_off, group, &hist_total,
                               &max_seg) < 0)
        return -1;
    if (plan->big) /* the workspaces of a group's utterances, the largest group's in all */
        for (size_t k = 0; k + 1 < group.size(); ++k) {
            size_t at = 0;
            for (int u = group[k]; u < group[k + 1]; ++u) {
                ws_off[(size_t)u] = (long long)at;
                at += grammar_big_ws_ints(g, fsg_of_utt ? fsg_of_utt[u] : 0);
            }
            ws_ints = std::max(ws_ints, at);
        }
    r = new ssw_recognition_set_t();
    r->m = m;
    r->d = d;
    r->n_utts = n_utts;
    r->n_frames.resize((size_t)n_utts);
    r->status.assign((size_t)n_utts, 0);
    r->score.assign((size_t)n_utts, 0);
    r->message.assign((size_t)n_utts, std::string());
    r->hyp.assign((size_t)n_utts, std::string());
    r->has_hyp.assign((size_t)n_utts, 0);
    r->seg_off.assign((size_t)n_utts + 1, 0);
    r->n_seg.assign((size_t)n_utts, 0);
    for (int u = 0; u < n_utts; ++u)
        r->n_frames[(size_t)u] = utt_off[u + 1] - utt_off[u];
    if (n_utts == 0)
        return 0;

    /* one staging buffer -> one copy (WsLayout); the graph's tables first (they stay while the
     * plan is the last one searched), the call's after `o_call` */
    const size_t nG = (size_t)g->n_utts, nU = (size_t)n_utts, nN = (size_t)g->n_nodes;
    const size_t nL = (size_t)g->n_leaves, nS = (size_t)g->n_slots;
    WsLayout L;
    L.in(&P.node_off, g->node_off, sizeof(int) * (nG + 1));
    L.in(&P.leaf_off, g->leaf_off, sizeof(int) * (nG + 1));
    L.in(&P.state_off, g->state_off, sizeof(int) * (nG + 1));
    L.in(&P.senid, g->senid, sizeof(uint16_t) * 4 * nN);
    L.in(&P.pen, g->pen, sizeof(int) * nN);
    L.in(&P.parent, g->parent, sizeof(int) * nN);
    L.in(&P.info, g->info, sizeof(uint32_t) * nN);
    L.in(&P.ctxt, g->ctxt, sizeof(uint64_t) * nN);
    L.in(&P.leaf_ord, g->leaf_ord, sizeof(int) * nN);
    L.in(&P.leaf_wid, g->leaf_wid, sizeof(int) * nL);
    L.in(&P.leaf_node, g->leaf_node, sizeof(int) * nL);
    L.in(&P.leaf_lscr, g->leaf_lscr, sizeof(int) * nL);
    L.in(&P.slot_off, g->slot_off, sizeof(int) * ((size_t)g->n_states + 1));
    L.in(&P.slot_leaf, g->slot_leaf, sizeof(int) * nS);
    L.in(&P.slot_pen, g->slot_pen, sizeof(int) * nS);
    L.in(&P.slot_null, g->slot_null, sizeof(int) * nS);
    L.in(&P.slot_state, g->slot_state, sizeof(int) * nS);
    L.in(&P.ls_off, g->ls_off, sizeof(int) * (nL + 1));
    L.in(&P.ls_slot, g->ls_slot, sizeof(int) * (size_t)g->n_ls);
    L.in(&P.g_start, g->g_start, sizeof(int) * nG);
    L.in(&P.g_final, g->g_final, sizeof(int) * nG);
    L.in(&P.sn_off, g->sn_off, sizeof(int) * (nG + 1));
    L.in(&P.sn_to, g->sn_to, sizeof(int) * (size_t)g->n_sn);
    L.in(&P.sn_pen, g->sn_pen, sizeof(int) * (size_t)g->n_sn);
    L.in(&P.tw, g->tw, sizeof(int) * (size_t)g->n_tw);
    L.in(&P.tw_off, g->tw_off, sizeof(int) * (nG + 1));
    L.in(&P.twin_ref, g->twin_ref, sizeof(int) * nN);
    L.in(&P.tw_rk, g->tw_rk, sizeof(int) * nG);
    const size_t o_call = L.mark();
    L.in(&P.utt_off, utt_off, sizeof(int) * (nU + 1));
    L.in(&P.fsg_of_utt, fsg_of_utt, fsg_of_utt ? sizeof(int) * nU : 0);
    L.in(&P.hist_off, hist_off.data(), sizeof(long long) * nU);
    L.in(&big_ws_off, ws_off.data(), sizeof(long long) * nU);
    const size_t in_bytes = L.in_bytes();
    L.out(&P.n_seg, sizeof(int) * nU);
    L.out(&P.score, sizeof(int) * nU);
    L.out(&d_only, sizeof(int) * nU);
    L.out(&P.seg, sizeof(ssw_fsg_seg_t) * nU * (size_t)max_seg);
    L.out(&P.hist, sizeof(int2) * (hist_total ? hist_total : 1));
    L.out(&big_ws, sizeof(int) * ws_ints);

    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess) {
        bool moved = false;
        const int got = devbuf_reserve(m->gr_ws, L.size(), "ssw_grammar_search_batch", L.size() / 4, &moved);
        if (moved) /* the cached graphs went with the old buffer */
            m->gr_ws_uid = 0;
        if (got < 0)
            return -1;
    }
    const bool cached = m->gr_ws_uid != 0 && m->gr_ws_uid == g->uid;
    const size_t up_from = cached ? o_call : 0;
    stage.resize(in_bytes - up_from + 1);
    if (e == hipSuccess) {
        L.fill(stage.data(), up_from);
        e = hipMemcpyAsync(m->gr_ws.p + up_from, stage.data(), in_bytes - up_from,
                           hipMemcpyHostToDevice, st);
        m->gr_ws_uid = e == hipSuccess ? g->uid : 0;
        uploaded = true;
    }
    if (e == hipSuccess) {
        L.resolve(m->gr_ws.p);
        if (!fsg_of_utt)
            P.fsg_of_utt = NULL;
        P.senscr = NULL;
        P.only = NULL;
        P.act_mask = NULL;
        P.act_off = NULL;
        P.tp = (const uint32_t *)m->d_tp;
        P.n_sen = m->h->n_sen;
        P.max_seg = max_seg;
        P.beam = g->beam;
        P.pbeam = g->pbeam;
        P.wbeam = g->wbeam;
        P.sil = m->h->sil;
    }
    if (e != hipSuccess) {
        m->gr_ws_uid = 0;
        ssw_set_error("ssw_grammar_search_batch: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

/* `mask` != NULL: the EXPORT instances, the sets of active HMMs into mask (cleared first where
 * the kernel does not write every word of a searched utterance's rows: the one-workgroup
 * kernels); `only`: NULL or empty for every utterance, else the ones to search */
hipError_t
grammar_run_t::launch(const int16_t *d_senscr, const std::vector<int> *only, unsigned long long *mask,
                      const long long *d_act_off, const int *d_node_cnt)
{
    hipError_t e = hipSuccess;
    const bool exp = mask != NULL;
    const int n_run = only != NULL && !only->empty() ? (int)only->size() : n_utts;
    P.senscr = d_senscr;
    P.only = NULL;
    P.act_mask = mask;
    P.act_off = d_act_off;
    if (plan->big) {
        /* the history groups one after the other in the same table and workspace; of a round's
         * utterances, the members of each group (hist_off and ws_off are offsets within an
         * utterance's own group: they hold for any subset of it), a group without one skipped.
         * The exporting instance writes every word of a searched utterance's rows: nothing to
         * clear, d_node_cnt not needed */
        (void)d_node_cnt;
        const bool sub = exp && only != NULL && !only->empty();
        if (sub) {
            only_host = *only; /* (kept here: every round ends in a synchronisation of the stream) */
            if (!std::is_sorted(only_host.begin(), only_host.end())) /* (fpa_run's are ascending) */
                std::sort(only_host.begin(), only_host.end());
            e = hipMemcpyAsync(d_only, only_host.data(), sizeof(int) * (size_t)n_run,
                               hipMemcpyHostToDevice, st); /* once per round, every group's part */
            P.only = d_only;
        }
        GrammarBigParams B;
        B.g = P;
        B.ws = big_ws;
        B.ws_off = big_ws_off;
        void (*kern)(GrammarBigParams) =
            exp ? grammar_search_big_kernel<1024, true> : grammar_search_big_kernel<1024>;
        for (size_t k = 0; k + 1 < group.size() && e == hipSuccess; ++k) {
            int first = group[k], n = group[k + 1] - group[k];
            if (sub) { /* only_host[first .. first + n): the ones within [group[k], group[k + 1]) */
                const auto lo = std::lower_bound(only_host.begin(), only_host.end(), group[k]);
                const auto hi = std::lower_bound(lo, only_host.end(), group[k + 1]);
                first = (int)(lo - only_host.begin());
                n = (int)(hi - lo);
            }
            if (n <= 0)
                continue;
            B.u0 = first;
            hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(1024), 0, st, B);
            e = hipGetLastError();
        }
        return e;
    }
    if (only != NULL && !only->empty()) {
        only_host = *only; /* (kept here: every round ends in a synchronisation of the stream) */
        e = hipMemcpyAsync(d_only, only_host.data(), sizeof(int) * (size_t)n_run,
                           hipMemcpyHostToDevice, st);
        P.only = d_only;
    }
    if (e == hipSuccess && exp) {
        hipLaunchKernelGGL(fpa_clear_kernel, dim3((unsigned)n_run), dim3(256), 0, st, mask, d_act_off,
                           P.utt_off, d_node_cnt, P.only);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        /* one HMM per thread while a workgroup can hold the largest grammar of the plan; beyond
         * 1024, four or eight per thread of a 512-thread workgroup: two waves per SIMD leave a
         * lane 256 registers, which hold eight HMMs' state (1024 threads leave 128: four HMMs
         * per thread spilt there) */
        void (*kern)(GrammarParams);
        int tpb;
        const int mn = plan->max_nodes;
        if (mn <= 256) {
            kern = exp ? grammar_search_kernel<1, 256, true> : grammar_search_kernel<1, 256>;
            tpb = 256;
        } else if (mn <= 512) {
            kern = exp ? grammar_search_kernel<1, 512, true> : grammar_search_kernel<1, 512>;
            tpb = 512;
        } else if (mn <= 1024) {
            kern = exp ? grammar_search_kernel<1, 1024, true> : grammar_search_kernel<1, 1024>;
            tpb = 1024;
        } else if (mn <= 2048) {
            kern = exp ? grammar_search_kernel<4, 512, true> : grammar_search_kernel<4, 512>;
            tpb = 512;
        } else {
            kern = exp ? grammar_search_kernel<8, 512, true> : grammar_search_kernel<8, 512>;
            tpb = 512;
        }
        const size_t lds_bytes = plan->lds_ints * sizeof(int);
        if (lds_bytes > 48 * 1024)
            e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(kern, dim3(n_run), dim3(tpb), lds_bytes, st, P);
            e = hipGetLastError();
        }
    }
    return e;
}

/* the set, filled; NULL after an error (the set is freed with the run) */
ssw_recognition_set_t *
grammar_run_t::finish()
{
    const ssw_fp_graphs_t *g = plan->g;
    if (n_utts == 0) {
        ssw_recognition_set_t *out = r;
        r = NULL;
        return out;
    }
    std::vector<int> n_seg((size_t)n_utts), score((size_t)n_utts);
    std::vector<ssw_fsg_seg_t> seg((size_t)n_utts * (size_t)max_seg);
    hipError_t e = hipMemcpyAsync(n_seg.data(), P.n_seg, sizeof(int) * (size_t)n_utts,
                                  hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(score.data(), P.score, sizeof(int) * (size_t)n_utts, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(seg.data(), P.seg, sizeof(ssw_fsg_seg_t) * (size_t)n_utts * (size_t)max_seg,
                           hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    else
        (void)hipStreamSynchronize(st);
    if (e != hipSuccess) {
        m->gr_ws_uid = 0;
        ssw_set_error("ssw_grammar_search_batch: %s", hipGetErrorString(e));
        return NULL;
    }
    for (int u = 0; u < n_utts; ++u) {
        const int gi = fsg_of_utt ? fsg_of_utt[u] : 0;
        const int n = n_seg[(size_t)u];
        r->seg_off[(size_t)u] = (int32_t)r->seg.size();
        if (n == -1) {
            /* fsg_search_find_exit's frame_idx is fsgs->frame at the end: the frames searched */
            char msg[96];
            snprintf(msg, sizeof(msg), "Final result does not match the grammar in frame %d",
                     r->n_frames[(size_t)u]);
            r->status[(size_t)u] = 1;
            r->message[(size_t)u] = msg;
            continue;
        }
        if (n < 0) { /* (-(3 + k) cannot happen: max_seg bounds every path) */
            r->status[(size_t)u] = 2;
            r->message[(size_t)u] = "No hypothesis: no word exit in any frame";
            continue;
        }
        r->n_seg[(size_t)u] = n;
        r->score[(size_t)u] = score[(size_t)u];
        const ssw_fsg_seg_t *sg = seg.data() + (size_t)u * (size_t)max_seg;
        r->seg.insert(r->seg.end(), sg, sg + n);
        /* fsg_search_hyp, src/fsg_search.c:980-1029: base words, fillers and nulls left out */
        std::string &hyp = r->hyp[(size_t)u];
        for (int i = 0; i < n; ++i) {
            if (sg[i].wid < 0)
                continue;
            /* the grammar's notion of a filler (fsg_model_is_filler): the leaf's flag; all
             * leaves of one word in one grammar agree, so the first one found tells */
            bool filler = false;
            for (int l = g->leaf_off[gi]; l < g->leaf_off[gi + 1]; ++l)
                if (g->leaf_wid[l] == sg[i].wid) {
                    filler = g->leaf_filler[l] != 0;
                    break;
                }
            if (filler)
                continue;
            const char *w = ssw_dict_word(d, ssw_dict_base_id(d, sg[i].wid));
            if (!hyp.empty())
                hyp += ' ';
            hyp += w ? w : "";
        }
        r->has_hyp[(size_t)u] = hyp.empty() ? 0 : 1;
    }
    r->seg_off[(size_t)n_utts] = (int32_t)r->seg.size();
    ssw_recognition_set_t *out = r;
    r = NULL;
    return out;
}

/* what every recognition entry point asks of its arguments; d_in: the rows or features it reads */
static int
recognize_check_args(const char *who, const ssw_model_t *m, const ssw_dict_t *d,
                     const ssw_grammar_plan_t *plan, const void *d_in, int32_t n_frames,
                     const int32_t *utt_off, int32_t n_utts)
{
    if (m == NULL || d == NULL || plan == NULL || n_utts < 0 || n_frames < 0 || utt_off == NULL
        || !utt_off_spans(utt_off, n_utts, n_frames) || (n_frames > 0 && d_in == NULL)) {
        ssw_set_error("bad arguments to %s", who);
        return -1;
    }
    return 0;
}

extern "C" ssw_recognition_set_t *
ssw_grammar_search_batch(ssw_model_t *m, const ssw_dict_t *d, const ssw_grammar_plan_t *plan,
                         const int32_t *fsg_of_utt, const int16_t *d_senscr, int32_t n_frames,
                         const int32_t *utt_off, int32_t n_utts, void *stream)
{
    if (recognize_check_args("ssw_grammar_search_batch", m, d, plan, d_senscr, n_frames, utt_off, n_utts) < 0)
        return NULL;
    if (check_has_device(m) < 0)
        return NULL;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    grammar_run_t R;
    if (R.begin(m, d, plan, fsg_of_utt, utt_off, n_utts, stream) < 0)
        return NULL;
    if (n_utts > 0) {
        const hipError_t e = R.launch(d_senscr, NULL, NULL, NULL, NULL);
        if (e != hipSuccess) {
            m->gr_ws_uid = 0;
            ssw_set_error("ssw_grammar_search_batch: %s", hipGetErrorString(e));
            return NULL;
        }
    }
    return R.finish();
}

extern "C" ssw_recognition_set_t *
ssw_recognize_batch(ssw_model_t *m, const ssw_dict_t *d, const ssw_grammar_plan_t *plan,
                    const int32_t *fsg_of_utt, int scorer, const float *d_feats, int32_t n_frames,
                    const int32_t *utt_off, int32_t n_utts, void *stream)
{
    if (m == NULL || n_frames < 0 || (n_frames > 0 && d_feats == NULL)) {
        ssw_set_error("bad arguments to ssw_recognize_batch");
        return NULL;
    }
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    if (check_has_device(m) < 0)
        return NULL;
    if (hipSetDevice(m->device) != hipSuccess)
        return NULL;
    if (text_rows_reserve(m, n_frames, "ssw_recognize_batch") < 0)
        return NULL;
    if (n_frames > 0
        && ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, m->text_scr.as<int16_t>(), stream) < 0)
        return NULL;
    return ssw_grammar_search_batch(m, d, plan, fsg_of_utt, m->text_scr.as<int16_t>(), n_frames, utt_off,
                                    n_utts, stream);
}

/* the loop's search step (fpa_graph_t): the EXPORT instances of grammar_search_kernel, or of
 * grammar_search_big_kernel for a plan with a grammar beyond one workgroup */
static int
grammar_active_search(void *arg, const int16_t *rows, const std::vector<int> &only,
                      unsigned long long *mask, const long long *d_act_off, const int *d_node_cnt)
{
    grammar_run_t &R = *static_cast<grammar_run_t *>(arg);
    const hipError_t e = R.launch(rows, &only, mask, d_act_off, d_node_cnt);
    if (e != hipSuccess) {
        R.m->gr_ws_uid = 0;
        ssw_set_error("%s: %s", R.who, hipGetErrorString(e));
        return -1;
    }
    return 0;
}

/* what the loop needs of a grammar run: every utterance's HMMs are those of its grammar */
static void
grammar_fpa_graph(fpa_graph_t &G, const char *who, grammar_run_t &R)
{
    const ssw_fp_graphs_t *g = R.plan->g;
    G.who = who;
    G.n_nodes = g->n_nodes;
    G.senid = g->senid;
    G.max_nodes = R.plan->max_nodes;
    for (int u = 0; u < R.n_utts; ++u) {
        const int gi = R.fsg_of_utt ? R.fsg_of_utt[u] : 0; /* (checked by begin) */
        G.node_base.push_back(g->node_off[gi]);
        G.node_cnt.push_back(g->node_off[gi + 1] - g->node_off[gi]);
    }
    G.search = grammar_active_search;
    G.arg = &R;
}

/* the loop's request as both grammar entries start it: the inputs, the rows, the grammar
 * entries' counters; each then names the outputs it wants */
static FpaReq
grammar_fpa_req(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_frames,
                const int32_t *utt_off, int32_t n_utts, int16_t *rows, void *stream)
{
    FpaReq A{};
    A.scorer = scorer;
    A.d_feats = d_feats;
    A.n_frames = n_frames;
    A.utt_off = utt_off;
    A.n_utts = n_utts;
    A.d_rows = rows;
    A.stats = m->gra_stats;
    A.stream = stream;
    return A;
}

/* decoder_set_fsg + decoder_process + decoder_hyp in the reference's DEFAULT configuration
 * (compallsen = no) for a batch, from features: every frame scored for the senones of the HMMs
 * fsg_search_sen_active lists (src/fsg_search.c:310-325), through acmod's flags2list with its
 * bridges (src/acmod.c:947-999), then searched by fsg_search_step (src/fsg_search.c:664-739) --
 * by speculation and proof (ssw_k7_fpactive.inc, ssw_k9_grammar.inc). */
extern "C" ssw_recognition_set_t *
ssw_recognize_batch_active(ssw_model_t *m, const ssw_dict_t *d, const ssw_grammar_plan_t *plan,
                           const int32_t *fsg_of_utt, int scorer, const float *d_feats,
                           int32_t n_frames, const int32_t *utt_off, int32_t n_utts,
                           int16_t *d_senscr, uint32_t *listed, int32_t *rounds, void *stream)
{
    const char *who = "ssw_recognize_batch_active";
    if (recognize_check_args(who, m, d, plan, d_feats, n_frames, utt_off, n_utts) < 0)
        return NULL;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    if (check_has_device(m) < 0)
        return NULL;
    if (cont_refuse_active(m, who) < 0)
        return NULL;
    if (plan->big && !plan->active) {
        ssw_set_error("grammar %d (%s) has %d phone-tree HMMs and is searched from an HBM workspace: "
                      "the default configuration (compallsen = no) holds a plan's largest grammar "
                      "in one workgroup; use ssw_recognize_batch", plan->big_fsg,
                      plan->big_name.c_str(), plan->big_nodes);
        return NULL;
    }
    if (scorer == SSW_SCORER_S2_SEMI) {
        ssw_recognition_set_t *r = NULL;
        semi_active_route(who, listed, "listed", m->gra_stats, n_utts, rounds, [&] {
            if (hipSetDevice(m->device) != hipSuccess)
                return -1;
            int16_t *all = active_rows(m, d_senscr, n_frames, who);
            if (all == NULL)
                return -1;
            if (n_frames > 0
                && ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, all, stream) < 0)
                return -1;
            r = ssw_grammar_search_batch(m, d, plan, fsg_of_utt, all, n_frames, utt_off, n_utts, stream);
            return r != NULL ? 0 : -1;
        });
        return r;
    }
    if (fpa_check_limits(m, who, scorer) < 0)
        return NULL;
    if (hipSetDevice(m->device) != hipSuccess)
        return NULL;
    int16_t *rows = active_rows(m, d_senscr, n_frames, who);
    if (rows == NULL)
        return NULL;
    grammar_run_t R;
    if (R.begin(m, d, plan, fsg_of_utt, utt_off, n_utts, stream) < 0)
        return NULL;
    if (n_utts == 0)
        return R.finish();
    fpa_graph_t G;
    grammar_fpa_graph(G, who, R);
    FpaReq A = grammar_fpa_req(m, scorer, d_feats, n_frames, utt_off, n_utts, rows, stream);
    A.full_rows = d_senscr != NULL;
    A.rounds_out = rounds;
    A.listed_out = listed;
    if (fpa_run(m, G, A) < 0)
        return NULL;
    return R.finish();
}

/* ---------------------------------------------------------------------------------- */
/* decoder_alignment after a grammar search (src/decoder.c:737-798)                     */
/* ---------------------------------------------------------------------------------- */
/* The best path's entries as alignment_add_word takes them (:758-768): every entry whose word is
 * a dictionary word -- fillers and alternate pronunciations included, "(NULL)" left out -- with
 * sf and ef - sf + 1, the windows as they are (the contiguity assert of :763 is compiled out of
 * a release build).  n_seg[u] = -1 and a status for an utterance that has no alignment. */
struct rec_word_segs_t {
    int32_t max_seg;
    std::vector<int32_t> n_seg, pre_status;
    std::vector<ssw_word_seg_t> seg;
    std::vector<std::string> message;
};

static void
recognition_word_segs(const ssw_recognition_set_t *r, rec_word_segs_t &w)
{
    const int n_utts = r->n_utts;
    w.max_seg = 1;
    for (int u = 0; u < n_utts; ++u)
        w.max_seg = std::max(w.max_seg, r->n_seg[(size_t)u]);
    w.n_seg.assign((size_t)n_utts, -1);
    w.pre_status.assign((size_t)n_utts, 1);
    w.message.assign((size_t)n_utts, std::string());
    w.seg.assign((size_t)n_utts * (size_t)w.max_seg, ssw_word_seg_t());
    for (int u = 0; u < n_utts; ++u) {
        if (r->status[(size_t)u] != 0) { /* decoder_seg_iter NULL: no alignment (:753-755) */
            w.message[(size_t)u] = r->message[(size_t)u];
            continue;
        }
        const ssw_fsg_seg_t *sg = r->seg.data() + r->seg_off[(size_t)u];
        ssw_word_seg_t *out = w.seg.data() + (size_t)u * (size_t)w.max_seg;
        int n = 0;
        for (int i = 0; i < r->n_seg[(size_t)u]; ++i) {
            if (sg[i].wid < 0)
                continue;
            out[n].wid = sg[i].wid;
            out[n].start = sg[i].sf;
            out[n].duration = sg[i].ef - sg[i].sf + 1;
            ++n;
        }
        if (n == 0) {
            w.pre_status[(size_t)u] = 2;
            w.message[(size_t)u] = "The best path holds no dictionary word (null transitions only): "
                                   "nothing to align";
            continue;
        }
        w.n_seg[(size_t)u] = n;
    }
}

static int
recognition_set_check(const char *who, const ssw_model_t *m, const ssw_recognition_set_t *r,
                      int32_t n_frames, const int32_t *utt_off)
{
    if (m == NULL || r == NULL || n_frames < 0 || utt_off == NULL
        || !utt_off_spans(utt_off, r->n_utts, n_frames)) {
        ssw_set_error("bad arguments to %s", who);
        return -1;
    }
    if (r->m != m) {
        ssw_set_error("%s: the recognition set was made with another model", who);
        return -1;
    }
    for (int u = 0; u < r->n_utts; ++u)
        if (utt_off[u + 1] - utt_off[u] != r->n_frames[(size_t)u]) {
            ssw_set_error("%s: utterance %d has %d frames in utt_off and %d in the recognition set",
                          who, u, utt_off[u + 1] - utt_off[u], r->n_frames[(size_t)u]);
            return -1;
        }
    return 0;
}

/* the second half for a recognition set; `who` has checked the set */
static ssw_alignment_set_t *
recognition_align(ssw_model_t *m, const ssw_recognition_set_t *r, const int16_t *d_senscr,
                  const int32_t *utt_off, const fpa_mode_t *fpa, const uint32_t *seed,
                  const uint32_t *d_carry, void *stream)
{
    rec_word_segs_t w;
    recognition_word_segs(r, w);
    AlignSegReq Q{};
    Q.d = r->d;
    Q.d_senscr = d_senscr;
    Q.utt_off = utt_off;
    Q.n_utts = r->n_utts;
    Q.n_seg = w.n_seg.data();
    Q.seg = w.seg.data();
    Q.max_seg = w.max_seg;
    Q.pre_status = w.pre_status.data();
    Q.message = &w.message;
    Q.fpa = fpa;
    Q.seed = seed;
    Q.d_carry = d_carry;
    Q.stream = stream;
    ssw_alignment_set_t *a = align_word_segments(m, Q);
    if (a != NULL)
        a->hyp = r->hyp; /* decoder_hyp's text, for the JSON line's "t" */
    return a;
}

extern "C" ssw_alignment_set_t *
ssw_recognition_set_align(ssw_model_t *m, const ssw_recognition_set_t *r, const int16_t *d_senscr,
                          int32_t n_frames, const int32_t *utt_off, void *stream)
{
    if (recognition_set_check("ssw_recognition_set_align", m, r, n_frames, utt_off) < 0)
        return NULL;
    if (n_frames > 0 && d_senscr == NULL) {
        ssw_set_error("bad arguments to ssw_recognition_set_align");
        return NULL;
    }
    if (check_has_device(m) < 0)
        return NULL;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    return recognition_align(m, r, d_senscr, utt_off, NULL, NULL, NULL, stream);
}

/* ssw_recognize_batch, then decoder_alignment over the same rows; with two_pass_history (PTM and
 * s2_semi) the rows are made again in between from the order every utterance's own search left,
 * as ssw_align_text_batch does (src/decoder.c:786-793, src/ptm_mgau.c:425-448) */
static ssw_alignment_set_t *
recognize_align_rows(const char *who, ssw_model_t *m, const ssw_dict_t *d,
                     const ssw_grammar_plan_t *plan, const int32_t *fsg_of_utt, int scorer,
                     const float *d_feats, int32_t n_frames, const int32_t *utt_off, int32_t n_utts,
                     int32_t two_pass_history, ssw_recognition_set_t **rec_out, void *stream)
{
    if (rec_out != NULL)
        *rec_out = NULL;
    if (recognize_check_args(who, m, d, plan, d_feats, n_frames, utt_off, n_utts) < 0)
        return NULL;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    if (check_has_device(m) < 0)
        return NULL;
    if (hipSetDevice(m->device) != hipSuccess)
        return NULL;
    if (text_rows_reserve(m, n_frames, who) < 0)
        return NULL;
    int16_t *rows = m->text_scr.as<int16_t>();
    if (n_frames > 0 && ssw_score_batch(m, scorer, d_feats, n_frames, utt_off, n_utts, rows, stream) < 0)
        return NULL;
    const bool two_pass = two_pass_history != 0
        && (scorer == SSW_SCORER_PTM || scorer == SSW_SCORER_S2_SEMI) && n_frames > 0 && n_utts > 0;
    if (two_pass && carry_last_orders(m, who, n_utts, stream) < 0)
        return NULL;
    ssw_recognition_set_t *r = ssw_grammar_search_batch(m, d, plan, fsg_of_utt, rows, n_frames,
                                                        utt_off, n_utts, stream);
    if (r == NULL)
        return NULL;
    ssw_alignment_set_t *a = NULL;
    rescore_t rs = rescore_request(m, scorer, d_feats, n_frames, utt_off, n_utts, rows, stream);
    if (!two_pass || rescore_run(&rs) >= 0)
        a = recognition_align(m, r, rows, utt_off, NULL, NULL, NULL, stream);
    if (a != NULL && rec_out != NULL)
        *rec_out = r;
    else
        ssw_recognition_set_free(r);
    return a;
}

extern "C" ssw_alignment_set_t *
ssw_recognize_align_batch(ssw_model_t *m, const ssw_dict_t *d, const ssw_grammar_plan_t *plan,
                          const int32_t *fsg_of_utt, int scorer, const float *d_feats,
                          int32_t n_frames, const int32_t *utt_off, int32_t n_utts,
                          int32_t two_pass_history, ssw_recognition_set_t **rec_out, void *stream)
{
    return recognize_align_rows("ssw_recognize_align_batch", m, d, plan, fsg_of_utt, scorer, d_feats,
                                n_frames, utt_off, n_utts, two_pass_history, rec_out, stream);
}

/* the same in the reference's default configuration (compallsen = no): ssw_recognize_batch_active,
 * then the second pass as ssw_align_batch_active_ex runs it, seeded with acmod's flags after the
 * grammar search's last frame (they only grow from there, src/state_align_search.c:186-189) and,
 * with two_pass_history and PTM, started from the orders the search left in history slot 1 */
extern "C" ssw_alignment_set_t *
ssw_recognize_align_batch_active(ssw_model_t *m, const ssw_dict_t *d,
                                 const ssw_grammar_plan_t *plan, const int32_t *fsg_of_utt,
                                 int scorer, const float *d_feats, int32_t n_frames,
                                 const int32_t *utt_off, int32_t n_utts, int32_t two_pass_history,
                                 ssw_recognition_set_t **rec_out, int32_t *rounds, void *stream)
{
    const char *who = "ssw_recognize_align_batch_active";
    if (rec_out != NULL)
        *rec_out = NULL;
    if (recognize_check_args(who, m, d, plan, d_feats, n_frames, utt_off, n_utts) < 0)
        return NULL;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return NULL;
    if (check_has_device(m) < 0)
        return NULL;
    if (cont_refuse_active(m, who) < 0)
        return NULL;
    if (plan->big && !plan->active) {
        ssw_set_error("%s: grammar %d (%s) has %d phone-tree HMMs and is searched from an HBM "
                      "workspace: the default configuration (compallsen = no) takes such a plan "
                      "from ssw_grammar_prepare_large_active only; use ssw_recognize_align_batch",
                      who, plan->big_fsg, plan->big_name.c_str(), plan->big_nodes);
        return NULL;
    }
    if (scorer == SSW_SCORER_S2_SEMI) {
        ssw_alignment_set_t *a = NULL;
        semi_active_route(who, NULL, NULL, m->gra_stats, n_utts, rounds, [&] {
            a = recognize_align_rows(who, m, d, plan, fsg_of_utt, scorer, d_feats, n_frames, utt_off,
                                     n_utts, two_pass_history, rec_out, stream);
            return a != NULL ? 0 : -1;
        });
        return a;
    }
    if (fpa_check_limits(m, who, scorer) < 0)
        return NULL;
    if (hipSetDevice(m->device) != hipSuccess)
        return NULL;
    int16_t *rows = active_rows(m, NULL, n_frames, who);
    if (rows == NULL)
        return NULL;
    const bool carry2 = two_pass_history != 0 && scorer == SSW_SCORER_PTM && n_utts > 0;
    if (carry2 && carry_rows_reserve(m, n_utts, who) < 0)
        return NULL;
    const uint32_t *d_carry = carry2 ? m->carry_rows.as<uint32_t>() : NULL;
    const size_t nw32 = ((size_t)m->h->n_sen + 31) / 32;
    std::vector<uint32_t> seed((size_t)n_utts * nw32, 0u); /* acmod's set after the last frame */
    ssw_recognition_set_t *r = NULL;
    {
        grammar_run_t R;
        R.who = who;
        if (R.begin(m, d, plan, fsg_of_utt, utt_off, n_utts, stream) < 0)
            return NULL;
        if (n_utts > 0) {
            fpa_graph_t G;
            grammar_fpa_graph(G, who, R);
            FpaReq A = grammar_fpa_req(m, scorer, d_feats, n_frames, utt_off, n_utts, rows, stream);
            A.seed_out = seed.data();
            A.rounds_out = rounds;
            A.d_carry_out = carry2 ? m->carry_rows.as<uint32_t>() : NULL;
            if (fpa_run(m, G, A) < 0)
                return NULL;
        }
        r = R.finish();
    }
    if (r == NULL)
        return NULL;
    fpa_mode_t mode = { scorer, d_feats, two_pass_history != 0 };
    ssw_alignment_set_t *a = recognition_align(m, r, rows, utt_off, &mode, seed.data(), d_carry, stream);
    if (a != NULL && rec_out != NULL)
        *rec_out = r;
    else
        ssw_recognition_set_free(r);
    return a;
}

/* [0] utterances searched by ssw_recognize_batch_active since the model was loaded, [1] their
 * verify rounds summed, [2] rounds of the last call, [3] utterances whose first assumption (the
 * compallsen = yes trajectory) was not the reference's */
extern "C" int
ssw_grammar_active_stats(ssw_model_t *m, int64_t stats[4])
{
    for (int i = 0; i < 4; ++i)
        stats[i] = m->gra_stats[i];
    return 0;
}

extern "C" int32_t
ssw_recognition_set_status(const ssw_recognition_set_t *r, int32_t utt)
{
    return (r == NULL || utt < 0 || utt >= r->n_utts) ? -1 : r->status[(size_t)utt];
}

extern "C" const char *
ssw_recognition_set_message(const ssw_recognition_set_t *r, int32_t utt)
{
    return (r == NULL || utt < 0 || utt >= r->n_utts) ? NULL : r->message[(size_t)utt].c_str();
}

extern "C" int32_t
ssw_recognition_set_segments(const ssw_recognition_set_t *r, int32_t utt, const ssw_fsg_seg_t **seg)
{
    if (r == NULL || utt < 0 || utt >= r->n_utts)
        return -1;
    if (seg)
        *seg = r->seg.data() + r->seg_off[(size_t)utt];
    return r->n_seg[(size_t)utt];
}

extern "C" int32_t
ssw_recognition_set_score(const ssw_recognition_set_t *r, int32_t utt, int32_t *score)
{
    if (r == NULL || utt < 0 || utt >= r->n_utts || r->status[(size_t)utt] != 0)
        return -1;
    if (score)
        *score = r->score[(size_t)utt];
    return 0;
}

extern "C" int32_t
ssw_recognition_set_hyp(const ssw_recognition_set_t *r, int32_t utt, char *out, int32_t out_len)
{
    if (r == NULL || utt < 0 || utt >= r->n_utts || !r->has_hyp[(size_t)utt])
        return -1;
    const std::string &h = r->hyp[(size_t)utt];
    if (out != NULL && out_len > 0)
        snprintf(out, (size_t)out_len, "%s", h.c_str());
    return (int32_t)h.size();
}

extern "C" int32_t
ssw_recognition_set_json(const ssw_recognition_set_t *r, int32_t utt, double utt_start,
                         int32_t frate, char *out, int32_t out_len)
{
    if (r == NULL || utt < 0 || utt >= r->n_utts || frate <= 0)
        return -1;
    const double base = r->m->h->cfg.logbase;
    std::string s;
    char tmp[128];
    /* format_hyp: duration = decoder_n_frames / frate = (frames + 1) / frate, prob =
     * logmath_exp(decoder_prob = 0) */
    snprintf(tmp, sizeof(tmp), "{\"b\":%.3f,\"d\":%.3f,\"p\":%.3f,\"t\":\"", utt_start,
             (double)(r->n_frames[(size_t)utt] + 1) / frate, pow(base, 0.0));
    s += tmp;
    s += r->hyp[(size_t)utt];
    s += "\",\"w\":[";
    const ssw_fsg_seg_t *sg = r->seg.data() + r->seg_off[(size_t)utt];
    for (int i = 0; i < r->n_seg[(size_t)utt]; ++i) {
        /* format_seg: st = start + sf / frate, dur = (ef + 1 - sf) / frate */
        const char *w = sg[i].wid < 0 ? "(NULL)" : ssw_dict_word(r->d, sg[i].wid);
        snprintf(tmp, sizeof(tmp), "%s{\"b\":%.3f,\"d\":%.3f,\"p\":%.3f,\"t\":\"", i ? "," : "",
                 utt_start + (double)sg[i].sf / frate, (double)(sg[i].ef + 1 - sg[i].sf) / frate,
                 pow(base, (double)(sg[i].ascr + sg[i].lscr)));
        s += tmp;
        s += w ? w : "";
        s += "\"}";
    }
    s += "]}\n";
    if (out != NULL && out_len > 0)
        snprintf(out, (size_t)out_len, "%s", s.c_str());
    return (int32_t)s.size();
}

extern "C" void
ssw_recognition_set_free(ssw_recognition_set_t *r)
{
    delete r;
}
