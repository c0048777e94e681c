/* fpa_shape and the round policy (csrc/ssw_fpa_shape.inc) on the CPU against the arithmetic they
 * were moved out of, kept here verbatim as it stood in fpa_run (the mask layout, cap, the LDS
 * limit check with its message, the utterance-start words, the comparison's slice count, the
 * one-by-one rule and the next round's `only`; the model, the graph and the request bound to
 * stand-ins).  Every output, over batches of 1, 4, 5, 16 and 17 utterances x node counts 1, 63,
 * 64, 65, 128, 129 dealt round the batch from six starting points x frames (short utterances; one
 * of them of 0 frames; n_frames = 0; 100,000 frames each, for the slices' upper bound) x n_sen 5,
 * 6 (cap bound by n_sen), 5126, 5381, 65000 (bound by 3 max_nodes + n_sen / 255 + 2, odd and
 * even), 1300000 (the plan kernel's bitmap alone beyond a CU) x PTM, ms, continuous x the
 * caller's bound on the HMMs 0, 200 and, found by the verbatim arithmetic for n_sen = 65000, the
 * last bound the kind accepts and the first it refuses x d_carry_out on and off.
 * Last line for the test to read:
 *   ok: N shapes, R of them refused, P policy cases
 * Built with -fsanitize=address,undefined (tests/test_fpa_shape_host.py); the tables have exactly
 * the size fpa_shape may read. */
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../soundswallower_amd/csrc/ssw_senone_lds.inc"
#include "../../soundswallower_amd/csrc/ssw_fpa_shape.inc"

/* ---- stand-ins for what the parent's code names ---- */
#define SSW_SCORER_PTM 0
#define SSW_SCORER_MS 1
struct RefHostModel {
    int n_sen, continuous, veclen_total;
};
struct RefKnobs {
    int fpa_sub;
};
struct RefModel {
    const RefHostModel *h;
    int n_cbf;
    RefKnobs kn;
};
struct RefGraph {
    const char *who;
    std::vector<int> node_cnt;
    int max_nodes;
};

static char ref_error[320];
static void
ssw_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ref_error, sizeof(ref_error), fmt, ap);
    va_end(ap);
}

/* (ssw_host_cont_listed.inc, as it stood) */
static size_t
cont_listed_lds(const RefModel *m, int cap)
{
    return ContListedCarve(m->h->veclen_total, cap).bytes();
}

struct RefShape {
    std::vector<long long> act_off;
    long long mask_words;
    int max_nodes, max_len, cap, nw32;
    size_t plan_lds, sen_lds, n_start_words, o_start_bytes;
};

static int
reference_shape(const RefModel *m, const RefGraph &G, int scorer, int32_t n_frames,
                const int32_t *utt_off, int32_t n_utts, uint32_t *d_carry_out, RefShape &out)
{
    const RefHostModel *h = m->h;
    /* ---- the parent's lines, verbatim ---- */
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
    size_t plan_lds_out, sen_lds_out;
    {
        /* what the two per-frame kernels keep in LDS per wave (four waves a workgroup) */
        const size_t plan_lds = 4 * ((4 * (size_t)nw32 + 2 * (size_t)cap + 8 + 15) & ~(size_t)15);
        const size_t sen_lds = h->continuous
            ? cont_listed_lds(m, cap)
            : 4 * (((scorer == SSW_SCORER_MS ? 0 : 8 * (size_t)m->n_cbf)
                    + 4 * (size_t)((cap + 1) & ~1) + 16 + 15) & ~(size_t)15);
        plan_lds_out = plan_lds;
        sen_lds_out = sen_lds;
        if (std::max(plan_lds, sen_lds) > 156 * 1024) {
            ssw_set_error("%s: %d senones x texts of up to %d phone-tree "
                          "HMMs need %zu KB of LDS per workgroup (160 KB a CU)", G.who, h->n_sen, max_nodes,
                          std::max(plan_lds, sen_lds) / 1024);
            return -1;
        }
    }
    const size_t nf = (size_t)std::max(n_frames, 1);
    int max_len = 0;
    for (int u = 0; u < n_utts; ++u)
        max_len = std::max(max_len, utt_off[u + 1] - utt_off[u]);
    /* (two-pass history: the whole batch's utterance-start bits, for fpa_carry_rows_kernel) */
    const size_t n_start_words = nf / 32 + 2;
    const size_t o_start_bytes = d_carry_out != NULL ? sizeof(uint32_t) * n_start_words : 0;
    /* ---- */
    out.act_off = act_off;
    out.mask_words = mask_words;
    out.max_nodes = max_nodes;
    out.max_len = max_len;
    out.cap = cap;
    out.nw32 = nw32;
    out.plan_lds = plan_lds_out;
    out.sen_lds = sen_lds_out;
    out.n_start_words = n_start_words;
    out.o_start_bytes = o_start_bytes;
    return 0;
}

/* the parent's slice count for a comparison over n_cmp utterances, verbatim */
static unsigned
reference_slices(long long mask_words, int n_cmp)
{
    const unsigned slices = (unsigned)std::min<long long>(
        64, std::max<long long>(1, mask_words / std::max(1, n_cmp) / (256 * 16)));
    return slices;
}

static RefHostModel
host_model(int kind, int n_sen)
{
    return RefHostModel{ n_sen, kind == FPA_CONT, 39 };
}

/* the smallest bound on the HMMs that the parent's arithmetic refuses for this kind of model with
 * 65,000 senones and one utterance of one HMM */
static int
first_refused_bound(int kind)
{
    const RefHostModel h = host_model(kind, 65000);
    const RefModel m = { &h, 12, { -1 } };
    const int32_t utt_off[2] = { 0, 10 };
    for (int bound = 1; bound < 40000; ++bound) {
        const RefGraph G = { "who", { 1 }, bound };
        RefShape out;
        if (reference_shape(&m, G, kind == FPA_MS ? SSW_SCORER_MS : SSW_SCORER_PTM, 10, utt_off, 1, NULL, out) < 0)
            return bound;
    }
    printf("FAILED: no bound is refused for kind %d\n", kind);
    exit(1);
}

#define FAIL(...)                                                                             \
    do {                                                                                      \
        printf("FAILED n_utts %d rotation %d frames %d n_sen %d kind %d bound %d carry %d: ", \
               n_utts, rot, fmode, n_sen, kind, bound, carry);                                \
        printf(__VA_ARGS__);                                                                  \
        printf("\n");                                                                         \
        return 1;                                                                             \
    } while (0)

static int
policy_cases(long &n_policy)
{
    for (int fpa_sub : { -1, 0, 1 })
        for (int n_utts : { 1, 4, 5, 16, 17 })
            for (int n_only : { 0, 1, 4, 5, n_utts / 4, n_utts / 4 + 1, n_utts - 1, n_utts }) {
                const RefKnobs kn = { fpa_sub };
                const RefModel mm = { NULL, 0, kn }, *m = &mm;
                std::vector<int> only((size_t)n_only), again;
                for (int i = 0; i < n_only; ++i)
                    only[(size_t)i] = 2 * i;
                /* the parent's rule, verbatim */
                const bool one_by_one = !only.empty()
                    && (m->kn.fpa_sub == 1
                        || (m->kn.fpa_sub != 0 && (int)only.size() <= std::max(4, n_utts / 4)));
                ++n_policy;
                if (fpa_one_by_one((size_t)n_only, n_utts, fpa_sub) != one_by_one) {
                    printf("FAILED: fpa_sub %d, %d utterances, %d unproven: one by one %d, the parent's %d\n",
                           fpa_sub, n_utts, n_only, !one_by_one, one_by_one);
                    return 1;
                }
                /* the next round: `again` of n_only utterances after a round over anything */
                for (int prev = 0; prev < 2; ++prev) {
                    std::vector<int> want_only(prev ? 3 : 0, 7), want_again((size_t)n_only);
                    for (int i = 0; i < n_only; ++i)
                        want_again[(size_t)i] = 3 * i + 1;
                    std::vector<int> got_only = want_only, got_again = want_again;
                    {
                        std::vector<int> &only = want_only, &again = want_again;
                        /* the parent's lines, verbatim */
                        only.swap(again);
                        if ((int)only.size() == n_utts && n_utts > 4 && m->kn.fpa_sub != 1)
                            only.clear(); /* every one of them: the whole batch as a whole */
                    }
                    fpa_next_only(got_only, got_again, n_utts, fpa_sub);
                    if (got_only != want_only) {
                        printf("FAILED: fpa_sub %d, %d utterances, %d go round again: the next round's "
                               "`only` has %zu, the parent's %zu\n", fpa_sub, n_utts, n_only,
                               got_only.size(), want_only.size());
                        return 1;
                    }
                    /* (the parent cleared a list that was not empty) */
                    if (fpa_whole_batch((size_t)n_only, n_utts, fpa_sub) != (n_only != 0 && want_only.empty())) {
                        printf("FAILED: fpa_whole_batch(%d, %d, %d)\n", n_only, n_utts, fpa_sub);
                        return 1;
                    }
                }
            }
    return 0;
}

int
main()
{
    const int NODES[6] = { 1, 63, 64, 65, 128, 129 };
    int refuse_at[3];
    for (int kind = 0; kind < 3; ++kind)
        refuse_at[kind] = first_refused_bound(kind);
    long n_cases = 0, n_refused = 0, n_policy = 0;
    long under_ok[3] = { 0, 0, 0 }, over_refused[3] = { 0, 0, 0 };
    unsigned max_slices = 0;
    static uint32_t carry_rows;
    for (int n_utts : { 1, 4, 5, 16, 17 })
        for (int rot = 0; rot < 6; ++rot)
            for (int fmode = 0; fmode < 4; ++fmode) {
                /* exactly what fpa_shape may read: [n_utts] node counts, [n_utts + 1] offsets */
                std::vector<int> node_cnt, utt_off(1, 0);
                for (int u = 0; u < n_utts; ++u) {
                    node_cnt.push_back(NODES[(u + rot) % 6]);
                    const int len = fmode == 2 ? 0
                        : fmode == 3           ? 100000
                        : fmode == 1 && u == n_utts / 2 ? 0
                                                        : 10 + 3 * u;
                    utt_off.push_back(utt_off.back() + len);
                }
                const int n_frames = utt_off.back();
                for (int n_sen : { 5, 6, 5126, 5381, 65000, 1300000 })
                    for (int kind = 0; kind < 3; ++kind)
                        for (int bsel = 0; bsel < 4; ++bsel)
                            for (int carry = 0; carry < 2; ++carry) {
                                const int bound = bsel == 0 ? 0
                                    : bsel == 1             ? 200
                                    : bsel == 2             ? refuse_at[kind] - 1
                                                            : refuse_at[kind];
                                const RefHostModel h = host_model(kind, n_sen);
                                const RefModel m = { &h, 12, { -1 } };
                                const RefGraph G = { "ssw_recognize_batch_active", node_cnt, bound };
                                const int scorer = kind == FPA_MS ? SSW_SCORER_MS : SSW_SCORER_PTM;
                                RefShape want;
                                ref_error[0] = 0;
                                const int rc_want = reference_shape(&m, G, scorer, n_frames, utt_off.data(), n_utts,
                                                                    carry ? &carry_rows : NULL, want);
                                const FpaModelSizes M = { kind, n_sen, 12, 39 };
                                FpaShape S;
                                const int rc = fpa_shape(G.who, M, node_cnt.data(), bound, utt_off.data(), n_utts,
                                                         n_frames, carry != 0, S);
                                ++n_cases;
                                if (rc != rc_want)
                                    FAIL("returns %d, the parent's lines %d", rc, rc_want);
                                if (n_sen == 65000 && bsel == 2)
                                    under_ok[kind] += rc == 0;
                                if (n_sen == 65000 && bsel == 3)
                                    over_refused[kind] += rc < 0;
                                if (rc < 0) {
                                    if (strcmp(S.err, ref_error) != 0)
                                        FAIL("message '%s', the parent's '%s'", S.err, ref_error);
                                    ++n_refused;
                                    continue;
                                }
                                if (S.act_off != want.act_off || S.mask_words != want.mask_words)
                                    FAIL("act_off differ, or mask_words %lld (%lld)", S.mask_words, want.mask_words);
                                if (S.max_nodes != want.max_nodes || S.max_len != want.max_len)
                                    FAIL("max_nodes %d (%d), max_len %d (%d)", S.max_nodes, want.max_nodes,
                                         S.max_len, want.max_len);
                                if (S.cap != want.cap || S.nw32 != want.nw32 || fpa_cap(n_sen, S.max_nodes) != want.cap)
                                    FAIL("cap %d (%d), nw32 %d (%d)", S.cap, want.cap, S.nw32, want.nw32);
                                if (S.plan_lds != want.plan_lds || S.sen_lds != want.sen_lds)
                                    FAIL("LDS of the plan %zu (%zu), of the listed scorer %zu (%zu)", S.plan_lds,
                                         want.plan_lds, S.sen_lds, want.sen_lds);
                                if (S.n_start_words != want.n_start_words || S.start_bytes != want.o_start_bytes)
                                    FAIL("start words %zu (%zu), their bytes %zu (%zu)", S.n_start_words,
                                         want.n_start_words, S.start_bytes, want.o_start_bytes);
                                for (int n_cmp : { n_utts, 1, std::max(1, n_utts / 4) }) {
                                    const unsigned sl = fpa_compare_slices(S.mask_words, n_cmp);
                                    if (sl != reference_slices(want.mask_words, n_cmp))
                                        FAIL("%u slices over %d utterances, the parent's %u", sl, n_cmp,
                                             reference_slices(want.mask_words, n_cmp));
                                    max_slices = std::max(max_slices, sl);
                                }
                            }
            }
    for (int kind = 0; kind < 3; ++kind)
        if (under_ok[kind] == 0 || over_refused[kind] == 0) {
            printf("FAILED: kind %d was not seen accepted just under and refused just over 156 KB\n", kind);
            return 1;
        }
    if (max_slices != 64) {
        printf("FAILED: no case reached the comparison's 64 slices (%u)\n", max_slices);
        return 1;
    }
    if (policy_cases(n_policy) != 0)
        return 1;
    printf("ok: %ld shapes, %ld of them refused, %ld policy cases\n", n_cases, n_refused, n_policy);
    return 0;
}
