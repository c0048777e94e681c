/* fp_shape (csrc/ssw_fp_shape.inc) on the CPU against the loops it was moved out of, kept here
 * verbatim as they stood in first_pass_run_impl (the sizing loops and the kernel choice chain;
 * the model, the graphs and the kernels bound to stand-ins, `runs` handed in where the parent
 * built it from `only` just above, the export flag where it read the model's borrowed pointer).  Every output, on synthetic offset tables: node counts at
 * 256/257, 512/513, 1024/1025; an LDS size one int below, at and one int above 160 * 1024 - 512
 * bytes; levels 0, 1, 2; the kernel forced big or not; the window and big threads-per-block
 * knobs 256 / 512 / 1024 / other; history band default, 1 and 512 with fewer and with more
 * word-final HMMs than the band; an utterance of 0 frames; `runs` all, some and none; export on
 * and off; the 2^31 refusal at the boundary.  Built with -fsanitize=address,undefined
 * (tests/test_fp_shape_host.py); the tables have exactly the size fp_shape may read. */
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../soundswallower_amd/csrc/ssw_fp_shape.inc"

/* ---- stand-ins for what the parent's code names ---- */
struct RefGraphs {
    const int *node_off, *leaf_off, *state_off, *tw_off, *tw_rk;
};
struct RefKnobs {
    const char *fp_kernel;
    int fp_hist_band, fp_big_tpb, fp_win_tpb;
};
struct RefModel {
    RefKnobs kn;
};
struct FirstPassParams {
    int hist_band;
};
/* (every instance a body of its own: no two of them may share an address) */
static volatile int kernel_ran;
template <int TPB, bool EXPORT = false> static void first_pass_kernel(FirstPassParams) { kernel_ran = 10000 + 2 * TPB + EXPORT; }
template <int TPB, bool BAND> static void first_pass_big_kernel(FirstPassParams) { kernel_ran = 20000 + 2 * TPB + BAND; }
template <int TPB> static void first_pass_win_kernel(FirstPassParams) { kernel_ran = 30000 + TPB; }

static char ref_error[256];
static void
ssw_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ref_error, sizeof(ref_error), fmt, ap);
    va_end(ap);
}

struct RefShape {
    std::vector<long long> hist_off, big_off;
    size_t hist_total, big_ints, hist_band, lds_launch;
    bool big, band, clear;
    void (*kern)(FirstPassParams);
    int tpb;
};

static int
reference_shape(const RefModel *m, const RefGraphs *g, const int32_t *utt_off, int32_t n_utts,
                const std::vector<char> &runs, int level, bool export_on, RefShape &out)
{
    /* ---- the parent's sizing loops, verbatim ---- */
    bool band = level >= 1;
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
    if (!big)
        big_ints = 0;
    /* ---- and its kernel choice chain, verbatim ---- */
        void (*kern)(FirstPassParams);
        int tpb;
        size_t lds_launch = lds_bytes;
        const bool exp = export_on; /* (the parent read the export pointer it had lent the model) */
        if (big) {
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
    /* ---- */
    out.hist_off = hist_off;
    out.big_off = big_off;
    out.hist_total = hist_total;
    out.big_ints = big_ints;
    out.hist_band = hist_band;
    out.lds_launch = lds_launch;
    out.big = big;
    out.band = band;
    out.clear = exp && big; /* (the parent: `if (.. exp && big)` ahead of fpa_clear_kernel) */
    out.kern = kern;
    out.tpb = tpb;
    return 0;
}

/* the kernel instance fp_launch maps a shape to, as the stand-ins' addresses */
static void (*kernel_of(const FpShape &S, bool exp))(FirstPassParams)
{
    const int t = S.tpb;
    if (S.kind == FP_WIN)
        return t == 1024 ? first_pass_win_kernel<1024> : t == 512 ? first_pass_win_kernel<512> : first_pass_win_kernel<256>;
    if (S.kind == FP_HBM_BAND)
        return t == 1024 ? first_pass_big_kernel<1024, true>
            : t == 512   ? first_pass_big_kernel<512, true>
                         : first_pass_big_kernel<256, true>;
    if (S.kind == FP_HBM)
        return first_pass_big_kernel<1024, false>;
    if (t == 256)
        return exp ? first_pass_kernel<256, true> : first_pass_kernel<256>;
    if (t == 512)
        return exp ? first_pass_kernel<512, true> : first_pass_kernel<512>;
    return exp ? first_pass_kernel<1024, true> : first_pass_kernel<1024>;
}

struct Utt {
    int nn, nl, ns, tw, rk, frames;
};

#define FAIL(...)                                                                             \
    do {                                                                                      \
        printf("FAILED batch %zu level %d big %d win_tpb %d big_tpb %d band %d runs %d exp %d: ", b, level, \
               force, wt, bt, hb, rmode, exp);                                                \
        printf(__VA_ARGS__);                                                                  \
        printf("\n");                                                                         \
        return 1;                                                                             \
    } while (0)

int
main()
{
    const Utt small = { 10, 3, 4, 0, 0, 20 }, none = { 10, 3, 4, 0, 0, 0 };
    std::vector<std::vector<Utt>> batches;
    for (int nn : { 256, 257, 512, 513, 1024, 1025 })
        batches.push_back({ small, Utt{ nn, nn / 4, nn / 4 + 1, 8, 2, 50 } });
    /* 3 * 1000 + 4 * 500 + 2 * 501 = 6002 ints, the rest in the twins' tables: 40832 ints are
     * 160 * 1024 - 512 bytes */
    for (int li : { 40831, 40832, 40833 })
        batches.push_back({ small, Utt{ 1000, 500, 501, li - 6002 - 3, 3, 50 } });
    /* a batch of several: 0 frames, fewer and more word-final HMMs than a band of 512 (and of 1) */
    batches.push_back({ small, Utt{ 1500, 700, 701, 12, 1, 0 }, Utt{ 300, 1, 2, 0, 0, 33 },
                        Utt{ 2000, 700, 650, 40, 5, 100 } });
    /* the history table's 2^31 entries: 2^31 - 1 is prime, so 1 x (2^31 - 1) is the boundary */
    batches.push_back({ none, Utt{ 4, 1, 2, 0, 0, INT_MAX - 1 } });
    batches.push_back({ none, Utt{ 4, 1, 2, 0, 0, INT_MAX } });
    batches.push_back({ none, Utt{ 4, 2, 2, 0, 0, (INT_MAX - 1) / 2 } });
    batches.push_back({ none, Utt{ 4, 2, 2, 0, 0, (INT_MAX - 1) / 2 + 1 } });
    long n_cases = 0, n_refused = 0;
    for (size_t b = 0; b < batches.size(); ++b) {
        const std::vector<Utt> &B = batches[b];
        const int n_utts = (int)B.size();
        /* exactly what fp_shape may read: [n_utts + 1] offsets, [n_utts] tw_rk and runs */
        std::vector<int> node_off(1, 0), leaf_off(1, 0), state_off(1, 0), tw_off(1, 0), utt_off(1, 0), tw_rk;
        for (const Utt &u : B) {
            node_off.push_back(node_off.back() + u.nn);
            leaf_off.push_back(leaf_off.back() + u.nl);
            state_off.push_back(state_off.back() + u.ns);
            tw_off.push_back(tw_off.back() + u.tw);
            utt_off.push_back(utt_off.back() + u.frames);
            tw_rk.push_back(u.rk);
        }
        const RefGraphs rg = { node_off.data(), leaf_off.data(), state_off.data(), tw_off.data(), tw_rk.data() };
        const FpGraphSizes gs = { node_off.data(), leaf_off.data(), state_off.data(), tw_off.data(), tw_rk.data() };
        for (int level = 0; level <= 2; ++level)
            for (int force = 0; force < 2; ++force)
                for (int wt : { 256, 512, 1024, 300 })
                    for (int bt : { 256, 512, 1024, 2000 })
                        for (int hb : { 0, 1, 512 })
                            for (int rmode = 0; rmode < 3; ++rmode) /* all, some (the odd ones), none */
                                for (int exp = 0; exp < 2; ++exp) {
                                    std::vector<char> runs((size_t)n_utts);
                                    for (int u = 0; u < n_utts; ++u)
                                        runs[(size_t)u] = rmode == 0 ? 1 : rmode == 1 ? (char)(u & 1) : 0;
                                    const RefModel m = { { force ? "big" : "", hb, bt, wt } };
                                    RefShape want;
                                    ref_error[0] = 0;
                                    const int rc_want = reference_shape(&m, &rg, utt_off.data(), n_utts, runs, level, exp != 0, want);
                                    const FpKnobs kn = { force != 0, hb, bt, wt };
                                    FpShape S;
                                    const int rc = fp_shape(gs, utt_off.data(), n_utts, runs.data(), level, kn, exp != 0, S);
                                    ++n_cases;
                                    if (rc != rc_want)
                                        FAIL("returns %d, the parent's loops %d", rc, rc_want);
                                    if (rc < 0) {
                                        if (strcmp(S.err, ref_error) != 0)
                                            FAIL("message '%s', the parent's '%s'", S.err, ref_error);
                                        ++n_refused;
                                        continue;
                                    }
                                    if (S.hist_off != want.hist_off || S.big_off != want.big_off)
                                        FAIL("hist_off / big_off differ");
                                    if (S.hist_total != want.hist_total || S.big_ints != want.big_ints)
                                        FAIL("hist_total %zu (%zu), big_ints %zu (%zu)", S.hist_total,
                                             want.hist_total, S.big_ints, want.big_ints);
                                    if (S.big != want.big || S.band != want.band || (size_t)S.hist_band != want.hist_band)
                                        FAIL("big %d (%d), band %d (%d), hist_band %d (%zu)", S.big, want.big,
                                             S.band, want.band, S.hist_band, want.hist_band);
                                    if (S.tpb != want.tpb || S.lds_bytes != want.lds_launch || S.clear_mask != want.clear)
                                        FAIL("tpb %d (%d), LDS bytes %zu (%zu), clear %d (%d)", S.tpb, want.tpb,
                                             S.lds_bytes, want.lds_launch, S.clear_mask, want.clear);
                                    if (kernel_of(S, exp != 0) != want.kern)
                                        FAIL("kind %d x %d threads is another kernel instance", S.kind, S.tpb);
                                }
    }
    if (n_refused == 0) {
        printf("FAILED: no case reached the 2^31 refusal\n");
        return 1;
    }
    printf("ok: %ld shapes, %ld of them refused\n", n_cases, n_refused);
    return 0;
}
