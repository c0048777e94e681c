/* ssw_fp_shape.inc -- host: what one launch of the first pass takes -- sizes, kernel kind, launch
 * shape -- from the graphs' offset tables and the knob values.  Plain C++17, no HIP header:
 * ssw_kernels.hip includes it ahead of the ssw_host_*.inc files, and a host program can include
 * it on its own (tests/harness/fp_shape_host.cpp).  Reads no environment, names no kernel. */
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <vector>

#define SSW_FP_HIST_BAND 512 /* banded history table: word-final HMMs per frame, on average */

/* the offset tables of a batch's graphs (ssw_fp_graphs_t), [n_utts + 1] but tw_rk [n_utts] */
struct FpGraphSizes {
    const int *node_off, *leaf_off, *state_off, *tw_off, *tw_rk;
};

struct FpKnobs {
    bool force_big; /* SSW_FP_KERNEL=big */
    int hist_band;  /* SSW_FP_HIST_BAND, <= 0: the default */
    int big_tpb;    /* SSW_FP_BIG_TPB */
    int win_tpb;    /* SSW_FP_WIN_TPB */
};

enum FpKind {
    FP_REG,      /* first_pass_kernel: HMMs in registers, one per thread */
    FP_WIN,      /* first_pass_win_kernel: a sliding window of nodes, banded history */
    FP_HBM,      /* first_pass_big_kernel<1024, false>: node state in HBM, full history table */
    FP_HBM_BAND, /* first_pass_big_kernel<.., true>: the same, banded */
};

/* one utterance's sizes, every formula once */
struct FpUttSizes {
    size_t nn, nl, ns, tw; /* phone-tree HMMs, word-final ones, states, twin ints (tw + rk) */

    FpUttSizes(const FpGraphSizes &g, int u)
        : nn((size_t)(g.node_off[u + 1] - g.node_off[u])), nl((size_t)(g.leaf_off[u + 1] - g.leaf_off[u])),
          ns((size_t)(g.state_off[u + 1] - g.state_off[u])),
          tw((size_t)(g.tw_off[u + 1] - g.tw_off[u]) + (size_t)g.tw_rk[u])
    {
    }
    /* what first_pass_kernel keeps in LDS */
    size_t lds_ints() const { return 3 * nn + 4 * nl + 2 * ns + tw; }
    /* first_pass_big_kernel's workspace, see there (.. SFIRST LFIRST FBASE FLLO) */
    size_t hbm_ints(size_t frames) const
    {
        return 13 * nn + 5 * nl + 2 * ns + tw + 64 + 2 * (ns + 2) + 2 * frames + 2;
    }
    /* history entries: one per (frame, word-final HMM); banded, a budget of `band` entries per
     * frame (fewer if the text has fewer word-final HMMs) */
    size_t hist_entries(size_t frames) const { return nl * frames; }
    size_t hist_entries(size_t frames, size_t band) const { return std::min(nl, band) * frames; }
};

struct FpShape {
    std::vector<long long> hist_off, big_off; /* [n_utts], what the kernels read */
    size_t hist_total, big_ints;              /* entries of the history table, ints of the HBM workspace */
    bool big, band;
    int hist_band;
    int kind, tpb; /* FpKind, threads per block */
    size_t lds_bytes; /* dynamic LDS of the launch */
    bool clear_mask;  /* the exported sets must be cleared first (fpa_clear_kernel) */
    char err[160];    /* the refusal, when fp_shape returns -1 */
};

/* runs[u] != 0: utterance u is searched by this launch; the sizes of those alone pick the kernel
 * and size the workspaces.  level: 2 window, 1 HBM banded, 0 HBM with the full table (a level
 * above what the batch needs means nothing: a batch that fits a workgroup is searched in
 * registers).  exp: the sets of active HMMs are exported. */
static inline int
fp_shape(const FpGraphSizes &g, const int *utt_off, int n_utts, const char *runs, int level,
         const FpKnobs &kn, bool exp, FpShape &S)
{
    S.hist_off.assign((size_t)n_utts, 0);
    S.big_off.assign((size_t)n_utts, 0);
    S.hist_total = S.big_ints = 0;
    S.err[0] = 0;
    size_t lds_ints = 0, max_nodes = 0;
    S.big = kn.force_big;
    for (int u = 0; u < n_utts; ++u) {
        if (!runs[u])
            continue;
        const FpUttSizes z(g, u);
        /* beyond one HMM per thread of a 1024-thread workgroup the sliding-window kernel is the
         * faster one (32 texts, ms of first pass, registers / window: 970 HMMs 7.8 / 11.7, 1,167
         * 13.9 / 13.7, 1,564 18.7 / 15.3, 1,961 41 / 23, 2,940 69 / 31, 3,918 109 / 40 -- round 5;
         * the 2- and 4-HMMs-per-thread register instances, the ones that spilt, are gone) */
        S.big = S.big || z.lds_ints() * sizeof(int) > 160 * 1024 - 512 || z.nn > 1024;
    }
    S.band = level >= 1 && S.big;
    /* SSW_FP_HIST_BAND (tests): a budget small enough to overflow */
    S.hist_band = kn.hist_band > 0 ? kn.hist_band : SSW_FP_HIST_BAND;
    for (int u = 0; u < n_utts; ++u) {
        S.hist_off[(size_t)u] = (long long)S.hist_total;
        S.big_off[(size_t)u] = (long long)S.big_ints;
        if (!runs[u])
            continue;
        const FpUttSizes z(g, u);
        const size_t frames = (size_t)(utt_off[u + 1] - utt_off[u]);
        if (z.hist_entries(frames) >= (size_t)INT_MAX) { /* entry ids are int32 */
            snprintf(S.err, sizeof(S.err), "utterance %d: %zu word-final HMMs x %d frames exceed the history "
                                           "table's 2^31 entries", u, z.nl, utt_off[u + 1] - utt_off[u]);
            return -1;
        }
        S.hist_total += S.band ? z.hist_entries(frames, (size_t)S.hist_band) : z.hist_entries(frames);
        lds_ints = std::max(lds_ints, z.lds_ints());
        max_nodes = std::max(max_nodes, z.nn);
        S.big_ints += z.hbm_ints(frames);
    }
    /* a text beyond what one workgroup holds in registers and LDS (about 400 words) sends the
     * batch through the kernel that keeps the node state in HBM; SSW_FP_KERNEL=big forces it */
    if (!S.big)
        S.big_ints = 0;
    S.clear_mask = exp && S.big; /* the long-text kernels export only the words that hold an active HMM */
    S.lds_bytes = 0;
    if (S.band && level == 2) {
        /* window of 512 nodes unless told otherwise (256 / 512 / 1024) */
        S.kind = FP_WIN;
        S.tpb = kn.win_tpb >= 1024 ? 1024 : kn.win_tpb >= 512 ? 512 : 256;
    } else if (S.band) {
        /* banded: a frame walks a few hundred nodes, so a small workgroup (cheaper barriers
         * and reductions) is the faster one; SSW_FP_BIG_TPB = 256 / 512 / 1024 (tuning) */
        S.kind = FP_HBM_BAND;
        S.tpb = kn.big_tpb == 1024 ? 1024 : kn.big_tpb == 512 ? 512 : 256;
    } else if (S.big) {
        S.kind = FP_HBM;
        S.tpb = 1024;
    } else {
        /* one thread per HMM while a workgroup can hold them (more than 1024 nodes: `big` above) */
        S.kind = FP_REG;
        S.tpb = max_nodes <= 256 ? 256 : max_nodes <= 512 ? 512 : 1024;
        S.lds_bytes = lds_ints * sizeof(int);
    }
    return 0;
}
