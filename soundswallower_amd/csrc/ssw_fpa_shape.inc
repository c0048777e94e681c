/* ssw_fpa_shape.inc -- host: what one call of the default configuration's loop of speculation and
 * proof (fpa_run, ssw_host_fpactive.inc) takes -- the layout of the exported sets, the list
 * capacity, the LDS of its two per-frame kernels and the refusal beyond a CU's -- and the policy of
 * its rounds, each formula once.  Plain C++17, no HIP header: ssw_kernels.hip includes it ahead of
 * the ssw_host_*.inc files, and a host program can include it on its own behind
 * ssw_senone_lds.inc, whose carves it sizes the LDS from (tests/harness/fpa_shape_host.cpp).
 * Reads no environment, names no kernel. */
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <vector>

#define SSW_FPA_LDS_LIMIT (156 * 1024) /* of a CU's 160 KB, per workgroup */

enum FpaScorerKind {
    FPA_PTM,  /* senone_listed_kernel<false>: a wave keeps every (codebook, stream)'s scores */
    FPA_MS,   /* senone_listed_kernel<true> */
    FPA_CONT, /* cont_listed_kernel: a continuous model, whatever the scorer */
};

/* what the shape needs of the model */
struct FpaModelSizes {
    int kind;    /* FpaScorerKind */
    int n_sen;
    int n_cbf;   /* codebooks x streams (PTM) */
    int featdim; /* floats of a frame (continuous) */
};

struct FpaShape {
    int nw32;                      /* 32-bit words of a senone bitmap */
    std::vector<long long> act_off; /* [n_utts]: the utterance's first 64-bit word of the exported
                                       sets, [n_frames_u][ceil(N_u / 64)] words each */
    long long mask_words;          /* their total */
    int max_nodes;                 /* the most HMMs of an utterance, at least the caller's bound */
    int max_len;                   /* the most frames of an utterance */
    int cap;                       /* senones a frame may list */
    size_t plan_lds, sen_lds;      /* dynamic LDS of the plan kernel and of the listed scorer */
    size_t n_start_words;          /* the batch's utterance-start bits (two-pass history) ... */
    size_t start_bytes;            /* ... and the space they take: none without the carry */
    char err[240];                 /* the refusal, when fpa_shape returns -1 */
};

/* a frame lists at most three senones per HMM plus the bridges between them (even: the plan
 * kernel's LDS words behind the list stay 4-byte aligned) */
static inline int
fpa_cap(int n_sen, int max_nodes)
{
    return ((int)std::min<long long>(n_sen, 3ll * max_nodes + n_sen / 255 + 2) + 1) & ~1;
}

/* the listed scorer's dynamic LDS for lists of up to `cap` senones */
static inline size_t
fpa_listed_lds(const FpaModelSizes &M, int cap)
{
    return M.kind == FPA_CONT ? ContListedCarve(M.featdim, cap).bytes()
                              : ListedCarve(M.kind == FPA_MS, M.n_cbf, cap).bytes();
}

/* node_cnt [n_utts]: every utterance's phone-tree HMMs; max_nodes: the caller's bound (a plan's
 * largest grammar), 0 for none; carry: the call hands the carried orders on (d_carry_out) */
static inline int
fpa_shape(const char *who, const FpaModelSizes &M, const int *node_cnt, int max_nodes,
          const int *utt_off, int n_utts, int n_frames, bool carry, FpaShape &S)
{
    S.nw32 = (M.n_sen + 31) / 32;
    S.act_off.assign((size_t)n_utts, 0);
    S.mask_words = 0;
    S.max_nodes = max_nodes;
    S.max_len = 0;
    S.err[0] = 0;
    for (int u = 0; u < n_utts; ++u) {
        const int nn = node_cnt[u], len = utt_off[u + 1] - utt_off[u];
        S.act_off[(size_t)u] = S.mask_words;
        S.mask_words += (long long)len * ((nn + 63) / 64);
        S.max_nodes = std::max(S.max_nodes, nn);
        S.max_len = std::max(S.max_len, len);
    }
    S.cap = fpa_cap(M.n_sen, S.max_nodes);
    /* what the two per-frame kernels keep in LDS per wave (four waves a workgroup) */
    S.plan_lds = FpaPlanCarve(S.nw32, S.cap).bytes();
    S.sen_lds = fpa_listed_lds(M, S.cap);
    S.n_start_words = (size_t)std::max(n_frames, 1) / 32 + 2;
    S.start_bytes = carry ? sizeof(unsigned) * S.n_start_words : 0;
    const size_t lds = std::max(S.plan_lds, S.sen_lds);
    if (lds > SSW_FPA_LDS_LIMIT) {
        snprintf(S.err, sizeof(S.err), "%s: %d senones x texts of up to %d phone-tree "
                                       "HMMs need %zu KB of LDS per workgroup (160 KB a CU)", who, M.n_sen,
                 S.max_nodes, lds / 1024);
        return -1;
    }
    return 0;
}

/* the comparison's slices of an utterance's words: enough workgroups for a single long utterance,
 * few for a batch of short ones */
static inline unsigned
fpa_compare_slices(long long mask_words, int n_cmp)
{
    return (unsigned)std::min<long long>(64, std::max<long long>(1, mask_words / std::max(1, n_cmp) / (256 * 16)));
}

/* The rounds' policy, from the count of utterances still unproven (n_only, 0 = a round over the
 * whole batch) and SSW_FPA_SUB (fpa_sub: 1 always one by one, 0 never, else by count).
 * Few unproven utterances left: they are scored one by one -- at most four, or a quarter of the
 * batch (a batch of one long utterance is "few") -- else the whole batch again. */
static inline bool
fpa_one_by_one(size_t n_only, int n_utts, int fpa_sub)
{
    return n_only != 0 && (fpa_sub == 1 || (fpa_sub != 0 && (int)n_only <= std::max(4, n_utts / 4)));
}

/* every utterance goes round again, and they are more than four: the whole batch as a whole */
static inline bool
fpa_whole_batch(size_t n_again, int n_utts, int fpa_sub)
{
    return (int)n_again == n_utts && n_utts > 4 && fpa_sub != 1;
}

/* the next round's `only` from the utterances that were not proven (ascending) */
static inline void
fpa_next_only(std::vector<int> &only, std::vector<int> &again, int n_utts, int fpa_sub)
{
    only.swap(again);
    if (fpa_whole_batch(only.size(), n_utts, fpa_sub))
        only.clear();
}
