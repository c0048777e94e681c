/* xcd_cut (csrc/ssw_xcd_cut.inc) on the CPU against the loop it was moved out of, kept here
 * verbatim as it stood in score_batch_impl's launch_scan (its model and parameter-block names
 * bound to locals).  All ten ints, for n_cbf in {1, 3, 7, 126} x tile_groups in {1, 2, 5, 64} x
 * both balance modes, on seeded random exact-list counts 0 .. 128, all-zero and all-equal ones.
 * Built with -fsanitize=address,undefined (tests/test_xcd_cut_host.py); the counts have exactly
 * the size the cut may read, so an overrun is an ASan report. */
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../soundswallower_amd/csrc/ssw_xcd_cut.inc"

#define SSW_EXLIST_STRIDE 132

static uint32_t rng_state = 0x5eed2026u;
static uint32_t
rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

/* what the reference loop reads of the model, the host model and the parameter block */
struct RefHost {
    const uint32_t *exlistm;
};
struct RefModel {
    int n_cbf;
};
struct RefParams {
    int tile_groups;
};

static std::array<int, 10>
reference_cut(const RefModel *m, const RefHost *h, const RefParams &F, bool mfma_balance)
{
    /* ---- the parent's loop, verbatim ---- */
                    const bool by_cost = mfma_balance;
                    const int n_pairs = m->n_cbf * F.tile_groups;
                    std::array<int, 10> cut;
                    double total = 0.0;
                    for (int c = 0; c < m->n_cbf; ++c)
                        total += (1400.0 + (by_cost ? 45.0 * h->exlistm[(size_t)c * SSW_EXLIST_STRIDE] : 0.0))
                            * F.tile_groups;
                    double acc = 0.0;
                    int x = 1;
                    cut[0] = 0;
                    for (int c = 0; c < m->n_cbf; ++c) {
                        const double w = 1400.0
                            + (by_cost ? 45.0 * h->exlistm[(size_t)c * SSW_EXLIST_STRIDE] : 0.0);
                        for (int g = 0; g < F.tile_groups; ++g) {
                            /* the pair goes to the chunk its middle falls into */
                            while (x < 8 && acc + 0.5 * w >= total * x / 8.0)
                                cut[x++] = c * F.tile_groups + g;
                            acc += w;
                        }
                    }
                    while (x <= 8)
                        cut[x++] = n_pairs;
                    cut[9] = 0;
                    for (int k = 0; k < 8; ++k)
                        if (cut[k + 1] - cut[k] > cut[9])
                            cut[9] = cut[k + 1] - cut[k];
    /* ---- */
    return cut;
}

int
main()
{
    static const int cbfs[] = { 1, 3, 7, 126 }, groups[] = { 1, 2, 5, 64 };
    long n_cases = 0;
    for (int n_cbf : cbfs)
        for (int tg : groups)
            for (int balance = 0; balance < 2; ++balance)
                for (int fill = 0; fill < 8; ++fill) { /* 0: all zero, 1: all equal, else random */
                    /* exactly what the cut may read: the last codebook's count is the last word */
                    const size_t n = (size_t)(n_cbf - 1) * SSW_EXLIST_STRIDE + 1;
                    std::vector<uint32_t> counts(n, 0xdeadbeefu);
                    const uint32_t same = rnd() % 129;
                    for (int c = 0; c < n_cbf; ++c)
                        counts[(size_t)c * SSW_EXLIST_STRIDE] = fill == 0 ? 0 : fill == 1 ? same : rnd() % 129;
                    const RefModel m{ n_cbf };
                    const RefHost h{ counts.data() };
                    const RefParams F{ tg };
                    const std::array<int, 10> want = reference_cut(&m, &h, F, balance != 0);
                    const std::array<int, 10> got
                        = xcd_cut(n_cbf, tg, counts.data(), SSW_EXLIST_STRIDE, balance != 0);
                    for (int k = 0; k < 10; ++k)
                        if (got[k] != want[k]) {
                            printf("FAILED n_cbf %d tile_groups %d balance %d fill %d: cut[%d] = %d, "
                                   "the parent's loop gives %d\n", n_cbf, tg, balance, fill, k, got[k], want[k]);
                            return 1;
                        }
                    /* what the scan kernel relies on: the chunks tile [0, n_pairs) in order */
                    bool ok = got[0] == 0 && got[8] == n_cbf * tg;
                    int longest = 0;
                    for (int k = 0; k < 8; ++k) {
                        ok = ok && got[k] <= got[k + 1];
                        longest = got[k + 1] - got[k] > longest ? got[k + 1] - got[k] : longest;
                    }
                    if (!ok || longest != got[9]) {
                        printf("FAILED n_cbf %d tile_groups %d balance %d fill %d: the chunks do not tile "
                               "the pairs\n", n_cbf, tg, balance, fill);
                        return 1;
                    }
                    ++n_cases;
                }
    printf("ok: %ld cuts\n", n_cases);
    return 0;
}
