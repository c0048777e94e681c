/* ssw_xcd_cut.inc -- host: the matrix-core scan's work cut into one chunk per XCD.  Plain C++17,
 * no HIP header: ssw_kernels.hip includes it ahead of the ssw_host_*.inc files, and a host
 * program can include it on its own (tests/harness/xcd_cut_host.cpp). */
#include <array>
#include <cstddef>
#include <cstdint>

/* Eight contiguous chunks of (codebook x stream, tile group) pairs, one per XCD, equal in COST:
 * ~1,400 vector instructions per wave and 64-frame step plus ~45 per density its codebook leaves
 * to the exact form (by_cost = false, SSW_MFMA_BALANCE=0: equal counts).  Pairs are numbered
 * c * tile_groups + g; exact_count[c * stride] = the densities codebook x stream c leaves to the
 * exact form.  Returns cut[0..8] = the first pair of every chunk and the end of the last,
 * cut[9] = the longest chunk. */
static inline std::array<int, 10>
xcd_cut(int n_cbf, int tile_groups, const uint32_t *exact_count, size_t stride, bool by_cost)
{
    const int n_pairs = n_cbf * tile_groups;
    std::array<int, 10> cut;
    double total = 0.0;
    for (int c = 0; c < n_cbf; ++c)
        total += (1400.0 + (by_cost ? 45.0 * exact_count[(size_t)c * stride] : 0.0)) * tile_groups;
    double acc = 0.0;
    int x = 1;
    cut[0] = 0;
    for (int c = 0; c < n_cbf; ++c) {
        const double w = 1400.0 + (by_cost ? 45.0 * exact_count[(size_t)c * stride] : 0.0);
        for (int g = 0; g < tile_groups; ++g) {
            /* the pair goes to the chunk its middle falls into */
            while (x < 8 && acc + 0.5 * w >= total * x / 8.0)
                cut[x++] = c * tile_groups + g;
            acc += w;
        }
    }
    while (x <= 8)
        cut[x++] = n_pairs;
    cut[9] = 0;
    for (int k = 0; k < 8; ++k)
        if (cut[k + 1] - cut[k] > cut[9])
            cut[9] = cut[k + 1] - cut[k];
    return cut;
}
