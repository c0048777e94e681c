/* The folded log-add table of the batch senone kernel (csrc/ssw_senone_lds.inc: senone_fold_hb,
 * senone_fold_table) on the CPU.
 *
 *   senone_fold_host table TAB WMAX SIZE OUT
 *       TAB = a file of 256 bytes (a log-add table); writes the SIZE bytes of the folded table to
 *       OUT and prints `hb N`.  With hb > 255 nothing is written (the host refuses such a table).
 *   senone_fold_host chains TAB WMAX MS
 *       ptm_senone_kernel's chain arithmetic (quad_chains and stage_item, restated below with the
 *       same 32-bit and packed 16-bit operations) against the reference's step
 *       x <- min(x, y) - tab[|x - y|] (tied_mgau_common.h:100-117), one slot pair and three
 *       streams at a time: the extremes (all weights 0, all WMAX, 0 beside WMAX, relative scores
 *       0 and the clamp, in every combination over the four codewords) and two million seeded
 *       random pairs.  The range claims of the fold are asserted on the way: the look-up address
 *       inside the table, every entry read a byte that the builder wrote, the running halves
 *       below 2^16.  MS = 1: the ms instance (table twice as long, relative scores up to 640, the
 *       accumulator's start value below zero as well as above).  Last line: `ok: N pairs`.
 * Built with -fsanitize=address,undefined. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../soundswallower_amd/csrc/ssw_senone_lds.inc"

#define FAIL(...)                                                                            \
    do {                                                                                     \
        printf("FAILED: ");                                                                  \
        printf(__VA_ARGS__);                                                                 \
        printf("\n");                                                                        \
        exit(1);                                                                             \
    } while (0)

static unsigned char g_tab[256];

static void
read_tab(const char *path)
{
    FILE *fh = fopen(path, "rb");
    if (fh == NULL || fread(g_tab, 1, 256, fh) != 256)
        FAIL("cannot read 256 bytes from %s", path);
    fclose(fh);
}

static int
ref_step(int x, int y)
{
    const int d = x > y ? x - y : y - x;
    return (x < y ? x : y) - (d < 256 ? (int)g_tab[d] : 0);
}

/* v_pk_add_u16 with one half of b in both lanes */
static uint32_t
pk_add_bcast(uint32_t a, uint32_t b16)
{
    return ((a + b16) & 0xffffu) | ((((a >> 16) + b16) & 0xffffu) << 16);
}

struct Pair {
    int nf;
    int w[8][4][2]; /* [stream][codeword][slot of the pair] */
    int rel[8][4];  /* relative to the best codeword: rel[.][0] = 0 */
    int e0[8];      /* PTM: the best codeword's normalised score */
    int norm;       /* MS: sum of fden_0 over the streams */
};

struct Fold {
    int ms, wmax, hb, T, size, cz;
    std::vector<unsigned char> tab;
    long n_pairs = 0, n_neg_start = 0, n_marked = 0, n_dmax = 0, n_dzero2 = 0, n_dlow = 0;
};

static void
run_pair(Fold &F, const Pair &P)
{
    /* stage_item */
    uint32_t acc;
    bool marked = false;
    if (F.ms) {
        const int a0n = -P.norm - 3 * F.hb * P.nf;
        const int a0 = -P.norm - 3 * F.T * P.nf;
        marked = a0 < 0 || a0 > 30000;
        acc = (uint32_t)(a0n & 0xffff) | (uint32_t)((a0n - (a0n < 0 ? 1 : 0)) & 0xffff) << 16;
        F.n_neg_start += a0n < 0 && !marked;
    } else {
        acc = 0;
        for (int f = 0; f < P.nf; ++f)
            acc += (uint32_t)P.e0[f] * 0x10001u;
    }
    int ref[2] = { 0, 0 };
    for (int f = 0; f < P.nf; ++f) {
        /* quad_chains, one chain */
        uint32_t x2 = (uint32_t)P.w[f][0][0] | (uint32_t)P.w[f][0][1] << 16;
        int rx[2] = { P.w[f][0][0], P.w[f][0][1] };
        for (int k = 1; k < 4; ++k) {
            const uint32_t npz = (uint32_t)(F.cz - P.rel[f][k] - F.hb * (k - 1)) & 0xffffu;
            const uint32_t z = pk_add_bcast(x2, npz);
            const uint32_t a[2] = { (z & 0xffffu) - (uint32_t)P.w[f][k][0],
                                    (z >> 16) - (uint32_t)P.w[f][k][1] };
            int dd[2];
            for (int s = 0; s < 2; ++s) {
                const int y = P.w[f][k][s] + P.rel[f][k];
                dd[s] = rx[s] - y;
                if (a[s] != (uint32_t)(F.cz + dd[s]))
                    FAIL("address %u, cz + d = %d", a[s], F.cz + dd[s]);
                if (a[s] >= (uint32_t)F.size)
                    FAIL("address %u beyond the table's %d bytes", a[s], F.size);
                if (dd[s] > F.wmax)
                    FAIL("d = %d beyond wmax = %d", dd[s], F.wmax);
                rx[s] = ref_step(rx[s], y);
            }
            F.n_dmax += dd[0] == F.wmax || dd[1] == F.wmax;
            F.n_dzero2 += dd[0] == 0 && dd[1] == 0;
            F.n_dlow += dd[0] <= -(F.wmax + (F.ms ? 640 : 96)) || dd[1] <= -(F.wmax + (F.ms ? 640 : 96));
            x2 = x2 + F.tab[a[0]] + ((uint32_t)F.tab[a[1]] << 16);
            for (int s = 0; s < 2; ++s) {
                const int half = (int)((x2 >> (16 * s)) & 0xffffu);
                if (half != rx[s] + F.hb * k)
                    FAIL("step %d: half %d, reference %d + %d", k, half, rx[s], F.hb * k);
            }
        }
        acc += x2;
        for (int s = 0; s < 2; ++s)
            ref[s] += rx[s] + (F.ms ? 0 : P.e0[f]);
    }
    ++F.n_pairs;
    if (marked) { /* the kernel redoes the frame with the reference's own arithmetic */
        ++F.n_marked;
        return;
    }
    for (int s = 0; s < 2; ++s) {
        const int got = (int)((acc >> (16 * s)) & 0xffffu);
        const int want = F.ms ? ref[s] - P.norm : ref[s] + 3 * F.hb * P.nf;
        if (got != want || want >= 32768)
            FAIL("slot %d ends at %d, the reference at %d (ms %d norm %d)", s, got, want, F.ms, P.norm);
    }
}

static uint32_t g_seed = 20261021u;
static uint32_t
rnd(uint32_t n)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (uint32_t)(((uint64_t)(g_seed >> 8) * n) >> 24);
}

static int
chains(const char *tabfile, int wmax, int ms)
{
    read_tab(tabfile);
    Fold F;
    F.ms = ms;
    F.wmax = wmax;
    F.hb = senone_fold_hb(g_tab, wmax);
    F.T = 0;
    for (int i = 0; i < 256; ++i)
        F.T = g_tab[i] > F.T ? g_tab[i] : F.T;
    F.size = (ms ? 2 : 1) * SSW_LOGADD_MIRROR;
    F.cz = F.size / 2;
    if (F.hb > 255)
        FAIL("hb = %d: the host refuses this table", F.hb);
    F.tab.assign((size_t)F.size, 0);
    senone_fold_table(g_tab, wmax, F.hb, F.size, F.tab.data());
    const int relmax = ms ? 640 : 96;
    /* where the accumulator of the ms instance starts: around 0 for the old and the new offset,
     * a typical value, and the upper guard */
    const int norms[] = { 0, -3 * 3 * F.T + 1, -3 * 3 * F.T, -3 * 3 * F.hb + 1, -3 * 3 * F.hb,
                          -3 * 3 * F.hb - 1, -700, -2500, -30000 - 3 * 3 * F.T, -30001 - 3 * 3 * F.T,
                          -29000 };
    const int n_norm = ms ? (int)(sizeof(norms) / sizeof(norms[0])) : 1;
    Pair P;
    memset(&P, 0, sizeof(P));
    P.nf = 3;
    /* extremes: per codeword the pair's weights (0 0, W W, 0 W, W 0) and its relative score (0
     * or the clamp), the same in the three streams */
    const int wv[4][2] = { { 0, 0 }, { wmax, wmax }, { 0, wmax }, { wmax, 0 } };
    for (int code = 0; code < 4 * 4 * 4 * 4 * 8; ++code) {
        int c = code;
        for (int k = 0; k < 4; ++k, c >>= 2)
            for (int f = 0; f < 3; ++f) {
                P.w[f][k][0] = wv[c & 3][0];
                P.w[f][k][1] = wv[c & 3][1];
            }
        for (int k = 1; k < 4; ++k, c >>= 1)
            for (int f = 0; f < 3; ++f)
                P.rel[f][k] = (c & 1) ? relmax : 0;
        for (int e = 0; e < 2; ++e)
            for (int ni = 0; ni < n_norm; ++ni) {
                for (int f = 0; f < 3; ++f)
                    P.e0[f] = ms ? 0 : e * 96;
                P.norm = ms ? norms[ni] : 0;
                run_pair(F, P);
            }
    }
    for (long i = 0; i < 2000000; ++i) {
        for (int f = 0; f < 3; ++f) {
            int prev = 0;
            for (int k = 0; k < 4; ++k) {
                for (int s = 0; s < 2; ++s) {
                    const uint32_t r = rnd(8);
                    P.w[f][k][s] = r == 0 ? 0 : r == 1 ? wmax : (int)rnd((uint32_t)wmax + 1);
                }
                /* sorted, as the top-N block is; ties and the clamp are common */
                if (k > 0) {
                    const uint32_t r = rnd(4);
                    prev = r == 0 ? prev : r == 1 ? relmax : prev + (int)rnd((uint32_t)(relmax - prev) + 1);
                    P.rel[f][k] = prev;
                }
            }
            P.e0[f] = ms ? 0 : (int)rnd((uint32_t)(96 - P.rel[f][3]) + 1);
        }
        P.norm = ms ? (rnd(4) == 0 ? norms[rnd((uint32_t)n_norm)] : -(int)rnd(31000)) : 0;
        run_pair(F, P);
    }
    if (F.n_dmax == 0 || F.n_dzero2 == 0 || F.n_dlow == 0)
        FAIL("the extremes did not occur: d = wmax %ld, d = 0 twice %ld, low end %ld", F.n_dmax,
             F.n_dzero2, F.n_dlow);
    if (ms && (F.n_neg_start == 0 || F.n_marked == 0))
        FAIL("ms: start below zero %ld, marked %ld", F.n_neg_start, F.n_marked);
    printf("hb %d wmax %d ms %d: d = wmax %ld, d = 0 in both halves %ld, low end %ld, start below "
           "zero %ld, marked %ld\n", F.hb, wmax, ms, F.n_dmax, F.n_dzero2, F.n_dlow, F.n_neg_start,
           F.n_marked);
    printf("ok: %ld pairs\n", F.n_pairs);
    return 0;
}

int
main(int argc, char **argv)
{
    if (argc == 6 && strcmp(argv[1], "table") == 0) {
        read_tab(argv[2]);
        const int wmax = atoi(argv[3]), size = atoi(argv[4]);
        const int hb = senone_fold_hb(g_tab, wmax);
        if (hb <= 255) {
            std::vector<unsigned char> out((size_t)size);
            senone_fold_table(g_tab, wmax, hb, size, out.data());
            FILE *fh = fopen(argv[5], "wb");
            if (fh == NULL || fwrite(out.data(), 1, out.size(), fh) != out.size())
                FAIL("cannot write %s", argv[5]);
            fclose(fh);
        }
        printf("hb %d\n", hb);
        return 0;
    }
    if (argc == 5 && strcmp(argv[1], "chains") == 0)
        return chains(argv[2], atoi(argv[3]), atoi(argv[4]));
    fprintf(stderr, "usage: %s table TAB WMAX SIZE OUT | chains TAB WMAX MS\n", argv[0]);
    return 2;
}
