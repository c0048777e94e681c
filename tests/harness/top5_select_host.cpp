// Host check of the scan's selection network (soundswallower_amd/csrc/ssw_top5_select.inc): the
// same text, compiled for the CPU with the three-input operations written in plain C (valid for
// non-NaN floats), against a full sort.  A lane of the scan sees 64 keys per column block -- four
// tiles of 16, each five triples and one leftover key -- whose low 7 bits are labels, so all keys
// are distinct.  tests/test_top5_select_host.py builds this with -fsanitize=address,undefined
// and runs it as a process of its own.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#define SSW_SEL_FN static inline
static inline float ssw_sel_max2(float a, float b) { return a > b ? a : b; }
static inline float ssw_sel_min2(float a, float b) { return a < b ? a : b; }
static inline float ssw_sel_max3(float a, float b, float c) { return ssw_sel_max2(ssw_sel_max2(a, b), c); }
static inline float ssw_sel_min3(float a, float b, float c) { return ssw_sel_min2(ssw_sel_min2(a, b), c); }
static inline float ssw_sel_med3(float a, float b, float c)
{
    return ssw_sel_max2(ssw_sel_min2(a, b), ssw_sel_min2(ssw_sel_max2(a, b), c));
}
#include "../../soundswallower_amd/csrc/ssw_top5_select.inc"

static const int NKEY = 64;
static long n_cases = 0;

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// label the keys the way the scan does (position = register + 16 x row block), run the network
// tile by tile, fold, and compare the list with the five largest of a full sort, bit for bit
static void check(const float (&raw)[NKEY], const char *what)
{
    float key[NKEY], sorted[NKEY];
    for (int i = 0; i < NKEY; ++i)
        sorted[i] = key[i] = float_of((bits_of(raw[i]) & 0xffffff80u) | (uint32_t)i);
    float H[5], M[2], Z;
    ssw_top5_reset(H, M, Z, -std::numeric_limits<float>::infinity());
    for (int t = 0; t < NKEY / 16; ++t) {
        float tile[16];
        for (int r = 0; r < 16; ++r)
            tile[r] = key[16 * t + r];
        ssw_top5_tile(H, M, Z, tile);
    }
    ssw_top5_fold(H, M, Z);
    std::partial_sort(sorted, sorted + 5, sorted + NKEY, [](float a, float b) { return a > b; });
    ++n_cases;
    for (int k = 0; k < 5; ++k)
        if (bits_of(H[k]) != bits_of(sorted[k])) {
            fprintf(stderr, "FAIL (%s, case %ld): rank %d is %.9g (label %u), a full sort gives %.9g (label %u)\n",
                    what, n_cases, k, H[k], bits_of(H[k]) & 127u, sorted[k], bits_of(sorted[k]) & 127u);
            for (int i = 0; i < NKEY; ++i)
                fprintf(stderr, "%s%.9g", i ? " " : "  keys: ", key[i]);
            fprintf(stderr, "\n");
            exit(1);
        }
}

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

// The five largest keys placed, in every order, on every 5 of the 9 consecutive positions from
// `start` on (wrapping at 64): with start a multiple of 3 inside a tile that is one triple and
// both its neighbours; the other starts straddle triples, the leftover 16th slot and the tile
// boundaries.  The 59 other keys lie below them, in an order that changes from case to case.
static void placements(int start)
{
    int pos[9];
    for (int i = 0; i < 9; ++i)
        pos[i] = (start + i) % NKEY;
    float raw[NKEY];
    int p[5];
    for (p[0] = 0; p[0] < 9; ++p[0])
    for (p[1] = 0; p[1] < 9; ++p[1])
    for (p[2] = 0; p[2] < 9; ++p[2])
    for (p[3] = 0; p[3] < 9; ++p[3])
    for (p[4] = 0; p[4] < 9; ++p[4]) {
        bool distinct = true;
        for (int a = 0; a < 5; ++a)
            for (int b = a + 1; b < 5; ++b)
                distinct = distinct && p[a] != p[b];
        if (!distinct)
            continue;
        const uint32_t h = rnd();
        for (int i = 0; i < NKEY; ++i)   // background: -1000 - 16 ((i * odd + h) % 64), distinct
            raw[i] = -1000.0f - 16.0f * (float)((i * (2 * (h & 31u) + 1) + (h >> 5)) % NKEY);
        for (int a = 0; a < 5; ++a)
            raw[pos[p[a]]] = 500.0f - 100.0f * (float)a;
        check(raw, "placement");
    }
}

int main()
{
    for (int start = 0; start < NKEY; ++start)
        placements(start);
    const long n_placed = n_cases;
    float raw[NKEY];
    // strictly ascending and descending, positive, negative and across zero
    for (int sign = -1; sign <= 1; sign += 2)
        for (int off = -1; off <= 1; ++off) {
            for (int i = 0; i < NKEY; ++i)
                raw[i] = (float)sign * (float)(i - (off + 1) * 32) * 3.5f + 0.25f;
            check(raw, "monotone");
        }
    // keys that differ in the label bits only, all of them and all but a few
    for (int v = 0; v < 4; ++v) {
        const float base = v == 0 ? 12.5f : v == 1 ? -12.5f : v == 2 ? 0.0f : -3.0e38f;
        for (int i = 0; i < NKEY; ++i)
            raw[i] = base;
        check(raw, "equal but for the labels");
        for (int rep = 0; rep < 200; ++rep) {
            for (int i = 0; i < NKEY; ++i)
                raw[i] = base;
            for (int j = 0; j < (int)(rnd() % 7u); ++j)
                raw[rnd() % NKEY] = base + (float)((int)(rnd() % 5u) - 2);
            check(raw, "nearly equal");
        }
    }
    // random draws: wide range, narrow range (many ties above the label bits), negative only
    for (int rep = 0; rep < 100000; ++rep) {
        const int mode = rep % 4;
        for (int i = 0; i < NKEY; ++i) {
            const float u = (float)(rnd() >> 8) * (1.0f / 16777216.0f) - 0.5f;
            raw[i] = mode == 0 ? u * 2.0e4f
                   : mode == 1 ? floorf(u * 12.0f)
                   : mode == 2 ? -1.0f - (u + 0.5f) * 4.0e9f
                               : ldexpf(u, (int)(rnd() % 60u) - 30);
        }
        check(raw, "random");
    }
    printf("ok: %ld cases (%ld placements of the five largest)\n", n_cases, n_placed);
    return 0;
}
