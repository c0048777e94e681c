// Host check of the scan's TWO-LEVEL selection network (ssw_top5_tile2 / ssw_top5_fold2), of the
// inserts that start where a key can land (ssw_top5_insert_from) and of the merge by position
// (ssw_top5_merge) in soundswallower_amd/csrc/ssw_top5_select.inc: the same text, compiled for
// the CPU with the three-input operations written in plain C (valid for non-NaN floats), against
// a full sort and against the one-level network (ssw_top5_tile / ssw_top5_fold), bit for bit.
// A lane of the scan sees 64 keys per column block -- four tiles of 16 -- whose low 7 bits are
// labels, so all keys are distinct; a frame's 128 keys are two such lanes' (bit 6 = the half).
// tests/test_top5_select2_host.py builds this with -fsanitize=address,undefined and runs it as a
// process of its own.
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
static const float NEG_INF = -std::numeric_limits<float>::infinity();
static long n_cases = 0, n_merges = 0;

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static bool above(float a, float b) { return a > b; }

static void fail(const char *what, const char *which, int k, float got, float want,
                 const float *key, int n)
{
    fprintf(stderr, "FAIL (%s, case %ld): rank %d is %.9g (label %u), %s gives %.9g (label %u)\n",
            what, n_cases, k, got, bits_of(got) & 127u, which, want, bits_of(want) & 127u);
    for (int i = 0; i < n; ++i)
        fprintf(stderr, "%s%.9g", i ? " " : "  keys: ", key[i]);
    fprintf(stderr, "\n");
    exit(1);
}

// the list of one lane: label the keys (position = register + 16 x row block, + half_bit), run
// the two-level network tile by tile and fold; compare with the five largest of a full sort and
// with the one-level network's list
static void lane_list(const float *raw, uint32_t half_bit, float (&H)[5], const char *what)
{
    float key[NKEY], sorted[NKEY];
    for (int i = 0; i < NKEY; ++i)
        sorted[i] = key[i] = float_of((bits_of(raw[i]) & 0xffffff80u) | (uint32_t)i | half_bit);
    float N[2], Y, M[2], Z, H1[5], M1[2], Z1;
    ssw_top5_reset2(H, N, Y, M, Z, NEG_INF);
    ssw_top5_reset(H1, M1, Z1, NEG_INF);
    for (int t = 0; t < NKEY / 16; ++t) {
        float tile[16];
        for (int r = 0; r < 16; ++r)
            tile[r] = key[16 * t + r];
        ssw_top5_tile2(H, N, Y, M, Z, tile);
        ssw_top5_tile(H1, M1, Z1, tile);
    }
    ssw_top5_fold2(H, N, Y, M, Z);
    ssw_top5_fold(H1, M1, Z1);
    std::partial_sort(sorted, sorted + 5, sorted + NKEY, above);
    ++n_cases;
    for (int k = 0; k < 5; ++k) {
        if (bits_of(H[k]) != bits_of(sorted[k]))
            fail(what, "a full sort", k, H[k], sorted[k], key, NKEY);
        if (bits_of(H[k]) != bits_of(H1[k]))
            fail(what, "the one-level network", k, H[k], H1[k], key, NKEY);
    }
}

static void check(const float (&raw)[NKEY], const char *what)
{
    float H[5];
    lane_list(raw, 0u, H, what);
}

// one frame: the lists of its two lanes (rows of the lower and of the upper half), merged by
// position, either into the other, against the sort of the 128 labelled keys
static void check_frame(const float (&raw)[2 * NKEY], const char *what)
{
    float LO[5], HI[5], sorted[2 * NKEY];
    lane_list(raw, 0u, LO, what);
    lane_list(raw + NKEY, 64u, HI, what);
    for (int i = 0; i < 2 * NKEY; ++i)
        sorted[i] = float_of((bits_of(raw[i]) & 0xffffff80u) | (uint32_t)i);
    std::partial_sort(sorted, sorted + 5, sorted + 2 * NKEY, above);
    float A[5], B[5];
    for (int k = 0; k < 5; ++k)
        A[k] = LO[k], B[k] = HI[k];
    ssw_top5_merge(A, HI);
    ssw_top5_merge(B, LO);
    ++n_merges;
    for (int k = 0; k < 5; ++k) {
        if (bits_of(A[k]) != bits_of(sorted[k]))
            fail(what, "a full sort of the frame (upper into lower)", k, A[k], sorted[k], sorted, 5);
        if (bits_of(B[k]) != bits_of(sorted[k]))
            fail(what, "a full sort of the frame (lower into upper)", k, B[k], sorted[k], sorted, 5);
    }
}

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

// background: -1000 - 16 ((i * odd + h) % 64), distinct, below the placed keys, another order
// from case to case
static void background(float (&raw)[NKEY])
{
    const uint32_t h = rnd();
    for (int i = 0; i < NKEY; ++i)
        raw[i] = -1000.0f - 16.0f * (float)((i * (2 * (h & 31u) + 1) + (h >> 5)) % NKEY);
}

// The five largest keys placed, in every order, on every 5 of the 9 consecutive positions from
// `start` on (wrapping at 64): one triple and both its neighbours, or across triples, the
// leftover 16th slot and the tile boundaries.
static void placements(int start)
{
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
        background(raw);
        for (int a = 0; a < 5; ++a)
            raw[(start + p[a]) % NKEY] = 500.0f - 100.0f * (float)a;
        check(raw, "placement");
    }
}

// The five largest on every 5 of the 16 positions of one tile (4,368 sets), each set in
// ORDERS_PER_SET random orders: the second-level triples span the whole tile, so the five fall
// 3 + 2, 2 + 2 + 1, ... across them and across the first level's triples, the leftover 16th key
// included.  The tiles before and behind hold background keys.
static const int ORDERS_PER_SET = 24;
static long tile_placements(int tile)
{
    float raw[NKEY];
    long n = 0;
    for (uint32_t set = 0; set < 65536u; ++set) {
        if (__builtin_popcount(set) != 5)
            continue;
        int pos[5], m = 0;
        for (int i = 0; i < 16; ++i)
            if ((set >> i) & 1u)
                pos[m++] = i;
        for (int rep = 0; rep < ORDERS_PER_SET; ++rep) {
            for (int i = 4; i > 0; --i)
                std::swap(pos[i], pos[rnd() % (uint32_t)(i + 1)]);
            background(raw);
            for (int a = 0; a < 5; ++a)
                raw[16 * tile + pos[a]] = 500.0f - 100.0f * (float)a;
            check(raw, "placement within a tile");
            ++n;
        }
    }
    return n;
}

static float draw(int mode)
{
    const float u = (float)(rnd() >> 8) * (1.0f / 16777216.0f) - 0.5f;
    return mode == 0 ? u * 2.0e4f                       // wide
         : mode == 1 ? floorf(u * 12.0f)                // narrow: many ties above the label bits
         : mode == 2 ? -1.0f - (u + 0.5f) * 4.0e9f      // negative only
                     : ldexpf(u, (int)(rnd() % 60u) - 30);
}

int main()
{
    for (int start = 0; start < NKEY; ++start)
        placements(start);
    const long n_placed = n_cases;
    long n_tile = 0;
    for (int tile = 0; tile < NKEY / 16; ++tile)
        n_tile += tile_placements(tile);
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
    // random draws: wide range, narrow range, negative only, and over 60 binades
    for (int rep = 0; rep < 100000; ++rep) {
        for (int i = 0; i < NKEY; ++i)
            raw[i] = draw(rep % 4);
        check(raw, "random");
    }
    // the merge by position: whole frames of 128 keys.  Random draws; the five largest split
    // k / 5 - k between the halves at random positions; all keys equal but for their labels
    float frame[2 * NKEY];
    for (int rep = 0; rep < 40000; ++rep) {
        for (int i = 0; i < 2 * NKEY; ++i)
            frame[i] = draw(rep % 4);
        check_frame(frame, "merge, random");
    }
    for (int rep = 0; rep < 6000; ++rep) {
        float lo[NKEY], hi[NKEY];
        background(lo);
        background(hi);
        for (int i = 0; i < NKEY; ++i)
            frame[i] = lo[i], frame[NKEY + i] = hi[i] - 0.5f;
        const int k_lo = rep % 6;   // 0..5 of the five largest in the lower half's rows
        int order[5] = { 0, 1, 2, 3, 4 };
        for (int i = 4; i > 0; --i)
            std::swap(order[i], order[rnd() % (uint32_t)(i + 1)]);
        for (int a = 0; a < 5; ++a) {
            int at;
            do
                at = (a < k_lo ? 0 : NKEY) + (int)(rnd() % NKEY);
            while (frame[at] > 0.0f);
            frame[at] = 500.0f - 100.0f * (float)order[a];
        }
        check_frame(frame, "merge, split placement");
    }
    for (int v = 0; v < 3; ++v) {
        for (int i = 0; i < 2 * NKEY; ++i)
            frame[i] = v == 0 ? 37.25f : v == 1 ? -37.25f : 0.0f;
        check_frame(frame, "merge, equal but for the labels");
    }
    printf("ok: %ld cases (%ld placements of the five largest within nine positions, %ld within "
           "one tile), %ld merges\n", n_cases, n_placed, n_tile, n_merges);
    return 0;
}
