/* feat_tiles_build and feat_tile_frames (csrc/ssw_feat_tiles.inc) on the CPU.  Built with
 * -fsanitize=address,undefined (tests/test_feat_types_host.py).
 *
 *   feat_tiles_host TF LEN LEN ...   prints "T <utt> <first>" per tile, then "ok: <tiles>"
 *   feat_tiles_host                  seeded random batches: every frame of every utterance lies in
 *                                    exactly one tile, no tile spans two utterances or is longer
 *                                    than TF, empty utterances have none; bad offsets are refused;
 *                                    the LDS image of feat_tile_frames fits its budget and one more
 *                                    frame would not; prints "ok: <batches> <tiles> <sizes>" */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../soundswallower_amd/csrc/ssw_feat_tiles.inc"

static uint32_t rng_state = 0x5eed2026u;
static uint32_t
rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

#define CHECK(cond, ...)                                                                      \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);                          \
            printf(__VA_ARGS__);                                                              \
            printf("\n");                                                                     \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

int
main(int argc, char **argv)
{
    std::vector<int32_t> tiles;
    if (argc > 2) {
        const int tf = atoi(argv[1]);
        std::vector<int32_t> off(1, 0);
        for (int a = 2; a < argc; ++a)
            off.push_back(off.back() + atoi(argv[a]));
        const long n = feat_tiles_build(off.data(), (int32_t)off.size() - 1, off.back(), tf, tiles);
        CHECK(n >= 0 && (size_t)n * 2 == tiles.size(), "refused");
        for (long t = 0; t < n; ++t)
            printf("T %d %d\n", tiles[2 * t], tiles[2 * t + 1]);
        printf("ok: %ld\n", n);
        return 0;
    }
    long n_batches = 0, n_tiles = 0, n_sizes = 0;
    static const int lens[] = { 0, 1, 2, 3, 7, 63, 64, 65, 127, 128, 129, 300 };
    for (int rep = 0; rep < 400; ++rep) {
        const int n_utts = (int)(rnd() % 9), tf = 1 + (int)(rnd() % 64);
        std::vector<int32_t> off((size_t)n_utts + 1, 0);
        for (int u = 0; u < n_utts; ++u)
            off[u + 1] = off[u] + (rnd() % 4 ? lens[rnd() % 12] : tf + (int)(rnd() % 3) - 1);
        const int32_t n_frames = off[n_utts];
        const long n = feat_tiles_build(off.data(), n_utts, n_frames, tf, tiles);
        CHECK(n >= 0 && (size_t)n * 2 == tiles.size(), "batch %d refused", rep);
        std::vector<int> covered((size_t)n_frames, 0);
        int last_u = -1, last_f = -1;
        for (long t = 0; t < n; ++t) {
            const int u = tiles[2 * t], f = tiles[2 * t + 1];
            CHECK(u >= 0 && u < n_utts && f >= off[u] && f < off[u + 1], "tile %ld outside its utterance", t);
            CHECK(u > last_u || (u == last_u && f == last_f + tf), "tile %ld out of order", t);
            const int end = f + tf < off[u + 1] ? f + tf : off[u + 1];
            for (int k = f; k < end; ++k)
                ++covered[k];
            last_u = u;
            last_f = f;
        }
        for (int32_t k = 0; k < n_frames; ++k)
            CHECK(covered[k] == 1, "frame %d covered %d times", k, covered[k]);
        /* refusals: an offset that decreases, a first offset that is not 0, a last one that is not
         * n_frames, no frames per tile */
        if (n_utts >= 2) {
            std::vector<int32_t> bad(off);
            bad[1] = off[2] + 1;
            CHECK(feat_tiles_build(bad.data(), n_utts, n_frames, tf, tiles) == -1,
                  "a decreasing offset was accepted");
        }
        if (n_utts >= 1) {
            std::vector<int32_t> bad(off);
            bad[0] = 1;
            CHECK(feat_tiles_build(bad.data(), n_utts, n_frames, tf, tiles) == -1, "offset 0 != 0 accepted");
            CHECK(feat_tiles_build(off.data(), n_utts, n_frames + 1, tf, tiles) == -1, "wrong total accepted");
            CHECK(feat_tiles_build(off.data(), n_utts, n_frames, 0, tiles) == -1, "tf 0 accepted");
        }
        ++n_batches;
        n_tiles += n;
    }
    for (int C = 1; C <= 64; C += 7)
        for (int W = 0; W <= 8; ++W)
            for (int mode = 0; mode < 4; ++mode) {
                const int R = C * (2 * W + 1), J = (mode & 1) ? 1 + (int)(rnd() % 256) : 0;
                const bool gather = (mode & 2) != 0;
                for (size_t budget : { (size_t)65536, (size_t)16384, (size_t)4096, (size_t)512 }) {
                    size_t bytes = 0;
                    const int tf = feat_tile_frames(C, W, R, J, gather, budget, &bytes);
                    const size_t per = (size_t)C + (J || gather ? (size_t)R : 0) + (J && gather ? (size_t)J : 0);
                    const size_t fixed = (size_t)2 * W * C;
                    CHECK(tf >= 0 && tf <= 64, "tf %d", tf);
                    if (tf == 0) {
                        CHECK((fixed + per) * 4 > budget, "one frame fits %zu", budget);
                        continue;
                    }
                    CHECK(bytes == (fixed + (size_t)tf * per) * 4 && bytes <= budget, "image %zu of %zu", bytes, budget);
                    CHECK(tf == 64 || (fixed + (size_t)(tf + 1) * per) * 4 > budget, "tf %d is not the most", tf);
                    ++n_sizes;
                }
            }
    printf("ok: %ld %ld %ld\n", n_batches, n_tiles, n_sizes);
    return 0;
}
