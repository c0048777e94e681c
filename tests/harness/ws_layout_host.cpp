/* WsLayout (csrc/ssw_ws_layout.inc) on the CPU: offsets against a restatement of the rule the
 * hand-written piece tables used, and fill() against an image built piece by piece.  Built with
 * -fsanitize=address,undefined (tests/test_ws_layout_host.py); every stage buffer has exactly the
 * size fill() may write, so an overrun is an ASan report. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../soundswallower_amd/csrc/ssw_ws_layout.inc"

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
main()
{
    static const size_t sizes[] = { 0, 1, 255, 256, 257, 4096 };
    const unsigned char SENTINEL = 0xA5;
    long n_layouts = 0, n_pieces = 0, n_fills = 0;
    for (int n = 1; n <= 40; ++n)
        for (int rep = 0; rep < 5; ++rep) {
            std::vector<size_t> bytes((size_t)n), want((size_t)n), got((size_t)n);
            std::vector<int> is_in((size_t)n);
            std::vector<std::vector<unsigned char>> src((size_t)n);
            /* the rule as the piece tables had it: a piece starts where the last one ended, and
             * the end is rounded up to the next multiple of 256 */
            size_t off = 0, want_in_end = 0;
            for (int i = 0; i < n; ++i) {
                bytes[i] = sizes[rnd() % 6];
                is_in[i] = rep == 0 ? 1 : (int)(rnd() & 1); /* rep 0: uploaded tables only */
                src[i].resize(bytes[i]);
                for (size_t k = 0; k < bytes[i]; ++k)
                    src[i][k] = (unsigned char)(rnd() & 0x7f); /* never the sentinel */
                want[i] = off;
                off = (off + bytes[i] + 255) & ~(size_t)255;
                if (is_in[i])
                    want_in_end = off;
            }
            const size_t want_total = off;
            WsLayout L;
            for (int i = 0; i < n; ++i) {
                CHECK(L.mark() == want[i], "piece %d of %d: mark %zu, rule %zu", i, n, L.mark(), want[i]);
                got[i] = is_in[i] ? L.in(src[i].data(), bytes[i]) : L.out(bytes[i]);
            }
            printf("L");
            for (int i = 0; i < n; ++i)
                printf(" %zu:%zu", bytes[i], got[i]);
            printf(" = %zu\n", L.size());
            for (int i = 0; i < n; ++i) {
                CHECK(got[i] == want[i], "piece %d of %d: offset %zu, rule %zu", i, n, got[i], want[i]);
                CHECK(got[i] % 256 == 0, "piece %d: offset %zu not a multiple of 256", i, got[i]);
                if (i + 1 < n)
                    CHECK(got[i] + bytes[i] <= got[i + 1], "pieces %d and %d overlap", i, i + 1);
                ++n_pieces;
            }
            CHECK(got[n - 1] + bytes[n - 1] <= L.size(), "the last piece ends beyond the total");
            CHECK(L.size() == want_total, "total %zu, rule %zu", L.size(), want_total);
            CHECK(L.in_bytes() == want_in_end, "in_bytes %zu, rule %zu", L.in_bytes(), want_in_end);
            ++n_layouts;
            /* fill from every piece boundary (and from the end of the uploaded part) */
            std::vector<size_t> froms(got);
            froms.push_back(L.in_bytes());
            for (size_t from : froms) {
                if (from > L.in_bytes())
                    continue; /* behind the uploaded part: nothing a caller would stage */
                const size_t len = L.in_bytes() - from;
                unsigned char *stage = (unsigned char *)malloc(len); /* exactly: ASan sees one byte more */
                CHECK(stage != NULL || len == 0, "malloc(%zu)", len);
                if (len)
                    memset(stage, SENTINEL, len);
                L.fill(stage, from);
                std::vector<unsigned char> image(len, SENTINEL);
                for (int i = 0; i < n; ++i)
                    if (is_in[i] && got[i] >= from)
                        for (size_t k = 0; k < bytes[i]; ++k)
                            image[got[i] - from + k] = src[i][k];
                for (size_t k = 0; k < len; ++k)
                    CHECK(stage[k] == image[k], "fill from %zu: byte %zu is %u, expected %u", from, k,
                          stage[k], image[k]);
                free(stage);
                ++n_fills;
            }
        }
    /* `room`: a piece that takes more space than it uploads (the + 16 tails, the max(x, 1) floors) */
    {
        WsLayout L;
        unsigned char two[2] = { 1, 2 };
        CHECK(L.in(two, 2, 2 + 16) == 0 && L.mark() == 256, "room");
        CHECK(L.in(two, 0, 1) == 256 && L.mark() == 512, "room of an empty table");
        CHECK(L.in(two, 256, 256 + 16) == 512 && L.mark() == 1024, "room across a boundary");
        CHECK(L.in(NULL, 0) == 1024 && L.mark() == 1024, "an empty table takes no space");
        CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512,
              "align256");
    }
    printf("ok: %ld layouts, %ld pieces, %ld fills\n", n_layouts, n_pieces, n_fills);
    return 0;
}
