/* WsLayout (csrc/ssw_ws_layout.inc) on the CPU: offsets against a restatement of the rule the
 * hand-written piece tables used, and fill() against an image built piece by piece.  The typed
 * overloads (a piece registered with the pointer that is to address it): the same offsets as the
 * plain calls give, and resolve() sets every pointer to base + offset.  Built with
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
    long n_layouts = 0, n_pieces = 0, n_fills = 0, n_slots = 0;
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
            /* the same pieces registered with typed pointers (three types in turn, as a kernel's
             * parameter block mixes them): the offsets of the plain calls, and resolve() */
            {
                const int *pi[40];
                uint16_t *ps[40];
                const long long *pl[40];
                WsLayout B;
                for (int i = 0; i < n; ++i) {
                    size_t at;
                    if (i % 3 == 0)
                        at = is_in[i] ? B.in(&pi[i], src[i].data(), bytes[i]) : B.out(&pi[i], bytes[i]);
                    else if (i % 3 == 1)
                        at = is_in[i] ? B.in(&ps[i], src[i].data(), bytes[i]) : B.out(&ps[i], bytes[i]);
                    else
                        at = is_in[i] ? B.in(&pl[i], src[i].data(), bytes[i]) : B.out(&pl[i], bytes[i]);
                    CHECK(at == got[i], "piece %d of %d with a pointer: offset %zu, plain %zu", i, n, at, got[i]);
                }
                CHECK(B.size() == L.size() && B.in_bytes() == L.in_bytes() && B.ins.size() == L.ins.size(),
                      "with pointers: total %zu (%zu), in_bytes %zu (%zu)", B.size(), L.size(),
                      B.in_bytes(), L.in_bytes());
                std::vector<unsigned char> ws(B.size() + 1);
                B.resolve(ws.data());
                for (int i = 0; i < n; ++i) {
                    const void *p = i % 3 == 0 ? (const void *)pi[i] : i % 3 == 1 ? (const void *)ps[i] : (const void *)pl[i];
                    CHECK(p == (const void *)(ws.data() + got[i]), "piece %d of %d: resolve() missed base + %zu", i, n, got[i]);
                    ++n_slots;
                }
            }
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
    /* a zero-byte optional table (the grammar search's fsg_of_utt: NULL = grammar 0) keeps its
     * slot: it takes no space, and its pointer is resolved like any other -- to where the next
     * piece lies; `room` and plain pieces mix with bound ones */
    {
        WsLayout L;
        unsigned char four[4] = { 1, 2, 3, 4 }, base[1024 + 1];
        const int *utt_off = NULL, *fsg_of_utt = NULL;
        const long long *hist_off = NULL;
        int *n_seg = NULL;
        CHECK(L.in(&utt_off, four, 4) == 0, "first");
        CHECK(L.in(&fsg_of_utt, NULL, 0) == 256 && L.mark() == 256, "an empty table with a pointer takes no space");
        CHECK(L.in(&hist_off, four, 4, 4 + 16) == 256, "the next piece lies where the empty one does");
        CHECK(L.in(four, 4) == 512, "a plain piece among bound ones");
        CHECK(L.out(&n_seg, 4) == 768 && L.size() == 1024, "device-only space with a pointer");
        CHECK(L.slots.size() == 4, "%zu slots, 4 registered", L.slots.size());
        L.resolve(base);
        CHECK((const void *)utt_off == base && (const void *)fsg_of_utt == base + 256
                  && (const void *)hist_off == base + 256 && (void *)n_seg == base + 768,
              "resolve() with an empty table");
        n_slots += 4;
    }
    printf("slots: %ld pointers resolved\n", n_slots);
    printf("ok: %ld layouts, %ld pieces, %ld fills\n", n_layouts, n_pieces, n_fills);
    return 0;
}
