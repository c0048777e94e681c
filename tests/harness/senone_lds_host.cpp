/* SenoneCarve, MsSenoneCarve, Active2Carve, ListedCarve and FpaPlanCarve (csrc/ssw_senone_lds.inc) on the CPU,
 * against a verbatim copy of the formulas they replaced: the kernels' typed-pointer carves (run
 * here over a host buffer standing in for the dynamic LDS) and the launchers' byte counts.  Every
 * region offset and bytes() must be equal; the regions of a carve must not overlap, must end
 * inside bytes() and must be aligned as their element type needs (16 for uint4 / int4, 4 for int
 * and uint32, 2 for the 16-bit arrays).  Last line for the test to read:
 *   ok: N carves
 * Built with -fsanitize=address,undefined. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../soundswallower_amd/csrc/ssw_senone_lds.inc"

#define SSW_MAX_FEAT 8 /* ssw_internal.h */
struct int4 {
    int x, y, z, w;
};
struct uint4 {
    unsigned x, y, z, w;
};

alignas(16) static unsigned char smem[1 << 20];
static long n_carves;

struct Region {
    const char *name;
    size_t off, size, align;
};

#define FAIL(...)                                                                            \
    do {                                                                                     \
        printf("FAILED %s: ", what);                                                         \
        printf(__VA_ARGS__);                                                                 \
        printf("\n");                                                                        \
        exit(1);                                                                             \
    } while (0)

static size_t
off_of(const void *p)
{
    return (size_t)(reinterpret_cast<const unsigned char *>(p) - smem);
}

/* regions in carve order: equal to the old offsets, aligned, disjoint, inside [base, end) */
static void
check(const char *what, const Region *r, const size_t *old_off, int n, size_t base, size_t end)
{
    size_t at = base;
    for (int i = 0; i < n; ++i) {
        if (r[i].off != old_off[i])
            FAIL("%s at %zu, was at %zu", r[i].name, r[i].off, old_off[i]);
        if (r[i].off % r[i].align)
            FAIL("%s at %zu is not %zu-aligned", r[i].name, r[i].off, r[i].align);
        if (r[i].off < at)
            FAIL("%s at %zu overlaps its predecessor (ends at %zu)", r[i].name, r[i].off, at);
        at = r[i].off + r[i].size;
    }
    if (at > end)
        FAIL("the last region ends at %zu, beyond %zu", at, end);
    if (end > sizeof(smem))
        FAIL("the harness's buffer is too small (%zu)", end);
    ++n_carves;
}

/* ptm_senone_kernel<.., FPB, .., MS> and launch_senone, as they stood */
static void
senone(int FPB, int n_cb, int n_feat, bool MS)
{
    char what[96];
    snprintf(what, sizeof(what), "SenoneCarve fpb %d n_cb %d n_feat %d ms %d", FPB, n_cb, n_feat, MS);
    const int MIRROR = MS ? 2 * SSW_LOGADD_MIRROR : SSW_LOGADD_MIRROR;
    struct { int n_cb, n_feat; } P = { n_cb, n_feat };
    /* the kernel */
    const int n_cbf = P.n_cb * P.n_feat;
    uint8_t *s_tab = smem;
    const int NORM_W = MS ? ((P.n_cb + 7) & ~7) : SSW_MAX_FEAT;
    int *s_norm = reinterpret_cast<int *>(smem + MIRROR);
    int *s_red = s_norm + 3 * NORM_W * FPB;
    uint4 *s_item = reinterpret_cast<uint4 *>(s_red + 16);
    const int n_item_pad = (FPB * n_cbf + 63) & ~63;
    int4 *s_stage_sc = reinterpret_cast<int4 *>(s_item + 2 * 2 * n_cbf * FPB);
    uint32_t *s_stage_cw = reinterpret_cast<uint32_t *>(s_stage_sc + n_item_pad);
    /* the launcher */
    const bool ms_packed = MS;
    const int fpb = FPB;
    struct { int n_cb; } hh = { n_cb }, *h = &hh;
    struct { int n_cbf; } mm = { n_cbf }, *m = &mm;
    size_t lds = (ms_packed ? 2 * SSW_LOGADD_MIRROR : SSW_LOGADD_MIRROR)
        + 3 * 4 * (size_t)(ms_packed ? ((h->n_cb + 7) & ~7) : SSW_MAX_FEAT) * fpb + 16 * sizeof(int)
        + 2 * 32 * (size_t)m->n_cbf * fpb
        + 20 * (size_t)((fpb * m->n_cbf + 63) & ~63) /* DMA staging: scores + codewords */
        + 16;

    const SenoneCarve c(FPB, n_cbf, n_cb, MS);
    if (c.bytes() != lds)
        FAIL("bytes() %zu, the launcher had %zu", c.bytes(), lds);
    if (c.norm_w != NORM_W || c.item_pad() != n_item_pad)
        FAIL("norm_w %d (%d), item_pad %d (%d)", c.norm_w, NORM_W, c.item_pad(), n_item_pad);
    const Region r[] = {
        { "tab", (size_t)c.tab(), (size_t)MIRROR, 4 },
        { "norm", (size_t)c.norm(), 4 * (size_t)(3 * NORM_W * FPB), 4 },
        { "red", (size_t)c.red(), 16 * sizeof(int), 4 },
        { "item", (size_t)c.item(), 32 * (size_t)(2 * n_cbf * FPB), 16 },
        { "stage_sc", (size_t)c.stage_sc(), 16 * (size_t)n_item_pad, 16 },
        { "stage_cw", (size_t)c.stage_cw(), 4 * (size_t)n_item_pad, 4 },
    };
    const size_t old_off[] = { off_of(s_tab), off_of(s_norm), off_of(s_red), off_of(s_item),
                               off_of(s_stage_sc), off_of(s_stage_cw) };
    check(what, r, old_off, 6, 0, c.bytes());
}

/* ms_senone_kernel and launch_senone's un-packed branch, as they stood */
static void
ms_senone(int n_cb, int n_feat)
{
    char what[96];
    snprintf(what, sizeof(what), "MsSenoneCarve n_cb %d n_feat %d", n_cb, n_feat);
    const int n_cbf = n_cb * n_feat;
    int4 *s_fd = reinterpret_cast<int4 *>(smem + 256);
    uint32_t *s_cw4 = reinterpret_cast<uint32_t *>(s_fd + n_cbf);
    int *s_red = reinterpret_cast<int *>(s_cw4 + n_cbf);
    struct { int n_cbf; } mm = { n_cbf }, *m = &mm;
    size_t lds = 256 + 20 * (size_t)m->n_cbf + 16 * sizeof(int);

    const MsSenoneCarve c(n_cbf);
    if (c.bytes() != lds)
        FAIL("bytes() %zu, the launcher had %zu", c.bytes(), lds);
    const Region r[] = {
        { "fd", (size_t)c.fd(), 16 * (size_t)n_cbf, 16 },
        { "cw4", (size_t)c.cw4(), 4 * (size_t)n_cbf, 4 },
        { "red", (size_t)c.red(), 16 * sizeof(int), 4 },
    };
    const size_t old_off[] = { off_of(s_fd), off_of(s_cw4), off_of(s_red) };
    check(what, r, old_off, 3, 256, c.bytes());
}

/* senone_active2_kernel<MS> and launch_active, as they stood */
static void
active2(bool MS, int n_cb, int n_feat, int cap, int n_sen, bool full)
{
    char what[128];
    snprintf(what, sizeof(what), "Active2Carve ms %d n_cb %d n_feat %d cap %d n_sen %d full %d", MS,
             n_cb, n_feat, cap, n_sen, full);
    static int16_t a_row;
    struct { int n_cb, n_feat, cap, n_sen; int16_t *out_full; } P
        = { n_cb, n_feat, cap, n_sen, full ? &a_row : nullptr };
    const int n_cbf = P.n_cb * P.n_feat;
    struct { int n_cbf; } mm = { n_cbf }, *m = &mm;
    struct { int n_sen; } hh = { n_sen }, *h = &hh;
    struct { int cap; int16_t *out_full; } A = { cap, P.out_full };
    const bool ms = MS;
    const Active2Carve c(MS, n_cbf, cap, n_sen, full);
    {   /* the launcher */
        const size_t per_wave = (ms ? 0 : 8 * (size_t)m->n_cbf) + 2 * (size_t)((A.cap + 1) & ~1)
            + (A.out_full != NULL ? 2 * (size_t)((h->n_sen + 1) & ~1) : 0);
        const size_t lds = 4 * ((per_wave + 15) & ~(size_t)15);
        if (c.bytes() != lds)
            FAIL("bytes() %zu, the launcher had %zu", c.bytes(), lds);
    }
    for (int w = 0; w < 4; ++w) {
        /* the kernel */
        const size_t per_wave = (MS ? 0 : 8 * (size_t)n_cbf) + 2 * (size_t)((P.cap + 1) & ~1)
            + (P.out_full != nullptr ? 2 * (size_t)((P.n_sen + 1) & ~1) : 0);
        unsigned char *mine = smem + (size_t)w * ((per_wave + 15) & ~(size_t)15);
        uint32_t *s_ns4 = reinterpret_cast<uint32_t *>(mine);
        uint32_t *s_cw4 = s_ns4 + (MS ? 0 : n_cbf);
        int16_t *s_a = reinterpret_cast<int16_t *>(s_cw4 + (MS ? 0 : n_cbf));
        int16_t *s_row = s_a + ((P.cap + 1) & ~1);

        const size_t b = c.wave(w);
        if (b % 16)
            FAIL("wave %d's block at %zu is not 16-aligned", w, b);
        const Region r[] = {
            { "ns4", b + (size_t)c.ns4(), MS ? 0 : 4 * (size_t)n_cbf, 4 },
            { "cw4", b + (size_t)c.cw4(), MS ? 0 : 4 * (size_t)n_cbf, 4 },
            { "a", b + (size_t)c.a(), 2 * (size_t)cap, 2 },
            { "row", b + (size_t)c.row(), full ? 2 * (size_t)n_sen : 0, 2 },
        };
        const size_t old_off[] = { off_of(s_ns4), off_of(s_cw4), off_of(s_a), off_of(s_row) };
        check(what, r, old_off, 4, b, w < 3 ? c.wave(w + 1) : c.bytes());
    }
}

/* senone_listed_kernel<MS> and launch_active, as they stood */
static void
listed(bool MS, int n_cb, int n_feat, int cap)
{
    char what[96];
    snprintf(what, sizeof(what), "ListedCarve ms %d n_cb %d n_feat %d cap %d", MS, n_cb, n_feat, cap);
    struct { int n_cb, n_feat, cap; } P = { n_cb, n_feat, cap }, L = P;
    const int n_cbf = P.n_cb * P.n_feat;
    struct { int n_cbf; } mm = { n_cbf }, *m = &mm;
    const bool ms = MS;
    const ListedCarve c(MS, n_cbf, cap);
    {   /* the launcher */
        const size_t per_wave = ((ms ? 0 : 8 * (size_t)m->n_cbf) + 4 * (size_t)((L.cap + 1) & ~1)
                                 + 16 + 15) & ~(size_t)15;
        const size_t lds = 4 * per_wave;
        if (c.bytes() != lds)
            FAIL("bytes() %zu, the launcher had %zu", c.bytes(), lds);
    }
    for (int w = 0; w < 4; ++w) {
        /* the kernel */
        const size_t per_wave = ((MS ? 0 : 8 * (size_t)n_cbf) + 4 * (size_t)((P.cap + 1) & ~1) + 16 + 15)
            & ~(size_t)15;
        unsigned char *mine = smem + (size_t)w * per_wave;
        uint32_t *s_ns4 = reinterpret_cast<uint32_t *>(mine);
        uint32_t *s_cw4 = s_ns4 + (MS ? 0 : n_cbf);
        uint16_t *s_sen = reinterpret_cast<uint16_t *>(s_cw4 + (MS ? 0 : n_cbf));
        int16_t *s_a = reinterpret_cast<int16_t *>(s_sen + ((P.cap + 1) & ~1));
        int *s_n = reinterpret_cast<int *>(s_a + ((P.cap + 1) & ~1));

        const size_t b = c.wave(w);
        if (b % 16)
            FAIL("wave %d's block at %zu is not 16-aligned", w, b);
        const Region r[] = {
            { "ns4", b + (size_t)c.ns4(), MS ? 0 : 4 * (size_t)n_cbf, 4 },
            { "cw4", b + (size_t)c.cw4(), MS ? 0 : 4 * (size_t)n_cbf, 4 },
            { "sen", b + (size_t)c.sen(), 2 * (size_t)cap, 2 },
            { "a", b + (size_t)c.a(), 2 * (size_t)cap, 2 },
            { "n", b + (size_t)c.count(), sizeof(int), 4 },
        };
        const size_t old_off[] = { off_of(s_ns4), off_of(s_cw4), off_of(s_sen), off_of(s_a), off_of(s_n) };
        check(what, r, old_off, 5, b, w < 3 ? c.wave(w + 1) : c.bytes());
    }
}

/* fpa_plan_kernel's pointer steps, kept there as typed-pointer steps, and the byte count the
 * three places that sized its launch had (kernel, LDS limit check, launch) */
static void
fpa_plan(int nw32, int cap)
{
    char what[96];
    snprintf(what, sizeof(what), "FpaPlanCarve nw32 %d cap %d", nw32, cap);
    struct { int nw32; } P = { nw32 };
    const FpaPlanCarve c(nw32, cap);
    {   /* the host, twice */
        const size_t plan_lds = 4 * ((4 * (size_t)nw32 + 2 * (size_t)cap + 8 + 15) & ~(size_t)15);
        if (c.bytes() != plan_lds)
            FAIL("bytes() %zu, the host had %zu", c.bytes(), plan_lds);
    }
    for (int w = 0; w < 4; ++w) {
        unsigned char *fpa_smem = smem;
        /* the kernel */
        const size_t per_wave = (4 * (size_t)P.nw32 + 2 * (size_t)cap + 8 + 15) & ~(size_t)15;
        uint32_t *bm = reinterpret_cast<uint32_t *>(fpa_smem + (size_t)w * per_wave);
        uint16_t *lst = reinterpret_cast<uint16_t *>(bm + P.nw32);
        uint32_t *cbm = reinterpret_cast<uint32_t *>(lst + cap); /* two words */

        if (c.per_wave() != per_wave)
            FAIL("per_wave() %zu, the kernel had %zu", c.per_wave(), per_wave);
        const size_t b = c.wave(w);
        if (b % 16)
            FAIL("wave %d's block at %zu is not 16-aligned", w, b);
        /* (an odd cap leaves the mask's words 2-aligned: fpa_cap hands out even ones only, and
         * the carve says so by the alignment this asks of it) */
        const Region r[] = {
            { "bitmap", b + (size_t)c.bitmap(), 4 * (size_t)nw32, 4 },
            { "list", b + (size_t)c.list(), 2 * (size_t)cap, 2 },
            { "cbm", b + (size_t)c.cbm(), 8, cap % 2 ? (size_t)2 : (size_t)4 },
        };
        const size_t old_off[] = { off_of(bm), off_of(lst), off_of(cbm) };
        check(what, r, old_off, 3, b, w < 3 ? c.wave(w + 1) : c.bytes());
    }
}

int
main()
{
    for (int nw32 : { 1, 2, 63, 64, 65, 66, 161, 2048 })
        for (int cap : { 2, 3, 64, 65, 66, 448, 449, 450, 5126, 65534 })
            fpa_plan(nw32, cap);
    const int fpbs[] = { 1, 2 }, n_cbs[] = { 1, 7, 8, 9, 36, 42, 64 }, n_feats[] = { 1, 3, 4 };
    const int caps[] = { 1, 2, 63, 64, 65, 449, 5126 }, n_sens[] = { 1, 2107, 2108, 5126 };
    for (int n_cb : n_cbs)
        for (int n_feat : n_feats) {
            ms_senone(n_cb, n_feat);
            for (int ms = 0; ms < 2; ++ms) {
                for (int fpb : fpbs)
                    senone(fpb, n_cb, n_feat, ms != 0);
                for (int cap : caps) {
                    listed(ms != 0, n_cb, n_feat, cap);
                    for (int n_sen : n_sens)
                        for (int full = 0; full < 2; ++full)
                            active2(ms != 0, n_cb, n_feat, cap, n_sen, full != 0);
                }
            }
        }
    printf("ok: %ld carves\n", n_carves);
    return 0;
}
