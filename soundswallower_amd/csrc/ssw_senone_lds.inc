/* ssw_senone_lds.inc -- the dynamic LDS of the senone kernels, each carve once: the kernel takes
 * its pointers from it and the launcher its byte count.  Plain C++17, no HIP header:
 * ssw_kernels.hip includes it ahead of the anonymous namespace, so that device and host code see
 * the same formulas, and a host program can include it on its own
 * (tests/harness/senone_lds_host.cpp).  Offsets are bytes from the start of the dynamic LDS. */
#include <cstddef>

#if defined(__HIPCC__)
#define SSW_HD __host__ __device__
#else
#define SSW_HD
#endif

#define SSW_LOGADD_LDS 512 /* 8-bit log-add table in LDS: 256 entries + zero padding */
/* the batch kernel's copy, 1,024 bytes around LDS address CZ = 512 (ms: 2,048 around 1,024): the
 * FOLDED table of senone_fold_table below, indexed by CZ + the signed difference x - y */
#define SSW_LOGADD_MIRROR 1024
#define SSW_SENONE_NORM_W 8 /* PTM: normaliser words per frame (= SSW_MAX_FEAT) */

/* The log-add step x <- min(x, y) - tab[|x - y|] (tied_mgau_common.h:100-117) is x + G[d] with
 * d = x - y and G[d] = -tab[|d|] - max(d, 0).  In ptm_senone_kernel's chains x starts from a
 * mixture-weight byte and only falls, and y = weight + a score relative to the stream's best
 * codeword >= 0: d <= wmax, the largest weight byte.  Over d <= wmax, G lies in [-Hb, 0] with
 *   Hb = max(T, max over 0 <= d <= wmax of d + tab[d]),     T = the largest entry of tab
 * (T = tab[0] in every table logmath writes, so that the first term changes nothing), and
 * H[d] = Hb + G[d] is ONE BYTE per entry whenever Hb <= 255: the minimum is folded into the
 * look-up and the chain only ever adds.  tab = 0 beyond its 256 entries, so H = Hb there; the
 * entries above wmax, which no chain reaches, hold Hb as well. */
inline int
senone_fold_hb(const unsigned char *tab /* [256] */, int wmax)
{
    int hb = 0;
    for (int d = 0; d < 256; ++d) {
        hb = tab[d] > hb ? tab[d] : hb;
        if (d <= wmax)
            hb = d + tab[d] > hb ? d + tab[d] : hb;
    }
    return hb;
}

/* out[size]: entry cz + d = H[d], cz = size / 2; only for hb <= 255 (the callers refuse the
 * model, or leave the kernel, otherwise) */
inline void
senone_fold_table(const unsigned char *tab /* [256] */, int wmax, int hb, int size,
                  unsigned char *out)
{
    const int cz = size / 2;
    for (int e = 0; e < size; ++e) {
        const int d = e - cz, ad = d < 0 ? -d : d;
        const int h = d > wmax ? hb : hb - (ad < 256 ? (int)tab[ad] : 0) - (d > 0 ? d : 0);
        out[e] = (unsigned char)h;
    }
}

/* ptm_senone_kernel: tab[mirror] | norm[3][fpb][norm_w] int | red[16] int | item[2][n_cbf][fpb]
 * of 32 bytes | stage_sc[pad64(fpb n_cbf)] int4 | stage_cw[..] uint32 | 16 bytes that nothing
 * reads or writes.  ms: the table is twice as long and a frame has a normaliser word per codebook
 * (padded to 8) instead of one per stream.  launch_senone takes bytes() from here; the kernel
 * keeps the same carve as typed-pointer steps (see there: its instances' code must not move) and
 * tests/harness/senone_lds_host.cpp holds the two against each other. */
struct SenoneCarve {
    int fpb, n_cbf, norm_w, mirror;

    SSW_HD SenoneCarve(int fpb_, int n_cbf_, int n_cb, bool ms)
        : fpb(fpb_), n_cbf(n_cbf_), norm_w(ms ? ((n_cb + 7) & ~7) : SSW_SENONE_NORM_W),
          mirror(ms ? 2 * SSW_LOGADD_MIRROR : SSW_LOGADD_MIRROR)
    {
    }
    SSW_HD int item_pad() const { return (fpb * n_cbf + 63) & ~63; } /* whole waves of items */
    SSW_HD int tab() const { return 0; }
    SSW_HD int norm() const { return mirror; }
    SSW_HD int red() const { return norm() + 4 * (3 * norm_w * fpb); }
    SSW_HD int item() const { return red() + 4 * 16; }
    SSW_HD int stage_sc() const { return item() + 16 * (2 * 2 * n_cbf * fpb); }
    SSW_HD int stage_cw() const { return stage_sc() + 16 * item_pad(); }
    SSW_HD size_t bytes() const { return (size_t)stage_cw() + 4 * (size_t)item_pad() + 16; }
};

/* ms_senone_kernel: 256 unused bytes (the table is static LDS) | fd[n_cbf] int4 | cw4[n_cbf]
 * uint32 | red[16] int */
struct MsSenoneCarve {
    int n_cbf;

    SSW_HD explicit MsSenoneCarve(int n_cbf_) : n_cbf(n_cbf_) {}
    SSW_HD int fd() const { return 256; }
    SSW_HD int cw4() const { return fd() + 16 * n_cbf; }
    SSW_HD int red() const { return cw4() + 4 * n_cbf; }
    SSW_HD size_t bytes() const { return (size_t)red() + 16 * sizeof(int); }
};

/* What the two wave-per-frame kernels keep first in a wave's block: PTM ns4[n_cbf] | cw4[n_cbf]
 * uint32 (normalised scores and codewords of every (codebook, stream), 4 x 8 bits each); ms
 * nothing.  pad2 = an even count of 16-bit entries. */
struct WaveItems {
    int n; /* entries of ns4 and of cw4 */

    SSW_HD WaveItems(bool ms, int n_cbf) : n(ms ? 0 : n_cbf) {}
    SSW_HD int ns4() const { return 0; }
    SSW_HD int cw4() const { return 4 * n; }
    SSW_HD int end() const { return 8 * n; }
    SSW_HD static int pad2(int count) { return (count + 1) & ~1; }
};

/* senone_active2_kernel, per wave (four to a workgroup): ns4 | cw4 | a[pad2(cap)] int16, the raw
 * scores of the listed entries | row[pad2(n_sen)] int16, only with `full` */
struct Active2Carve : WaveItems {
    int cap, n_sen;
    bool full;

    SSW_HD Active2Carve(bool ms, int n_cbf, int cap_, int n_sen_, bool full_)
        : WaveItems(ms, n_cbf), cap(cap_), n_sen(n_sen_), full(full_)
    {
    }
    SSW_HD int a() const { return end(); }
    SSW_HD int row() const { return a() + 2 * pad2(cap); }
    SSW_HD size_t per_wave() const
    {
        return ((size_t)row() + (full ? 2 * (size_t)pad2(n_sen) : 0) + 15) & ~(size_t)15;
    }
    SSW_HD size_t wave(int w) const { return (size_t)w * per_wave(); }
    SSW_HD size_t bytes() const { return 4 * per_wave(); }
};

/* senone_listed_kernel, per wave: ns4 | cw4 | sen[pad2(cap)] uint16, the list | a[pad2(cap)]
 * int16, its raw scores | n, the entry counter (an int, in 16 bytes of its own) */
struct ListedCarve : WaveItems {
    int cap;

    SSW_HD ListedCarve(bool ms, int n_cbf, int cap_) : WaveItems(ms, n_cbf), cap(cap_) {}
    SSW_HD int sen() const { return end(); }
    SSW_HD int a() const { return sen() + 2 * pad2(cap); }
    SSW_HD int count() const { return a() + 2 * pad2(cap); }
    SSW_HD size_t per_wave() const { return ((size_t)count() + 16 + 15) & ~(size_t)15; }
    SSW_HD size_t wave(int w) const { return (size_t)w * per_wave(); }
    SSW_HD size_t bytes() const { return 4 * per_wave(); }
};

/* cont_listed_kernel (ssw_k11_cont.inc), per wave: x[pad4(featdim)] float, the frame's features |
 * fw[64] int, a slot per lane: the terms a group's leader combines | sen[pad2(cap)] uint16, the
 * list | a[pad2(cap)] int16, its raw scores | n, the entry counter (an int, in 16 bytes of its
 * own) */
struct ContListedCarve {
    int featdim, cap;

    SSW_HD ContListedCarve(int featdim_, int cap_) : featdim(featdim_), cap(cap_) {}
    SSW_HD static int pad2(int count) { return (count + 1) & ~1; }
    SSW_HD int x() const { return 0; }
    SSW_HD int fw() const { return 4 * ((featdim + 3) & ~3); }
    SSW_HD int sen() const { return fw() + 4 * 64; }
    SSW_HD int a() const { return sen() + 2 * pad2(cap); }
    SSW_HD int count() const { return a() + 2 * pad2(cap); }
    SSW_HD size_t per_wave() const { return ((size_t)count() + 16 + 15) & ~(size_t)15; }
    SSW_HD size_t wave(int w) const { return (size_t)w * per_wave(); }
    SSW_HD size_t bytes() const { return 4 * per_wave(); }
};

/* fpa_plan_kernel (ssw_k7_fpactive.inc), per wave: bm[nw32] uint32, the frame's senone bitmap |
 * lst[cap] uint16, the flagged senones in ascending order | cbm[2] uint32, the codebook mask's two
 * words.  cap is even (fpa_cap, ssw_fpa_shape.inc): the words behind the list stay 4-byte aligned */
struct FpaPlanCarve {
    int nw32, cap;

    SSW_HD FpaPlanCarve(int nw32_, int cap_) : nw32(nw32_), cap(cap_) {}
    SSW_HD int bitmap() const { return 0; }
    SSW_HD int list() const { return 4 * nw32; }
    SSW_HD int cbm() const { return list() + 2 * cap; }
    SSW_HD size_t per_wave() const
    {
        return (4 * (size_t)nw32 + 2 * (size_t)cap + 8 + 15) & ~(size_t)15;
    }
    SSW_HD size_t wave(int w) const { return (size_t)w * per_wave(); }
    SSW_HD size_t bytes() const { return 4 * per_wave(); }
};
