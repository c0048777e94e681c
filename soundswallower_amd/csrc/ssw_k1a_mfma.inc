/* ssw_k1a_mfma.inc -- K1a on the matrix cores: the speculative top-N scan of ssw_k1a_frames.inc
 * with the 26 fp32 multiply-adds per (frame, density) replaced by binary16 MFMAs.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/*
 * The scan only needs a key that provably bounds the reference's density value from above
 * (ssw_k1a_frames.inc); the four best candidates are re-evaluated exactly afterwards, in the
 * reference's operation order, and a pair whose order cannot be proven is redone exactly
 * in-wave.  The key is the quadratic form  key[i][t] = sum_k W[i][k] X[k][t]  with
 * W[i] = (a_0..a_12, 0, 0, c | b_0..b_12, 0, 0, 0) and X[t] = (x_0..x_12, *, *, 2^ec | x_0^2..
 * x_12^2, 0, 0, 0): a 128 x 32 by 32 x N matrix product per (codebook, stream).  fp32 FMAs on
 * the vector unit made the scan VALU-bound (26 of the 39 instructions per density; the loop ran
 * at 100 % issue rate, DESIGN.md section 5).  Round 4: W (scaled by a power of two per codebook
 * x stream, on the host) and X are cut into TWO binary16 parts each (22 significand bits; the
 * split of W is done on the host and its residual charged element by element) and the three
 * part products that matter -- (1,1) (1,2) (2,1) -- are accumulated by six
 * v_mfma_f32_32x32x16_f16 per tile, which run at 16 x the fp32 rate on a pipe of their own,
 * beside the vector unit that keeps the running top-5 lists.  (Rounds 2-3: three bf16 parts, six
 * part products, twelve MFMAs per tile for the same error constant: 303 -> 247 ns of SIMD time
 * per tile, tools/microbench/mfma_f16_scan.hip.)  The error of that evaluation is bounded in
 * ssw_model.c (ssw_host_build_mfma_records) and folded into c, so the key stays an upper bound;
 * nothing downstream changes.  binary16's exponent range is what the price is paid in: a frame
 * with a feature beyond +-255 (its square would overflow) is not trusted and takes the exact
 * pass; small values are safe (subnormals are honoured by v_cvt and by the matrix pipe: same
 * microbenchmark), and the spare K slots 13 and 14 of X hold 32768 so that an inert row (a
 * density left to the exact form) can be made -4e9 with binary16 entries.
 *
 * Work split: a wave owns one (codebook, stream) and 128 frames = 4 column blocks of 32.  In the
 * 32 x 32 output tile of one MFMA lane l holds column (frame) l % 32 and 16 of the 32 rows
 * (densities): lanes l and l + 32 share a frame.  Each lane keeps the top 5 of its 16 rows per
 * row block (found from sorted triples of keys: ssw_top5_select.inc), for two column blocks at
 * a time; then the halves swap one list each, so that the
 * lower half finishes the first block's frames and the upper half the second's (merge, exact
 * re-evaluation of the four candidates, sort, proof: once per frame).
 */
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

#define SSW_MFMA_WIDEN 1.8537045e-05f /* (3 K + 17 + 6) 2^-24 with K = 96 (ssw_model.c) */
#define SSW_MFMA_XMAX 255.0f          /* |x_j| beyond this: x_j^2 does not fit binary16 */

/* this scan's form of key for scan_upper_bound (ssw_scan_common.inc): scaled by a power of two
 * per codebook x stream, widened by the part of the error bound that grows with the key */
struct ScanKeysMfma {
    static constexpr float widen = SSW_MFMA_WIDEN;
    float scale;
    __device__ __forceinline__ float unscaled(float ub) const { return ub * scale; }
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct SplitX {
    f16x8 p[2];
};

/* Two binary16 parts of eight floats: p0 + p1 = v up to max(2^-22 |v|, 2^-25).  Two values per
 * conversion (round to nearest even, subnormals kept), which already leaves them packed the way
 * the MFMA operand wants them; the residual v - part is exact in fp32. */
__device__ __forceinline__ SplitX
split2_f16(const float (&v)[8])
{
    SplitX s;
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        r[j] = v[j];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        u32x4 w;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const float2v pr = { r[j], r[j + 1] };
            const f16x2 h = __builtin_convertvector(pr, f16x2);
            w[j >> 1] = __builtin_bit_cast(uint32_t, h);
            if (p == 0) {
                /* r - (float)h, exact either way, as ONE instruction: the mixed-precision fma
                 * takes the binary16 half as it stands (tools/microbench/fma_mix_probe.hip:
                 * equal to v_cvt_f32_f16 + v_sub_f32 on every binary16 value, subnormals
                 * included, both halves) */
                asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]"
                    : "=v"(r[j]) : "v"(w[j >> 1]), "v"(r[j]));
                asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                    : "=v"(r[j + 1]) : "v"(w[j >> 1]), "v"(r[j + 1]));
            }
        }
        s.p[p] = __builtin_bit_cast(f16x8, w);
    }
    return s;
}

/* This lane's share of the X operand for its frame: half 0 of the wave holds k = 0..7 of both
 * 16-wide K blocks, half 1 k = 8..15.  K block 0 = (x_0 .. x_12, 32768, 32768, 2^ec), K block 1 =
 * (x_0^2 .. x_12^2, 0, 0, 0), the squares rounded to fp32 first; each cut into two binary16
 * parts.  A lane fetches the dimensions of ITS half only -- two 16-byte loads: 0..3 and 4..7, or
 * 8..11 and 9..12 (the latter for its last element: nothing is read beyond the row) -- so that
 * squares and parts are made of 8 values, not of 13 with a select per slot. */
struct XRaw {
    float4u a, b;
};

template <int VECLEN>
__device__ __forceinline__ XRaw
mfma_load_x(const float *__restrict__ xp, bool hi)
{
    static_assert(VECLEN == 13, "K layout: 13 dimensions, the constant at slot 15");
    XRaw r;
    r.a = *reinterpret_cast<const float4u *>(xp + (hi ? 8 : 0));
    r.b = *reinterpret_cast<const float4u *>(xp + (hi ? 9 : 4));
    return r;
}

__device__ __forceinline__ void
mfma_build_x(const XRaw &r, bool hi, float xconst, SplitX (&bx)[2])
{
    const float4u a = r.a, b = r.b;
    float v0[8], v1[8];
    v0[0] = a.x, v0[1] = a.y, v0[2] = a.z, v0[3] = a.w;
    v0[4] = hi ? b.w : b.x;
    v0[5] = hi ? 32768.0f : b.y;
    v0[6] = hi ? 32768.0f : b.z;
    v0[7] = hi ? xconst : b.w;
#pragma unroll
    for (int j = 0; j < 5; ++j)
        v1[j] = v0[j] * v0[j];
    v1[5] = hi ? 0.0f : b.y * b.y;
    v1[6] = hi ? 0.0f : b.z * b.z;
    v1[7] = hi ? 0.0f : b.w * b.w;
    bx[0] = split2_f16(v0);
    bx[1] = split2_f16(v1);
}

template <int VECLEN>
__device__ __forceinline__ void
mfma_build_x(const float *__restrict__ xp, bool hi, float xconst, SplitX (&bx)[2])
{
    mfma_build_x(mfma_load_x<VECLEN>(xp, hi), hi, xconst, bx);
}

/* Keys of one 32-density x 32-frame tile: the three part products that matter, smallest first --
 * (1,2) (2,1) of both K blocks, then (1,1), parts numbered from 1 -- six MFMAs into one fp32
 * accumulator (this order is what the bound of ssw_model.c charges: only the last two MFMAs add
 * terms of the size of M).  A fragments from the workgroup's LDS copy. */
__device__ __forceinline__ v16f
mfma_key_tile_frag(const f16x8 (&a)[2][2], const SplitX (&bx)[2])
{
    v16f acc = {};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kb][0], bx[kb].p[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kb][1], bx[kb].p[0], acc, 0, 0, 0);
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kb][0], bx[kb].p[0], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ v16f
mfma_key_tile(const uint4 *s_w, int rb, int lane, const SplitX (&bx)[2])
{
    f16x8 a[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int p = 0; p < 2; ++p)
            a[kb][p] = __builtin_bit_cast(f16x8, s_w[((rb * 2 + kb) * 2 + p) * 64 + lane]);
    return mfma_key_tile_frag(a, bx);
}

/* Parity / bound check view (ssw_debug_scan_keys): the raw keys of one (codebook, stream) for
 * every frame, exactly as the scan computes them (same operand build, same MFMA order), one
 * wave per 128 frames, scaled back by 2^s.  out [n_frames][128], relative to the codebook's d0. */
template <int VECLEN>
__global__ void __launch_bounds__(64)
ptm_mfma_keys_kernel(const uint4 *__restrict__ wfrag, const float *__restrict__ recmax,
                     const float *__restrict__ feats, int n_frames, int featdim, int foff, int cbf,
                     float *__restrict__ out)
{
    const int lane = threadIdx.x & 63, col = lane & 31;
    const bool hi = lane >= 32;
    __shared__ uint4 s_w[16 * 64];
    for (int i = lane; i < 16 * 64; i += 64)
        s_w[i] = wfrag[(size_t)cbf * (16 * 64) + i];
    const float scale = recmax[(size_t)cbf * SSW_REC_FLOATS + 1];
    const float xconst = recmax[(size_t)cbf * SSW_REC_FLOATS + 3];
    __syncthreads();
    for (int cb = 0; cb < 4; ++cb) {
        const int t = (int)blockIdx.x * 128 + 32 * cb + col;
        const int tl = t < n_frames ? t : n_frames - 1;
        const float *xp = feats + (size_t)tl * featdim + foff;
        SplitX bx[2];
        mfma_build_x<VECLEN>(xp, hi, xconst, bx);
        for (int rb = 0; rb < 4; ++rb) {
            const v16f acc = mfma_key_tile(s_w, rb, lane, bx);
            if (t < n_frames)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    out[(size_t)t * 128 + 32 * rb + 8 * (r >> 2) + (hi ? 4 : 0) + (r & 3)]
                        = acc[r] * scale;
        }
    }
}

/* (the list operations: ssw_top5_select.inc) */
#define SSW_TOP5_INSERT(L, key) ssw_top5_insert(L, key);

/* The 16 keys of a lane's share of one tile, labelled: label = register + 16 x row block (0..63):
 * wave-uniform, an SGPR operand; bit 6 = the lane's half, added when the halves swap lists.  (No
 * inline asm on the accumulator: the compiler pads the MFMA -> VALU read hazard only for
 * instructions it can see.) */
__device__ __forceinline__ void
mfma_label_keys(const v16f &acc, int rb, uint32_t keymask, float (&key)[16])
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        uint32_t lab;
        asm("s_add_i32 %0, %1, %2" : "=s"(lab) : "s"(16 * rb), "i"(r) : "scc");
        key[r] = __uint_as_float((__float_as_uint(acc[r]) & keymask) | lab);
    }
}

/* The halves swap: each hands over the list of the column block it does not finish (the lower
 * half finishes A, the upper half B) and merges what it receives -- the other half's rows of ITS
 * block -- into its own.  In registers: v_permlane32_swap_b32 exchanges the upper half of its
 * first operand with the lower half of its second, which leaves {A.lo | B.lo} in the first and
 * {A.hi | B.hi} in the second: for every lane the two lists of its own frame, the first from
 * the lower half's rows and the second from the upper half's, so the half bit (64) goes into
 * the second alone and no lane has to choose.  The second is sorted: it is merged by position
 * (ssw_top5_merge).  LA and LB are used up. */
__device__ __forceinline__ void
mfma_swap_merge(float (&LA)[5], float (&LB)[5], float (&L)[5])
{
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(LA[k]),
                                                         __float_as_uint(LB[k]), false, false);
        L[k] = __uint_as_float(sw[0]);
        LB[k] = __uint_as_float(sw[1] | 64u);
    }
    ssw_top5_merge(L, LB);
}

/* density index of a label: 32 rb + 8 (r / 4) + 4 half + r % 4 */
__host__ __device__ __forceinline__ constexpr uint32_t
mfma_label_density(uint32_t lab)
{
    return ((lab >> 4) & 3u) * 32u + ((lab >> 2) & 3u) * 8u + (lab >> 6) * 4u + (lab & 3u);
}

/* ... and the label of a density: bits 0-1 = r % 4, 2 = half, 3-4 = r / 4, 5-6 = rb of the index
 * go to bits 0-1, 6, 2-3, 4-5 of the label */
__host__ __device__ __forceinline__ constexpr uint32_t
mfma_density_label(int cw)
{
    return (uint32_t)((cw & 3) | ((cw >> 3) & 3) << 2 | (cw >> 5) << 4 | ((cw >> 2) & 1) << 6);
}

/* the two are inverses, on all 128 densities */
constexpr bool
mfma_labels_invert()
{
    for (int cw = 0; cw < 128; ++cw)
        if (mfma_label_density(mfma_density_label(cw)) != (uint32_t)cw
            || mfma_density_label((int)mfma_label_density((uint32_t)cw)) != (uint32_t)cw)
            return false;
    return true;
}
static_assert(mfma_labels_invert(), "mfma_density_label is the inverse of mfma_label_density");

/* NSTEP = 64-frame steps per wave: 2 (a wave owns 128 frames) or 1 (64 frames, twice the
 * workgroups: the chip's 1,024 workgroup slots are then refilled as groups finish instead of
 * draining in one round). */
#ifndef SSW_MFMA_WAVES
#define SSW_MFMA_WAVES 5 /* waves per SIMD the register budget is cut for (512 / 5 -> 96 VGPRs) */
#endif
/* AUDIT (SSW_SCAN_AUDIT=k, round 5): every k-th wave hands ALL of its frames to the exact in-wave
 * pass, proven or not, and compares what the exact pass finds for a proven pair with what the
 * scan wrote for it -- the scan's claim checked in the product's own process, on the data it is
 * given.  Instances of their own: the default kernel's registers and schedule are untouched. */
template <int VECLEN, bool MS, int NSTEP, bool AUDIT = false, bool MASKED = false>
__global__ void __launch_bounds__(256, SSW_MFMA_WAVES)
ptm_topn_mfma_kernel(const float *__restrict__ rec, const uint4 *__restrict__ wfrag,
                     const float *__restrict__ recmax, const uint32_t *__restrict__ exlist,
                     const float *__restrict__ feats, FramesParams P)
{
    static_assert(VECLEN == 13, "K layout: 13 dimensions, the constant at slot 15");
    const int lane = threadIdx.x & 63;
    const int col = lane & 31;
    const bool hi = lane >= 32; /* second half: rows 4..7 (+8 k) of a tile, K slice 8..15 */
    /* placement as in the FMA scan: the (codebook, stream) x tile-group pairs are cut into 8
     * contiguous chunks, one per XCD (workgroups b and b + 8 share an XCD) -- here by cost
     * (FramesParams::xcd_lo) */
    const int pair = P.xcd_lo[blockIdx.x & 7u] + (int)(blockIdx.x >> 3);
    if (pair >= P.xcd_lo[(blockIdx.x & 7u) + 1])
        return;
    const int cbf = pair / P.tile_groups;
    const int tile = (pair - cbf * P.tile_groups) * 4
        + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t_base = P.frame_lo + tile * (64 * NSTEP);
    const int f = cbf % P.n_feat;
    const int foff = P.featoff[f];

    /* LDS: the codebook's exact records (epilogue and exact pass), packed to 28 floats a row
     * (14 KB), and its binary16 A fragments, 16 of 1 KB: [row block][K block][part][lane] x 16 B.
     * 30 KB in all: FIVE workgroups per CU.  (A CU hands out 160 KB, but five workgroups of
     * 32 KB do not fit and five of 31 KB do: tools/microbench/lds_occupancy.hip.)  Rows of seven
     * 16-byte chunks need no swizzle: neighbouring rows start 7 chunks apart, so eight lanes
     * reading the same chunk of eight consecutive rows hit the eight bank groups. */
    __shared__ float4 s_rec[128 * (SSW_REC28_FLOATS / 4)];
    __shared__ uint4 s_w[16 * 64];
    /* the utterance-start bits of the wave's frames, 64 per step (t_base is a multiple of 64:
     * two aligned words), requested here with the rest of the prologue's loads and made uniform
     * after the barrier.  The exact in-wave pass used to fetch the bit of every pair it redid
     * with a load of its own, and s_waitcnt vmcnt(0) also waits for the stores the epilogue has
     * just issued: microseconds.  (Plain loads, not an s_load in inline asm with its wait in a
     * second statement: the compiler is free to copy or spill such an output before the wait
     * -- the two-step instance did, and took garbage for the bits of its second step.) */
    uint2 ustart_v[NSTEP];
#pragma unroll
    for (int q = 0; q < NSTEP; ++q) {
        const int tq = t_base + 64 * q < P.n_frames ? t_base + 64 * q : 0;
        ustart_v[q] = *reinterpret_cast<const uint2 *>(P.utt_start + (tq >> 5));
    }
    /* the keys are relative to d0 and scaled: key' = (key - d0) 2^-s (one power of two per
     * codebook x stream, ssw_model.c); xconst = 2^ec is the constant's slot of X */
    const float4 cbc = *reinterpret_cast<const float4 *>(recmax + (size_t)cbf * SSW_REC_FLOATS);
    const float d0 = cbc.x, scale = cbc.y, inv_scale = cbc.z, xconst = cbc.w;
    /* the exact-form list of the codebook (count, then up to 128 entries: two per lane),
     * fetched here once: read inside the epilogue's loop, every entry was a dependent trip to
     * memory (700 clocks per density: the waves of codebook x stream 0 of en-us, 28 such
     * densities, lived 32 K clocks, twice the others) */
    static_assert(SSW_EXLIST_STRIDE >= 129, "two entries per lane behind the count");
    const uint32_t *xl = exlist + (size_t)cbf * SSW_EXLIST_STRIDE;
    const uint32_t n_ex_v = xl[0], my_ex0 = xl[1 + lane], my_ex1 = xl[65 + lane];
    int n_ex;
    /* One step per wave: the X operand is fetched with the LDS fill's loads and built between
     * the fill's stores and the barrier -- it needs nothing from LDS, and at the start of a launch
     * every wave of the chip stands in this prologue with nobody to hide its latencies behind
     * (+1.7-2.2 % frames/s at 4,096 frames).  (With two steps the operands would have to live
     * across the loop's back edge: 23 spilt registers; unrolled instead, the launch at 16,384
     * frames lost 2 %.) */
    constexpr bool pre_x = NSTEP == 1;
    SplitX bxa[2], bxb[2];
    auto x_row = [&](int t) {
        return feats + (size_t)(t < P.n_frames ? t : P.n_frames - 1) * P.featdim + foff;
    };
    {
        /* (rec = the packed copy of the exact records, [cbf][128][28]: 896 16-byte pieces) */
        const float4 *src = reinterpret_cast<const float4 *>(rec + (size_t)cbf * 128 * SSW_REC28_FLOATS);
        const uint4 *wsrc = wfrag + (size_t)cbf * (16 * 64);
        uint4 wst[4];
        float4 stage[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            stage[i] = src[i * 256 + (int)threadIdx.x < 896 ? i * 256 + (int)threadIdx.x : 895];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            wst[i] = wsrc[i * 256 + (int)threadIdx.x];
        XRaw ra, rb;
        if (pre_x) {
            ra = mfma_load_x<VECLEN>(x_row(t_base + col), hi);
            rb = mfma_load_x<VECLEN>(x_row(t_base + 32 + col), hi);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = i * 256 + (int)threadIdx.x;
            if (e < 896)
                s_rec[e] = stage[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            s_w[i * 256 + (int)threadIdx.x] = wst[i];
        if (pre_x) {
            mfma_build_x(ra, hi, xconst, bxa);
            mfma_build_x(rb, hi, xconst, bxb);
        }
        n_ex = __builtin_amdgcn_readfirstlane((int)n_ex_v);
    }
    unsigned long long ustart[NSTEP];
#pragma unroll
    for (int q = 0; q < NSTEP; ++q)
        ustart[q] = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)ustart_v[q].y) << 32)
            | (uint32_t)__builtin_amdgcn_readfirstlane((int)ustart_v[q].x);
    __syncthreads();
    if (t_base >= P.n_frames)
        return;
    SSW_TL(0)
#ifdef SSW_TIMELINE
    if (lane == 0) {
        int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (wv < 8192) {
            g_timeline[wv * 6 + 4] = __builtin_amdgcn_s_getreg(63492); /* HW_ID */
            g_timeline[wv * 6 + 5] = __builtin_amdgcn_s_getreg(20 | (31 << 11)); /* XCC_ID */
        }
    }
#endif

    uint32_t keymask;
    asm volatile("v_mov_b32 %0, 0xffffff80" : "=v"(keymask));
    const float NEG_INF = -__builtin_huge_valf();
    const float *srec_f = reinterpret_cast<const float *>(s_rec);

    /* Two column blocks (64 frames) at a time.  Lanes l and l + 32 share the rows of a tile, so
     * both of them work on column block A = frames t0 .. t0 + 31 and then on B = t0 + 32 ..
     * t0 + 63 (same A fragments); afterwards the lower half of the wave FINISHES block A and the
     * upper half block B -- lane l ends up owning frame t0 + l -- so that merge, exact
     * re-evaluation, sort and proof run once per frame, not once per lane of the pair.
     * What the exact in-wave pass needs afterwards, per lane and 64-frame step: the codeword
     * order and the 4th candidate's score (floor of topn_exact_step). */
    uint32_t cpk[2] = { 0u, 0u };
    int s3[2] = { 0, 0 };
    unsigned long long need[2] = { 0ull, 0ull };
    unsigned long long audited[2] = { 0ull, 0ull }; /* AUDIT: proven pairs redone all the same */
    const bool audit_wave = AUDIT && P.audit_k > 0
        && (pair * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) % P.audit_k == 0;

#pragma unroll 1
    for (int step = 0; step < NSTEP; ++step) {
        const int t0 = t_base + 64 * step;
        if (!pre_x) {
            mfma_build_x<VECLEN>(x_row(t0 + col), hi, xconst, bxa);
            mfma_build_x<VECLEN>(x_row(t0 + 32 + col), hi, xconst, bxb);
        }
        /* selection state per column block: the list of 5; the two best middles and the best
         * smallest of the key triples (M, Z) and of the triples of their largest (N, Y)
         * (ssw_top5_select.inc) */
        float LA[5], LB[5], NA[2], NB[2], YA, YB, MA[2], MB[2], ZA, ZB;
        ssw_top5_reset2(LA, NA, YA, MA, ZA, NEG_INF);
        ssw_top5_reset2(LB, NB, YB, MB, ZB, NEG_INF);
        /* (a rolled loop: unrolled, the compiler runs the MFMAs of all row blocks ahead into
         * dozens of accumulator registers, which costs the 4th wave per SIMD; the overlap of
         * the matrix pipe with the inserts comes from the other waves) */
#pragma unroll 1
        for (int rb = 0; rb < 4; ++rb) {
            f16x8 a[2][2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    a[kb][p] = __builtin_bit_cast(f16x8, s_w[((rb * 2 + kb) * 2 + p) * 64 + lane]);
            {
                const v16f acc = mfma_key_tile_frag(a, bxa);
                float key[16];
                mfma_label_keys(acc, rb, keymask, key);
                ssw_top5_tile2(LA, NA, YA, MA, ZA, key);
            }
            {
                const v16f acc = mfma_key_tile_frag(a, bxb);
                float key[16];
                mfma_label_keys(acc, rb, keymask, key);
                ssw_top5_tile2(LB, NB, YB, MB, ZB, key);
            }
        }
        /* back to plain lists of 5, then the halves swap */
        ssw_top5_fold2(LA, NA, YA, MA, ZA);
        ssw_top5_fold2(LB, NB, YB, MB, ZB);
        float L[5];
        mfma_swap_merge(LA, LB, L);
        /* from here on lane l works on frame t0 + l alone */
        const int t = t0 + lane;
        const int tl = t < P.n_frames ? t : P.n_frames - 1;
        const float *xp = feats + (size_t)tl * P.featdim + foff;
        float x[VECLEN];
#pragma unroll
        for (int j = 0; j + 4 <= VECLEN; j += 4) {
            const float4u v = *reinterpret_cast<const float4u *>(xp + j);
            x[j] = v.x, x[j + 1] = v.y, x[j + 2] = v.z, x[j + 3] = v.w;
        }
#pragma unroll
        for (int j = VECLEN & ~3; j < VECLEN; ++j)
            x[j] = xp[j];
        /* One density of the codebook exactly, for this lane's frame (sub, mul, mul, sub per
         * dimension, each rounded once: src/ptm_mgau.c:63-68).  Round 3: written on pairs of
         * dimensions -- the differences, squares and products of dimensions 2p, 2p + 1 are one
         * packed instruction each (v_pk_add_f32 / v_pk_mul_f32 round every lane on its own: no
         * contraction, same bits), the 13 subtractions from the running value stay sequential,
         * in j order -- 34 vector instructions per density where the compiler's own pairing
         * spent ~70 on shuffles; and the record's eight 16-byte chunks sit at (row base ^ chunk
         * << 4 ^ (row & 7) << 4), one v_xor each. */
        float2v x2[6];
#pragma unroll
        for (int p = 0; p < 6; ++p)
            x2[p] = float2v{ x[2 * p], x[2 * p + 1] };
        auto exact_row = [&](uint32_t row) -> float {
            const unsigned char *rowp = reinterpret_cast<const unsigned char *>(s_rec)
                + row * (SSW_REC28_FLOATS * 4);
            float4v rv[SSW_REC28_FLOATS / 4];
#pragma unroll
            for (int q = 0; q < SSW_REC28_FLOATS / 4; ++q)
                rv[q] = *reinterpret_cast<const float4v *>(rowp + q * 16);
            /* keep the 16-byte LDS reads whole, and in flight together (one statement) */
            asm volatile("" : "+v"(rv[0]), "+v"(rv[1]), "+v"(rv[2]), "+v"(rv[3]), "+v"(rv[4]),
                              "+v"(rv[5]), "+v"(rv[6]));
            /* floats of the packed row: mean j = e[j], det = e[13], scale j = e[14 + j] */
            float dd = rv[3].y;
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const float2v mean = (p & 1) ? float2v{ rv[p >> 1].z, rv[p >> 1].w }
                                             : float2v{ rv[p >> 1].x, rv[p >> 1].y };
                /* scale pair at e[14 + 2p]: chunk (14 + 2p) / 4, second half for even p */
                const int vq = (14 + 2 * p) >> 2;
                const float2v var = (p & 1) ? float2v{ rv[vq].x, rv[vq].y }
                                            : float2v{ rv[vq].z, rv[vq].w };
                const float2v diff = x2[p] - mean;
                const float2v sq = diff * diff;
                const float2v cc = sq * var;
                dd = dd - cc.x;
                dd = dd - cc.y;
            }
            {
                const float diff = x[12] - rv[3].x;
                const float sq = diff * diff;
                const float cc = sq * rv[6].z;
                dd = dd - cc;
            }
            return dd;
        };
        /* densities left to the exact form (inert MFMA rows), evaluated the reference's way */
        for (int i = 0; i < n_ex; ++i) {
            const int cwx = i < 64 ? __builtin_amdgcn_readlane((int)my_ex0, i)
                                   : __builtin_amdgcn_readlane((int)my_ex1, i - 64);
            float dd = exact_row((uint32_t)cwx);
            dd = (dd - d0) * inv_scale; /* into the scan's scaled domain (a power of two: exact) */
            const uint32_t lab = mfma_density_label(cwx);
            const float key = __uint_as_float((__float_as_uint(dd) & keymask) | lab);
            SSW_TOP5_INSERT(L, key)
        }
        /* the four candidates exactly */
        int c[4], sk[4];
        float dv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t lab = __float_as_uint(L[k]) & 127u;
            c[k] = (int)mfma_label_density(lab);
            dv[k] = exact_row((uint32_t)c[k]);
            sk[k] = MS ? ms_fden(dv[k]) : dens2int(dv[k]);
        }
        /* sorted best first, then the proof: four distinct values above the bound the 5th key
         * puts on every other density (ssw_scan_common.inc) */
        sort4_best_first<MS>(sk, c, dv);
        const ScanBound ub = scan_upper_bound(L[4], ScanKeysMfma{ scale }, d0);
        bool proven = scan_proven<MS>(sk, dv, ub);
        /* a feature whose square does not fit binary16 made every key of this frame -inf or
         * NaN: nothing the scan says about it can be trusted (a NaN feature hides from v_max,
         * but then the four exact values are NaN and the tests above have already failed) */
        float am5;
        {
            float am0, am1, am2, am3, am4;
            asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(am0) : "v"(x[0]), "v"(x[1]), "v"(x[2]));
            asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(am1) : "v"(x[3]), "v"(x[4]), "v"(x[5]));
            asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(am2) : "v"(x[6]), "v"(x[7]), "v"(x[8]));
            asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(am3) : "v"(x[9]), "v"(x[10]), "v"(x[11]));
            asm("v_max3_f32 %0, %1, %2, |%3|" : "=v"(am4) : "v"(am0), "v"(am1), "v"(x[12]));
            asm("v_max3_f32 %0, %1, %2, %3" : "=v"(am5) : "v"(am2), "v"(am3), "v"(am4));
            proven = proven && am5 <= SSW_MFMA_XMAX;
        }
        /* the floor the exact step may scan from (topn_exact_step): the lowest of the four
         * candidates' scores, a valid floor when they are four DIFFERENT codewords.  Keys at
         * different positions of the tiles name different codewords, except that a density left
         * to the exact form has two keys, its true one and its inert row's (-4.3e9): with the
         * 4th key above that, finite, and the frame's features within the scan's range, the four
         * are different.  (A frame the scan could not rank -- every key -inf / NaN -- can name
         * one codeword four times.)  Ties among the four no longer cost the floor: tying frames
         * are most of what is redone. */
        const int floor_s = (L[3] > -4.0e9f && am5 <= SSW_MFMA_XMAX) ? sk[3] : INT_MIN;
        const uint32_t cpk_s = order_pack(c);
        unsigned long long need_s = __ballot(!proven && t < P.n_frames);
        if (AUDIT && audit_wave) {
            const unsigned long long proven_s = __ballot(proven && t < P.n_frames);
            need_s |= proven_s;
#pragma unroll
            for (int q = 0; q < 2; ++q)
                audited[q] = q == step ? proven_s : audited[q];
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) { /* step is wave-uniform: scalar selects */
            cpk[q] = q == step ? cpk_s : cpk[q];
            s3[q] = q == step ? floor_s : s3[q];
            need[q] = q == step ? need_s : need[q];
        }
        if (t < P.n_frames) { /* final unless the exact pass below rewrites it */
            const size_t idx = (size_t)t * P.n_cbf + cbf;
            P.topn_cw[idx] = cpk_s;
            P.topn_sc[idx] = make_int4(sk[0], sk[1], sk[2], sk[3]);
        }
        if (step == 0) {
            SSW_TL(1)
        }
    }
    SSW_TL(2)

    /* Exact in-wave pass: unproven pairs redone by the whole wave in frame order; the frame
     * before is the neighbouring lane, lane 63 of the step before, or -- for the tile's first
     * frame, or behind a frame that did not scan this codebook -- re-derived.  What it must do is
     * stated once, in ssw_scan_common.inc ("the exact in-wave pass"); its text stays here and in
     * ptm_topn_frames_kernel because any function around it, or around its choice of the carried
     * order alone, changes this kernel's default instances.  Here: the utterance-start bits are
     * the words prefetched above, the floor is the one kept per step (s3), and a redone pair is
     * stored at once (the scan has already stored what it found). */
    if (P.seg_of_frame != nullptr) {
#pragma unroll
        for (int q = 0; q < NSTEP; ++q) {
            need[q] &= scan_mask_unscanned(P, cbf, t_base + 64 * q + lane);
            audited[q] &= need[q];
        }
    }
    if ((need[0] | (NSTEP > 1 ? need[1] : 0ull)) != 0ull) {
        const float *srow0 = srec_f + lane * SSW_REC28_FLOATS;
        const float *srow1 = srow0 + 64 * SSW_REC28_FLOATS;
        const int sw = 0; /* (the packed rows are not swizzled) */
        unsigned n_done = 0;
        SSW_TL2(0)
#pragma unroll
        for (int h = 0; h < NSTEP; ++h) {
            unsigned long long todo = need[h];
            while (todo != 0ull) {
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int t = t_base + 64 * h + l;
                float dvx[2];
                int ivx[2];
                wave_frame_densities<VECLEN, true, !MS>(feats, P.featdim, foff, t, srow0, srow1,
                                                        sw, dvx, ivx);
                if (n_done == 0) {
                    SSW_TL2(1)
                }
                int Lc[4], Ls[4];
                if (MS) {
                    float Ld[4];
                    ms_exact_step(dvx, Lc, Ld);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        Ls[k] = ms_fden(Ld[k]);
                } else if (!topn_self_determined(ivx, lane, Lc, Ls)) {
                    /* (round 4: most redone pairs are there because the 5th key's bound reached
                     * the 4th candidate, not because ints tie: with all 128 exact values on the
                     * table the test of the claim itself -- four distinct ints above every other
                     * -- settles those in ~100 vector instructions, history or not; only real
                     * ties go through the reference's state machine, ~500 scalar instructions
                     * at one per 4-5 clocks) */
                    if ((ustart[h] >> l) & 1ull) {
                        start_order(P, cbf, t, Lc);
                    } else if ((h == 0 && l == 0) || !cb_scanned_u(P, cbf / P.n_feat, t - 1)
                               || chain_skipped(P, t - 1)) {
                        carried_order_of<VECLEN, true, MASKED>(P, cbf, feats, foff, t - 1, lane, srow0,
                                                       srow1, sw, Lc);
                    } else {
                        const uint32_t pk = l == 0
                            ? (uint32_t)__builtin_amdgcn_readlane((int)cpk[0], 63)
                            : (uint32_t)__builtin_amdgcn_readlane((int)cpk[h], l - 1);
                        order_unpack(pk, Lc);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        Ls[k] = INT_MIN;
                    topn_exact_step<2, 4>(dvx, ivx, Lc, Ls, true,
                                          __builtin_amdgcn_readlane(s3[h], l));
                }
                if (n_done == 0) {
                    SSW_TL2(2)
                }
                const bool was_proven = AUDIT && ((audited[h] >> l) & 1ull) != 0ull;
                if (AUDIT && was_proven) {
                    /* what the scan wrote for this pair (by this very lane; its stores have
                     * been acknowledged: vmcnt counts them), read past the vector cache */
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (lane == l) {
                        const size_t idx = (size_t)t * P.n_cbf + cbf;
                        const uint32_t newpk = order_pack(Lc);
                        const int *old = reinterpret_cast<const int *>(P.topn_sc + idx);
                        bool same = __hip_atomic_load(P.topn_cw + idx, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT) == newpk;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            same = same && __hip_atomic_load(old + k, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT) == Ls[k];
                        if (!same)
                            atomicAdd(P.n_fixed + 3, 1ull);
                    }
                }
                if (lane == l) {
                    cpk[h] = order_pack(Lc);
                    const size_t idx = (size_t)t * P.n_cbf + cbf;
                    P.topn_cw[idx] = cpk[h];
                    P.topn_sc[idx] = make_int4(Ls[0], Ls[1], Ls[2], Ls[3]);
                }
                if (!was_proven)
                    ++n_done;
            }
        }
        SSW_TL2(3)
#ifdef SSW_TIMELINE
        if (lane == 0) {
            int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
            if (wv < 8192)
                g_timeline2[wv * 8 + 4] = n_done;
        }
#endif
        if (lane == 0)
            atomicAdd(P.n_fixed, (unsigned long long)n_done);
        if (AUDIT && lane == 0 && (audited[0] | audited[1]) != 0ull)
            atomicAdd(P.n_fixed + 2, (unsigned long long)(__builtin_popcountll(audited[0])
                                                          + __builtin_popcountll(audited[1])));
    }
    SSW_TL(3)
}
#undef SSW_TOP5_INSERT

/* Selection view (ssw_debug_scan_top5): the scan's selection alone, on keys the caller supplies
 * -- keys [n_frames][128] by density.  One wave per 64 frames; each lane takes the keys the MFMA
 * tiles would hand it (lane l, register r of row block rb: density 32 rb + 8 (r >> 2) + 4 half +
 * (r & 3) of frame l % 32 of the column block, as ptm_mfma_keys_kernel writes them), labels
 * them and runs what the scan runs: the tiles' selection network, the fold, the swap of the
 * halves and the merge.  Out, per frame: the densities of the five best keys and those keys
 * with the label bits cleared. */
__global__ void __launch_bounds__(64)
ptm_scan_top5_debug_kernel(const float *__restrict__ keys, int n_frames, int32_t *__restrict__ out_idx,
                           float *__restrict__ out_key)
{
    const int lane = threadIdx.x & 63, col = lane & 31;
    const bool hi = lane >= 32;
    const int t0 = (int)blockIdx.x * 64;
    uint32_t keymask;
    asm volatile("v_mov_b32 %0, 0xffffff80" : "=v"(keymask));
    const float NEG_INF = -__builtin_huge_valf();
    float LA[5], LB[5], NA[2], NB[2], YA, YB, MA[2], MB[2], ZA, ZB;
    ssw_top5_reset2(LA, NA, YA, MA, ZA, NEG_INF);
    ssw_top5_reset2(LB, NB, YB, MB, ZB, NEG_INF);
    auto tile_of = [&](int blk, int rb) {
        const int t = t0 + 32 * blk + col;
        const float *kp = keys + (size_t)(t < n_frames ? t : n_frames - 1) * 128 + 32 * rb
            + (hi ? 4 : 0);
        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc[r] = kp[8 * (r >> 2) + (r & 3)];
        return acc;
    };
#pragma unroll 1
    for (int rb = 0; rb < 4; ++rb) {
        float key[16];
        mfma_label_keys(tile_of(0, rb), rb, keymask, key);
        ssw_top5_tile2(LA, NA, YA, MA, ZA, key);
        mfma_label_keys(tile_of(1, rb), rb, keymask, key);
        ssw_top5_tile2(LB, NB, YB, MB, ZB, key);
    }
    ssw_top5_fold2(LA, NA, YA, MA, ZA);
    ssw_top5_fold2(LB, NB, YB, MB, ZB);
    float L[5];
    mfma_swap_merge(LA, LB, L);
    const int t = t0 + lane;
    if (t < n_frames)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint32_t bits = __float_as_uint(L[k]);
            out_idx[(size_t)t * 5 + k] = (int32_t)mfma_label_density(bits & 127u);
            out_key[(size_t)t * 5 + k] = __uint_as_float(bits & ~127u);
        }
}

/* Parity aid (ssw_debug_mfma_eps): one v_mfma_f32_32x32x16_f16 per 32 x 32 tile, D = A B + C with
 * A [32][16], B [16][32] binary16 and C [32][32] fp32 as the host laid them out -- so that the
 * accumulation error the bound of ssw_model.c ASSUMES (eps <= 34 u of the sum of the |terms|) is
 * measured on the device the tests run on, not only by a microbenchmark.  One wave per tile. */
__global__ void __launch_bounds__(64)
mfma_f16_tile_kernel(const _Float16 *__restrict__ A, const _Float16 *__restrict__ B,
                     const float *__restrict__ C, float *__restrict__ D)
{
    const int l = threadIdx.x;
    const size_t tile = blockIdx.x;
    A += tile * 32 * 16, B += tile * 16 * 32, C += tile * 32 * 32, D += tile * 32 * 32;
    f16x8 a, b;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = A[(l % 32) * 16 + 8 * (l / 32) + i];
        b[i] = B[(8 * (l / 32) + i) * 32 + (l % 32)];
    }
    v16f c;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        c[r] = C[(8 * (r / 4) + 4 * (l / 32) + r % 4) * 32 + (l % 32)];
    const v16f d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        D[(8 * (r / 4) + 4 * (l / 32) + r % 4) * 32 + (l % 32)] = d[r];
}

/* ---------------------------------------------------------------------------------- */
/* Load-time self-test of the one hardware assumption the scan's bound makes           */
/* ---------------------------------------------------------------------------------- */
/* ssw_model.c charges every v_mfma_f32_32x32x16_f16 with an accumulation error of at most
 * eps = 34 u (u = 2^-24) of the sum of the |terms| it adds (16 products + C).  The adder is not
 * documented, so ssw_model_load MEASURES it on the device the model is loaded on, before the
 * matrix-core scan is allowed to run there (ssw_host_model.inc: mfma_self_test): one wave per
 * tile, operands made in registers from the tile number (no upload), D = A B + C by the
 * instruction itself, the reference sum in fp64 on the vector unit (products of binary16
 * values are exact in fp64, the 17-term sum is good to 2^-52 of the terms: 2^-28 u), worst
 * |D - exact| / sum |terms| per tile written out in u, D[0][0] beside it.
 *   tiles 0..23    the adversarial alignment set of tests/test_gpu_mfma_bound.py (one big term
 *                  and fifteen small ones just below / above 2^-j ulp of it, j = 0..5; the big
 *                  term as a product or as C) -- every entry of such a tile is the same sum,
 *                  which the HOST also knows in closed form and checks D[0][0] against
 *   tiles 24..     five random families in rotation: plain, C cancelling the dot product to
 *                  1e-3, operands spread over 2^+-10, products of equal size and alternating
 *                  sign (cancelling against C), one product 2^12 times the others
 * Row i of A is one random row a[k] scaled by 2^((i % 3) - 1) (exact), so a lane can form the
 * reference of its 16 outputs from what it generates itself; C differs per element. */
__device__ __forceinline__ uint32_t
selftest_hash(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
/* a binary16 value (1 + m / 1024) 2^e, sign s, exactly representable; e in [-14, 15] */
__device__ __forceinline__ float
selftest_f16val(uint32_t h, int e_lo, int e_span)
{
    const int e = e_lo + (int)((h >> 11) % (uint32_t)e_span);
    const float v = (1.0f + (float)(h & 1023u) * (1.0f / 1024.0f)) * __builtin_exp2f((float)e);
    return (h >> 31) ? -v : v;
}

#define SSW_SELFTEST_ADVERSARIAL 24
#define SSW_SELFTEST_TILES (SSW_SELFTEST_ADVERSARIAL + 320)
/* (results in a device symbol: a hipMalloc / hipFree pair costs more than the whole test) */
__device__ float2 g_selftest_out[SSW_SELFTEST_TILES];
__global__ void __launch_bounds__(64)
mfma_selftest_kernel(uint32_t seed)
{
    float2 *out = g_selftest_out;
    const int l = threadIdx.x, col = l & 31, half = l >> 5;
    const uint32_t tile = blockIdx.x;
    float a[16], b[16];   /* a[k] = A[0][k] (row 0), b[k] = B[k][col] */
    float cbig = 0.0f;
    int fam = -1;
    if (tile < SSW_SELFTEST_ADVERSARIAL) {
        const int j = tile >> 2;
        const bool above = (tile >> 1) & 1u, in_c = tile & 1u;
        const float frac = above ? 1.0f + 0.0009765625f : 1.0f - 0.00048828125f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            a[k] = 0.03125f * frac;                    /* 2^-5 frac */
            b[k] = __builtin_exp2f((float)(-6 - j));  /* product = 2^(-11 - j) frac */
        }
        if (in_c)
            cbig = 4096.0f;
        else
            a[0] = 64.0f, b[0] = 64.0f;
    } else {
        fam = (int)((tile - SSW_SELFTEST_ADVERSARIAL) % 5u);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t ha = selftest_hash(seed ^ (tile * 977u + (uint32_t)k * 131u + 1u));
            const uint32_t hb = selftest_hash(seed ^ (tile * 1409u + (uint32_t)k * 61u + (uint32_t)col * 7919u + 2u));
            if (fam == 2) {
                a[k] = selftest_f16val(ha, -10, 21);
                b[k] = selftest_f16val(hb, -10, 21);
            } else if (fam == 3) { /* +t, -t, +t ...: equal size, alternating sign */
                a[k] = __builtin_fabsf(selftest_f16val(selftest_hash(seed ^ (tile * 977u)), -1, 2)) * ((k & 1) ? -1.0f : 1.0f);
                b[k] = __builtin_fabsf(selftest_f16val(selftest_hash(seed ^ (tile * 1409u + (uint32_t)col * 7919u)), -1, 2));
            } else {
                a[k] = selftest_f16val(ha, -2, 3);
                b[k] = selftest_f16val(hb, -2, 3);
            }
        }
        if (fam == 4)
            a[0] *= 4096.0f; /* <= 2^13: still binary16 */
    }
    /* reference dot product of row 0 and the sum of its |terms|, fp64 */
    double dot = 0.0, terms = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const double pr = (double)a[k] * (double)b[k];
        dot += pr;
        terms += __builtin_fabs(pr);
    }
    f16x8 af, bf;
    v16f c;
    /* this lane's A fragment is row (l % 32) = row `col` of A, K slice 8 half .. + 7; rows are
     * row 0 scaled by 2^((row % 3) - 1).  (For the adversarial tiles every row is row 0.) */
    const float rs_own = fam < 0 ? 1.0f : __builtin_exp2f((float)((col % 3) - 1));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        af[i] = (_Float16)(a[8 * half + i] * rs_own);
        bf[i] = (_Float16)b[8 * half + i];
    }
    double cd[16], rs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 8 * (r / 4) + 4 * half + r % 4;
        rs[r] = fam < 0 ? 1.0 : (double)__builtin_exp2f((float)((row % 3) - 1));
        const uint32_t hc = selftest_hash(seed ^ (tile * 2741u + (uint32_t)row * 389u + (uint32_t)col * 17u + 3u));
        const float u01 = (float)(hc & 0xffffu) * (1.0f / 65536.0f);
        float cv;
        if (fam < 0)
            cv = cbig;
        else if (fam == 1 || fam == 3)
            cv = (float)(-(dot * rs[r]) * (1.0 + 1.0e-3 * (double)u01));
        else
            cv = (u01 - 0.5f) * (fam == 0 ? 1.0f : 8.0f);
        c[r] = cv;
        cd[r] = (double)cv;
    }
    const v16f d = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, c, 0, 0, 0);
    float worst = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const double exact = dot * rs[r] + cd[r];
        const double tsum = terms * rs[r] + __builtin_fabs(cd[r]);
        const double err = __builtin_fabs((double)d[r] - exact);
        const float ratio = (float)(err / tsum * 16777216.0);
        worst = ratio > worst ? ratio : worst;       /* (a NaN result: caught on the host by D00) */
        if (!(d[r] == d[r]))
            worst = __builtin_huge_valf();
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(worst, off, WAVE);
        worst = o > worst ? o : worst;
    }
    if (l == 0)
        out[tile] = make_float2(worst, d[0]);
}
