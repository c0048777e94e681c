/* ssw_k1b_senone.inc -- K1b / K3: normalise the top-N block, combine with the mixture weights (PTM, one-frame, ms).
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* K1b: normalise the top-N block and combine it with the mixture weights              */
/* ---------------------------------------------------------------------------------- */

struct SenoneParams {
    const uint32_t *topn_cw; /* [n_frames][n_cbf] 4 codewords packed */
    const int4 *topn_sc;     /* [n_frames][n_cbf] raw scores */
    const uint8_t *mixw;     /* [n_feat][n_density][slot_stride], slot order */
    const uint8_t *quad_cb;  /* [n_quads] codebook of slots 4q..4q+3 */
    const short4 *slot_sen;  /* [n_quads] senone ids of the 4 slots, -1 = padding */
    /* [n_quads] first senone id s0 | 4 consecutive ids << 16 | n << 17 | codebook << 24: the
     * quad's first n slots hold s0 .. s0 + n - 1 and the others are padding (every quad of the
     * prefix layout, ssw_slot_layout.inc); n = 0: it has no such form, its slots' ids are read
     * from slot_sen */
    const uint32_t *quad_info;
    const uint8_t *logadd8;  /* [256] */
    const uint8_t *logadd_mirror; /* the batch kernels' LDS table, ready-made (ssw_host_model.inc) */
    unsigned long long *nfixed; /* optional: [0] running count of the frames kernel's exact
                                 * in-wave pass, moved to [1] (= last batch) here */
    int16_t *out;            /* [n_frames][n_sen] */
    int n_frames, n_cb, n_feat, n_density, n_sen, slot_stride, n_quads;
    int aw, zero; /* ms scorer: acoustic weight divisor, logmath zero at shift 10 */
    int raw;      /* ms scorer: 1 = skip the frame normalisation (the caller applies it over an
                   * active set, src/ms_mgau.c:342-364) */
    int tab_max;  /* largest entry of logadd8 (its entry 0) */
    int hb;       /* what every look-up of the folded table adds (senone_fold_hb, ssw_senone_lds.inc) */
    /* COMPACT instances (round 5, ssw_score_batch_compact): `out` holds, per utterance, rows of
     * its OWN states only -- what its forced alignment will read (src/state_align_search.c:
     * 186-189 activates just those senones) -- instead of [n_sen] rows: every senone is still
     * evaluated (the frame's best score is taken over all of them, src/ptm_mgau.c:394-400), but
     * 0.9 KB of a frame's 10 KB are stored.
     *   utt_of_frame [n_frames]           utterance of every frame
     *   cutt_off [n_utts + 1], crow_off [n_utts], cstride [n_utts]
     *                                     frame t of utterance u: row at out + crow_off[u] +
     *                                     (t - cutt_off[u]) * cstride[u] (int16 elements)
     *   cpos [n_utts][slot_stride]        per mixture-weight slot: BYTE offset of its score in
     *                                     the utterance's row, 0xffffffff = not wanted (beyond
     *                                     any row: the buffer store drops it); a dword each, so
     *                                     that a quad's four arrive as the four store offsets */
    const int32_t *utt_of_frame, *cutt_off, *cstride;
    const long long *crow_off;
    const uint32_t *cpos;
    int nfixed_acc; /* add the count to the last batch's instead of replacing it */
    int frame_base; /* COMPACT: batch frame number of this launch's frame 0 (a piece of a large
                     * batch: topn_* are offset, utt_of_frame / cutt_off are not) */
};

constexpr int SEN_MAX_THREADS = 1024;

typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));
typedef uint32_t uint2u __attribute__((ext_vector_type(2), aligned(2))); /* 2-byte aligned 8 bytes */
typedef uint32_t uint1u __attribute__((aligned(2)));                     /* 2-byte aligned 4 bytes */

__device__ __forceinline__ uint32_t
pk_min_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(ushort2v, a),
                                                                  __builtin_bit_cast(ushort2v, b)));
}

__device__ __forceinline__ uint32_t
pk_max_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(ushort2v, a),
                                                                  __builtin_bit_cast(ushort2v, b)));
}

/* One workgroup per FPB consecutive frames.  Senones are visited in "slot" order: grouped by
 * codebook, each run of consecutive ids (dense layout: each group) padded to a multiple of 4
 * (ssw_slot_layout.inc), so one lane owns 4 consecutive slots that
 * share their top-N block and fetches the 4 mixture weights of a (stream, codeword) row with one
 * dword load.  R = quads per thread.  Several frames per workgroup amortise the prologue, the
 * barriers and the launch of 704-thread groups, which is what bounded the one-frame version.
 *
 * The chain of fast_logmath_add steps (tied_mgau_common.h:100-117: x <- min(x, y) -
 * tab[|x - y|]) runs on TWO slots per register, 16 bits each, arranged so that a step is 4
 * vector instructions for the pair:
 *   - the step is x + G[d], d = x - y, G[d] = -tab[|d|] - max(d, 0): the minimum is folded
 *     into the table.  d <= wmax, the largest weight byte (x starts from a weight and only
 *     falls, y >= 0 relative to the stream's best codeword), so H[d] = Hb + G[d] is a byte
 *     (senone_fold_table, ssw_senone_lds.inc; the host refuses Hb > 255);
 *   - step k works on x' = x + Hb (k - 1) and leaves x' + H[d]: nothing is ever subtracted,
 *     the halves stay non-negative, below 2^16 (255 + 3 x 255), and cannot carry into each other;
 *   - the offsets are the same for every senone of the frame and cancel in `score - best`
 *     (src/ptm_mgau.c:394-400);
 *   - H comes from ONE byte table (4 neighbouring d share a bank word, so look-ups rarely
 *     conflict; a dword table per half was measured at 40 x the bank conflicts): the low
 *     half's entry with ds_read_u8, the high half's with ds_read_u8_d16_hi, which on gfx950
 *     delivers `byte << 16` with a zero low half (tools/microbench/d16_probe.hip).  The
 *     compiler does not select d16 loads on sramecc targets, so the look-ups of a batch of
 *     chains are inline asm, followed by one s_waitcnt through which their results pass;
 *   - the table stands around LDS address CZ (512; ms 1,024) and the look-up's address is
 *     CZ + d itself, never negative: z = x' + npz_k with npz_k = CZ - rel_k - Hb (k - 1) staged
 *     per item (16-bit wrap, as the packed add's), then z - the weight BYTE as it lies in the
 *     gathered mixture-weight dword (v_sub_u32_sdwa WORD_n - BYTE_m, one per half): y itself
 *     is never formed.
 * Per step and pair: v_pk_add_u16, two v_sub_u32_sdwa (one per half), the two look-ups,
 * v_add3_u32.
 * Round 3 as well: the 12 mixture-weight dwords of a quad and frame are fetched with buffer
 * loads whose resource has ADD_TID_ENABLE set (stride 4): address = wave base + row offset (the
 * VGPR read from LDS as it stands) + 4 x lane, no per-lane address add (addr_probe.hip). */
/* The chains of NS streams of one quad (2 slot pairs each), step by step; mw[f][k] = weights of
 * the 4 slots for codeword k of stream f, np[f] = its normalised scores; acc[p] += the pairs'
 * results. */
/* a + (one half of b, in both halves): v_pk_add_u16 with op_sel picking b's low (HI = 0) or
 * high (HI = 1) half for both lanes of the packed add */
template <int HI>
__device__ __forceinline__ uint32_t
pk_add_bcast_u16(uint32_t a, uint32_t b)
{
    uint32_t r;
    if (HI)
        asm("v_pk_add_u16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
    else
        asm("v_pk_add_u16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <int NS, int TOPN>
__device__ __forceinline__ void
quad_chains(const uint32_t (*mw)[TOPN], const uint2 *np, uint32_t (&acc)[2])
{
    /* np[f] = per codeword k = 1..3 of the stream, 16 bits each (x = . | 1 << 16, y = 2 | 3 <<
     * 16; the packed add broadcasts the half it needs): npz_k = CZ - rel_k - Hb (k - 1), rel_k =
     * its normalised score RELATIVE TO THE BEST CODEWORD'S.  Round 4: log-add commutes with a
     * common shift (min(x + c, y + c) - tab[|x - y|]), so the best codeword's score is taken
     * out of the chain -- its term is the weight as it stands -- and the three streams' best
     * scores go into the accumulator once per quad (the caller: asc2 starts from their sum). */
    constexpr int NC = 2 * NS;
    uint32_t x2[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        x2[c] = __builtin_amdgcn_perm(mw[c >> 1][0], mw[c >> 1][0],
                                      (c & 1) ? 0x0c030c02u : 0x0c010c00u);
#pragma unroll
    for (int k = 1; k < TOPN; ++k) {
        uint32_t tl[NC], th[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const uint32_t w = mw[c >> 1][k];
            const uint32_t z = k == 1 ? pk_add_bcast_u16<1>(x2[c], np[c >> 1].x)
                : k == 2              ? pk_add_bcast_u16<0>(x2[c], np[c >> 1].y)
                                      : pk_add_bcast_u16<1>(x2[c], np[c >> 1].y);
            /* CZ + x - y of each half = the look-up's address: the half of z minus the slot's
             * weight byte where it lies (slots 2 (c & 1) and 2 (c & 1) + 1 of the quad) */
            const uint32_t dlo = (z & 0xffffu) - ((w >> ((c & 1) ? 16 : 0)) & 0xffu);
            const uint32_t dhi = (z >> 16) - ((w >> ((c & 1) ? 24 : 8)) & 0xffu);
            asm volatile("ds_read_u8 %0, %2\n\tds_read_u8_d16_hi %1, %3"
                         : "=&v"(tl[c]), "=&v"(th[c]) : "v"(dlo), "v"(dhi));
        }
        if constexpr (NC == 6)
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(tl[0]), "+v"(tl[1]), "+v"(tl[2]), "+v"(tl[3]), "+v"(tl[4]),
                           "+v"(tl[5]), "+v"(th[0]), "+v"(th[1]), "+v"(th[2]), "+v"(th[3]),
                           "+v"(th[4]), "+v"(th[5]));
        else
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(tl[0]), "+v"(tl[1]), "+v"(th[0]), "+v"(th[1]));
#pragma unroll
        for (int c = 0; c < NC; ++c)
            x2[c] = x2[c] + tl[c] + th[c];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
        acc[c & 1] += x2[c];
}

/* the four mixture-weight rows of one stream of a quad (its slots' weights for the four codewords),
 * a dword each: ro = the rows' byte offsets as staged, soff = the round's offset */
__device__ __forceinline__ void
load_quad_rows(__amdgpu_buffer_rsrc_t mw_rsrc, uint4 ro, int soff, uint32_t (&mw)[4])
{
    mw[0] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(mw_rsrc, (int)ro.x, soff, 0);
    mw[1] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(mw_rsrc, (int)ro.y, soff, 0);
    mw[2] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(mw_rsrc, (int)ro.z, soff, 0);
    mw[3] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(mw_rsrc, (int)ro.w, soff, 0);
}

/* One frame of the ms scorer by the whole workgroup with the reference's own arithmetic
 * (src/ms_senone.c:314-362, src/ms_mgau.c:299-321): the frames the packed kernel marks.  Raw
 * top-N items and the log-add table straight from global memory (rare path); `scratch` = one
 * LDS int per wave.  Same slot layout, same output as ms_senone_kernel. */
template <int R, bool COMPACT = false>
__device__ __forceinline__ void
ms_exact_frame(const SenoneParams &P, int t, int tid, int nthr, int *scratch)
{
    const int n_cbf = P.n_cb * P.n_feat;
    /* the four clamped scores of quad q (no arrays kept between the two passes below: this
     * path is rare and must not cost the kernel registers or scratch) */
    auto quad_scores = [&](int q, int (&v)[4]) {
        const int cb = P.quad_cb[q];
        const uint8_t *mq = P.mixw + (size_t)q * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = 0;
        for (int f = 0; f < P.n_feat; ++f)
            ms_quad_scores(mq, f, P.n_density, P.slot_stride,
                           P.topn_cw[(size_t)t * n_cbf + cb * P.n_feat + f],
                           P.topn_sc[(size_t)t * n_cbf + cb * P.n_feat + f], P.zero, P.logadd8, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = ms_finish(v[j], 1); /* (aw != 1 stays with ms_senone_kernel) */
    };
    int best = INT_MAX;
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
        const int q = r * nthr + tid;
        if (q < P.n_quads) {
            int v[4];
            quad_scores(q, v);
            const short4 s4 = P.slot_sen[q];
            const int sj[4] = { s4.x, s4.y, s4.z, s4.w };
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (sj[j] >= 0)
                    best = v[j] < best ? v[j] : best;
        }
    }
    best = -wave_max_dpp(-best);
    lds_barrier(); /* the scratch words are free */
    if ((tid & 63) == 0)
        scratch[tid >> 6] = best;
    lds_barrier();
    for (int k = 0; k < (nthr >> 6); ++k)
        best = scratch[k] < best ? scratch[k] : best;
    int uu = 0;
    if (COMPACT)
        uu = P.utt_of_frame[P.frame_base + t];
    int16_t *orow = COMPACT
        ? P.out + P.crow_off[uu] + (long long)(P.frame_base + t - P.cutt_off[uu]) * P.cstride[uu]
        : P.out + (size_t)t * P.n_sen;
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
        const int q = r * nthr + tid;
        if (q < P.n_quads) {
            int v[4];
            quad_scores(q, v);
            const short4 s4 = P.slot_sen[q];
            const int sj[4] = { s4.x, s4.y, s4.z, s4.w };
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                /* final_score<true> (ssw_senone_common.inc) as text: through the call -- or
                 * through clamp_i16 -- the clamp is scheduled one instruction earlier in the 16
                 * MS COMPACT instances of ptm_senone_kernel, which stay byte-equal */
                int bs = v[j] - best; /* src/ms_mgau.c:314-320 */
                bs = bs > 32767 ? 32767 : bs;
                bs = bs < -32768 ? -32768 : bs;
                if (COMPACT) {
                    const uint32_t cp = P.cpos[(size_t)uu * P.slot_stride + 4 * q + j];
                    if (cp != 0xffffffffu)
                        orow[cp >> 1] = (int16_t)bs;
                } else if (sj[j] >= 0)
                    orow[sj[j]] = (int16_t)bs;
            }
        }
    }
}

/* Round 3: the workgroup is PERSISTENT.  It takes the units (FPB consecutive frames) blockIdx.x,
 * blockIdx.x + gridDim.x, ... and overlaps the latency-bound parts of neighbouring units with the
 * vector-bound main loop: the next unit's top-N items are fetched into registers before the
 * current unit's main loop starts, normalised into the OTHER half of a double-buffered LDS block
 * between the current unit's two barriers, and the current unit's output stores are issued and
 * left behind.  In the one-unit-per-group form every group of a round sat in its prologue (one
 * round trip to memory, three barriers), its main loop and its output phase at the same time as
 * all the others -- a third of a group's life was not main loop (profiles/r02_senone_timeline.txt).
 * Per unit now: two LDS-only barriers.  With gridDim.x = the number of units this is the old
 * kernel (small batches). */
/* MS = the ms scorer's senone_eval on the same machinery (round 3; src/ms_senone.c:314-362,
 * src/ms_mgau.c:299-321).  There the top-N block holds fden_k = ((int32)dist_k + 1023) >> 10,
 * descending, and a slot's stream score is logmath_add over fden_k - pdf_k: max(x, y) +
 * tab[|x - y|] (tab = 0 from 256 up) with the `zero` short-cuts.  Relative to the stream's best
 * codeword and negated, X = fden_0 - x, that is the PTM chain min(X, Y) - tab[|X - Y|] with
 * X_0 = pdf_0, Y_k = pdf_k + (fden_0 - fden_k); a difference beyond 640 is as good as 640 (the
 * table is 0 from 256 and X <= 255), so everything fits 16 bits with the folded table
 * around 1024.  The slot's score -sum_f fscr_f = sum_f X_f - sum_f fden_0f: the second sum is
 * one number per (frame, codebook), added up with LDS atomics where the PTM kernel takes its
 * normaliser, and the accumulator starts from it.  What this form cannot express -- a density
 * at or below logmath's zero (the short-cuts), a score beyond int16 (the clamps) -- marks the
 * frame, and marked frames are redone after the unit with the reference's own arithmetic
 * (ms_exact_frame).  aw != 1 and the un-normalised mode stay with ms_senone_kernel. */
template <int TOPN, int R, int FPB, int NF, bool MS, bool COMPACT = false>
__global__ void __launch_bounds__(SEN_MAX_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
ptm_senone_kernel(SenoneParams P)
{
    constexpr int MIRROR = MS ? 2 * SSW_LOGADD_MIRROR : SSW_LOGADD_MIRROR;
    constexpr int MID = MIRROR / 2;
    constexpr int MS_NMAX = 640; /* fden_0 - fden_k beyond this acts like this */
#ifdef SSW_TIMELINE_SEN
#define STL(k)                                                                               \
    if ((threadIdx.x & 63) == 0) {                                                           \
        int wv = blockIdx.x * 11 + (threadIdx.x >> 6);                                       \
        if (wv < 16384)                                                                      \
            g_timeline[wv * 6 + (k)] = __builtin_amdgcn_s_memtime();                        \
    }
#else
#define STL(k)
#endif
    STL(0)
    /* set-up, block minimum and output are short latency-bound phases that the rest of the
     * workgroup waits for: let them issue ahead of other groups' main loops */
    __builtin_amdgcn_s_setprio(3);
    /* NF = number of streams when known at compile time (0 = read it from P): with a constant
     * trip count the 12 row loads of a quad are all issued before the first log-add */
    const int n_feat = NF ? NF : P.n_feat;
    static_assert(TOPN == 4, "top-N block is packed 4 x 8 bit");
    extern __shared__ __align__(16) unsigned char smem[];
    const int n_cbf = P.n_cb * P.n_feat;
    /* The log-add table is indexed by the difference without a bound, as in the reference; x, y
     * <= 255 + 96 and the running value can dip 3 T below zero (the host refuses tables with
     * 351 + 3 T >= 512, so that MID + x - y >= 0; it is <= MID + 255).  It holds the folded
     * entries Hb - tab[|d|] - max(d, 0) at LDS address MID + d (this kernel has
     * no static LDS: its dynamic LDS starts at 0, which is what the look-ups' asm assumes).
     * The carve is SenoneCarve's (ssw_senone_lds.inc), from which launch_senone takes the byte
     * count: tab[MIRROR] | norm[3][FPB][NORM_W] | red[16] | item[2][n_cbf][FPB] 32 B |
     * stage_sc[pad64(FPB n_cbf)] int4 | stage_cw[..].  It stays written out here as typed-pointer
     * steps: taken from the struct's byte offsets the same addresses are computed by other
     * instructions and every instance's set-up is scheduled differently.
     * tests/harness/senone_lds_host.cpp holds these lines verbatim and compares them with the
     * struct region by region: change both together.  norm / red have three slots (unit i uses
     * slot i % 3): a slot is re-armed two barriers after its last reader and two before its next
     * writer. */
    uint8_t *s_tab = smem;
    /* norm: PTM [3][FPB][8] per-stream normalisers; MS [3][FPB][NORM_W] sums of fden_0 per codebook */
    const int NORM_W = MS ? ((P.n_cb + 7) & ~7) : SSW_MAX_FEAT;
    int *s_norm = reinterpret_cast<int *>(smem + MIRROR);
    int *s_red = s_norm + 3 * NORM_W * FPB; /* [0..11] block minima, [12..14] MS: marked frames per slot */
    /* normalised scores of the 4 codewords of every (frame, codebook, stream) plus the step
     * offset, in both halves */
    /* staged items, 32 bytes each, [half][codebook x stream][frame]: x y z w = byte offsets of
     * the 4 mixture-weight rows, then the 4 normalised scores (+ step offsets) 16 bits each in
     * two dwords.  Frame innermost: the FPB x NF items a quad reads sit at compile-time offsets
     * from ONE address (its codebook's), so nothing per (frame, stream) is kept in registers. */
    uint4 *s_item = reinterpret_cast<uint4 *>(s_red + 16);
    /* the next unit's raw items, fetched by LDS-DMA while the main loop runs (no registers, no
     * round trip to memory between two main loops): scores [FPB * n_cbf] int4, codewords
     * [FPB * n_cbf] (padded to whole waves) */
    const int n_item_pad = (FPB * n_cbf + 63) & ~63;
    int4 *s_stage_sc = reinterpret_cast<int4 *>(s_item + 2 * 2 * n_cbf * FPB);
    uint32_t *s_stage_cw = reinterpret_cast<uint32_t *>(s_stage_sc + n_item_pad);

    const int tid = threadIdx.x;
    const int nthr = blockDim.x;
    const uint32_t T = (uint32_t)P.tab_max;
    const uint32_t Hb = (uint32_t)P.hb;
    const int n_units = (P.n_frames + FPB - 1) / FPB;
    const int stride_u = (int)gridDim.x;
    int u = (int)blockIdx.x;
    if (u >= n_units)
        return;

    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u)
        __builtin_trap(); /* folds away: the dynamic LDS of a kernel without static LDS starts at 0 */

    /* the thread's item (frame, codebook, stream) of a unit: one item per thread (the host
     * launches nthr >= FPB * n_cbf), fetched into registers a unit ahead.  Which item is the
     * thread's does not change from unit to unit: frame my_fr of the unit, normaliser word
     * my_norm (within a slot), staged item my_item (within a half), first mixture-weight row
     * my_row0 of its stream -- packed into two registers. */
    uint32_t my_a, my_b;
    {
        /* (frame of the unit without a division: the set-up is issue-bound -- seven waves per
         * SIMD run it at the same moment -- and a 32-bit division is 20 instructions) */
        int fr = 0;
#pragma unroll
        for (int k = 1; k < FPB; ++k)
            fr += tid >= k * n_cbf ? 1 : 0;
        const int i = tid - fr * n_cbf, f = i % n_feat;
        const int nidx = MS ? fr * NORM_W + i / n_feat : fr * SSW_MAX_FEAT + f;
        my_a = (uint32_t)fr | (uint32_t)nidx << 4 | (uint32_t)(f * P.n_density) << 16;
        my_b = (uint32_t)(2 * (i * FPB + fr));
    }
    int4 sc0 = make_int4(0, 0, 0, 0);
    uint32_t cw0 = 0;
    auto item_live = [&](int unit) { /* the unit has this thread's frame (the last unit may not) */
        return tid < FPB * n_cbf && unit * FPB + (int)(my_a & 0xfu) < P.n_frames;
    };
    auto fetch_item = [&](int unit) {
        if (item_live(unit)) {
            sc0 = P.topn_sc[(size_t)unit * FPB * n_cbf + tid];
            cw0 = P.topn_cw[(size_t)unit * FPB * n_cbf + tid];
        }
    };
    /* the same fetch as LDS-DMA (global_load_lds: destination = M0 base + 16 or 4 bytes x
     * lane, the source address per lane), issued at the top of a main loop; the thread that
     * issued a piece is the one that reads it back, after its own s_waitcnt vmcnt(0).  Inline
     * asm: the compiler's own counted waits stay correct, these operations are simply older
     * than anything it waits for. */
    auto fetch_item_dma = [&](int unit) {
        if (item_live(unit)) {
            const int4 *gsc = P.topn_sc + ((size_t)unit * FPB * n_cbf + tid);
            const uint32_t *gcw = P.topn_cw + ((size_t)unit * FPB * n_cbf + tid);
            const uint32_t wave0 = (uint32_t)tid & ~63u;
            const uint32_t dst_sc = (uint32_t)__builtin_amdgcn_readfirstlane(
                (int)((uint32_t)(uintptr_t)(__attribute__((address_space(3))) int4 *)s_stage_sc + wave0 * 16u));
            const uint32_t dst_cw = (uint32_t)__builtin_amdgcn_readfirstlane(
                (int)((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)s_stage_cw + wave0 * 4u));
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                         "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                         "global_load_lds_dword %2, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(gsc), "v"(gcw), "s"(dst_sc), "s"(dst_cw) : "memory");
        }
    };
    auto take_item_dma = [&](int unit) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (item_live(unit)) {
            sc0 = s_stage_sc[tid];
            cw0 = s_stage_cw[tid];
        }
    };
    /* part 1 of a unit's set-up: per-stream normaliser, max over codebooks of (best >> 10),
     * src/ptm_mgau.c:271-278, combined with LDS atomics into slot `ns` */
    auto norm_item = [&](int unit, int ns) {
        if (item_live(unit)) {
            int *w = &s_norm[ns * FPB * NORM_W + (int)((my_a >> 4) & 0xfffu)];
            if (MS) {
                atomicAdd(w, sc0.x);
                /* a density near logmath's zero: the short-cuts of logmath_add could apply */
                if (sc0.w <= P.zero + 4096)
                    atomicOr(&s_red[12 + ns], 1 << (int)(my_a & 0xfu));
            } else
                atomicMax(w, sc0.x >> SSW_SENSCR_SHIFT);
        }
    };
    /* part 2: s = min(96, -((s >> 10) - norm)), src/ptm_mgau.c:284-290, and the row offsets,
     * into half `buf` of the LDS block */
    auto stage_item = [&](int unit, int ns, int buf) {
        if (item_live(unit)) {
            const int norm = s_norm[ns * FPB * NORM_W + (int)((my_a >> 4) & 0xfffu)];
            const int v[4] = { sc0.x, sc0.y, sc0.z, sc0.w };
            uint32_t sp[4];
#pragma unroll
            for (int k = 0; k < TOPN; ++k) {
                int q;
                if (MS) {
                    q = v[0] - v[k]; /* >= 0: the block is sorted by density */
                    q = q > MS_NMAX ? MS_NMAX : q;
                } else {
                    q = -((v[k] >> SSW_SENSCR_SHIFT) - norm);
                    q = q > SSW_MAX_NEG_ASCR ? SSW_MAX_NEG_ASCR : q;
                }
                sp[k] = (uint32_t)(q & 0x3ff);
            }
            /* the chain works relative to the best codeword's score (the block is sorted: it is
             * the smallest); that score itself travels in the item's third dword, in both
             * halves, and starts the accumulator (MS: already relative, sp[0] = 0).  What is
             * staged per codeword k >= 1 is npz_k = MID - rel_k - Hb (k - 1), which the chain
             * adds to its running value to get the look-up's address less the weight byte
             * (quad_chains); it may be negative and wraps within its 16 bits, as the packed add
             * does */
            const uint32_t e0 = MS ? 0u : sp[0];
#pragma unroll
            for (int k = 0; k < TOPN; ++k)
                sp[k] = k == 0 ? 0u
                               : ((uint32_t)MID - (sp[k] - e0) - Hb * (uint32_t)(k - 1)) & 0xffffu;
            /* MS: the accumulator ends at sum_f (X_f + 3 Hb) + a0n = sum_f X_f - (sum of fden_0),
             * a0n = -(sum of fden_0) - 3 Hb per stream.  X_f >= -3 T and <= 255, so with
             * a0 = -(sum of fden_0) - 3 T per stream in 0 .. 30,000 every slot's end value lies
             * in 0 .. 30,000 + n_feat (255 + 3 T) < 2^15 (T <= 21: ms_takes_packed_kernel):
             * otherwise the frame is marked, as it always was.  a0n itself may be negative
             * (Hb > T): then the low half starts from a0n + 2^16 and, since it ends in
             * 0 .. 2^16 - 1 and 32-bit sums do not depend on their order, carries into the high
             * half exactly once -- which therefore starts one lower.  Nothing else can carry: a
             * slot's sum of streams is at most n_feat (255 + 3 x 255) = 8,160. */
            const int a0n = -norm - (int)(3u * Hb) * n_feat;
            if (MS) {
                const int a0 = -norm - (int)(3u * T) * n_feat;
                if (a0 < 0 || a0 > 30000)
                    atomicOr(&s_red[12 + ns], 1 << (int)(my_a & 0xfu));
            }
            uint4 *dst = s_item + (2 * buf * n_cbf * FPB + (int)my_b);
            const uint32_t row0 = my_a >> 16;
            dst[0] = make_uint4(__umul24(row0 + (cw0 & 0xffu), (uint32_t)P.slot_stride),
                                __umul24(row0 + ((cw0 >> 8) & 0xffu), (uint32_t)P.slot_stride),
                                __umul24(row0 + ((cw0 >> 16) & 0xffu), (uint32_t)P.slot_stride),
                                __umul24(row0 + (cw0 >> 24), (uint32_t)P.slot_stride));
            reinterpret_cast<uint2 *>(dst + 1)[0]
                = make_uint2(sp[0] | (sp[1] << 16), sp[2] | (sp[3] << 16));
            /* what the quads of this codebook start their sums from, in both halves: MS the
             * frame's offset (stream 0's item is the one read), PTM this stream's best score */
            /* (PTM: a slot ends at most at n_feat (255 + 3 x 255 + 96) = 8,928 < 2^15) */
            reinterpret_cast<uint32_t *>(dst + 1)[2] = MS
                ? (uint32_t)(a0n & 0xffff) | (uint32_t)((a0n - (a0n < 0 ? 1 : 0)) & 0xffff) << 16
                : e0 * 0x10001u;
        }
    };

    /* ---- set-up of the group's first unit: one round trip to memory, the item and the table
     * entries fetched before the first barrier (the barriers here wait for LDS only) ---- */
    fetch_item(u);
    /* (the quads' constants travel in the same round trip; they are settled further down) */
    uint32_t qi_ld[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int q = r * nthr + tid;
        qi_ld[r] = q < P.n_quads ? P.quad_info[q] : 0u;
    }
    /* the folded table comes ready-made (ssw_host_model.inc): nthr >= 256, one or
     * two dwords per thread */
    constexpr int TAB_DW = MIRROR / 4;
    uint32_t tv[(TAB_DW + 255) / 256] = {};
#pragma unroll
    for (int j = 0; j < (TAB_DW + 255) / 256; ++j) {
        const int e = tid + j * nthr;
        if (e < TAB_DW)
            tv[j] = reinterpret_cast<const uint32_t *>(P.logadd_mirror)[e];
    }
    if (tid < 3 * NORM_W * FPB)
        s_norm[tid] = MS ? 0 : SSW_WORST_SCORE;
    if (3 * NORM_W * FPB > nthr) /* (not with the shapes the host launches: workgroup-uniform) */
        for (int i = tid + nthr; i < 3 * NORM_W * FPB; i += nthr)
            s_norm[i] = MS ? 0 : SSW_WORST_SCORE;
    if (tid < 16)
        s_red[tid] = tid < 12 ? INT_MAX : 0;
    if (P.nfixed != nullptr && blockIdx.x == 0 && tid == 0)
        move_exact_count(P.nfixed, P.nfixed_acc);
    lds_barrier();
    norm_item(u, 0);
#pragma unroll
    for (int j = 0; j < (TAB_DW + 255) / 256; ++j)
        if (tid + j * nthr < TAB_DW)
            reinterpret_cast<uint32_t *>(s_tab)[tid + j * nthr] = tv[j];
    lds_barrier();
    stage_item(u, 0, 0);

    /* mixture-weight rows through a buffer resource with ADD_TID_ENABLE (word 3 bit 23) and
     * stride 4: address = base + soffset + voffset + 4 x lane.  base = the wave's first quad of
     * round 0, soffset = the round's 4 * r * nthr, voffset = the row's byte offset from LDS;
     * the range check in this mode is lane < num_records. */
    const __amdgpu_buffer_rsrc_t mw_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(P.mixw)
            + (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)tid & ~63u) * 4),
        (short)4, 64, (int)(1u << 23));
    /* per quad, in one register (from quad_info): its first senone id s0 << 17 | byte offset of
     * its codebook's staged items within a half (a multiple of 32 below 2^15: an item is 32 bytes
     * and every thread of the group, 1,024 at the most, has one of its own) |
     * bits 0..2: n, the quad's first n slots hold s0 .. s0 + n - 1 (0 = no such form).  Settled
     * here, so that no load is pending when the loop starts. */
    uint32_t qoff[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t qi = qi_ld[r];
        qoff[r] = (qi >> 24) * (uint32_t)(n_feat * FPB * 32) | ((qi >> 17) & 7u) | (qi << 17);
    }

    for (int it = 0;; ++it) {
        const int t0 = u * FPB;
        const int nfr = (P.n_frames - t0) < FPB ? (P.n_frames - t0) : FPB;
        const int u_next = u + stride_u;
        const bool has_next = u_next < n_units; /* workgroup-uniform */
        const int buf = it & 1, slot = it % 3, slot_next = (it + 1) % 3;
        lds_barrier();          /* half `buf` of the LDS block is staged */
        if (has_next)
            fetch_item_dma(u_next); /* lands in LDS during the main loop */
        STL(1)
        /* senone combine, src/ptm_mgau.c:342-395: asc2[..][p] = slots 2p (low half), 2p + 1 (high) */
        uint32_t asc2[R][FPB][2];
        const uint4 *item_b = s_item + 2 * buf * n_cbf * FPB;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int q = r * nthr + tid;
            const int soff = __builtin_amdgcn_readfirstlane(r * nthr * 4);
#pragma unroll
            for (int fr = 0; fr < FPB; ++fr) {
                const uint32_t dead = (q < P.n_quads && fr < nfr) ? 0u : 0xffffffffu;
                asc2[r][fr][0] = asc2[r][fr][1] = dead;
            }
            if (q < P.n_quads) {
                const uint4 *item_cb = reinterpret_cast<const uint4 *>(
                    reinterpret_cast<const unsigned char *>(item_b) + (qoff[r] & 0x1ffe0u));
                /* + 2 * (f * FPB + fr): immediate offsets */
                if (MS) {
#pragma unroll
                    for (int fr = 0; fr < FPB; ++fr)
                        if (fr < nfr)
                            asc2[r][fr][0] = asc2[r][fr][1]
                                = reinterpret_cast<const uint32_t *>(item_cb + 2 * fr + 1)[2];
                }
#pragma unroll
                for (int fr = 0; fr < FPB; ++fr) {
                    /* Issue priority falls with progress through the main loop (4 levels).  With
                     * equal priorities the SIMD serves its oldest wave first, the waves of a
                     * workgroup reach the barrier far apart and the last ones run with few
                     * neighbours to hide their look-up latency; letting the laggards pass keeps
                     * them together (measured: 45.9 -> 42.8 us per 4096 frames). */
                    {
                        constexpr int NI = R * FPB;
                        const int item = r * FPB + fr;
                        if (item * 4 < NI)
                            __builtin_amdgcn_s_setprio(3);
                        else if (item * 4 < 2 * NI)
                            __builtin_amdgcn_s_setprio(2);
                        else if (item * 4 < 3 * NI)
                            __builtin_amdgcn_s_setprio(1);
                        else
                            __builtin_amdgcn_s_setprio(0);
                    }
                    if (fr < nfr) {
                        if (NF) {
                            uint32_t mw[NF ? NF : 1][TOPN];
                            uint2 np[NF ? NF : 1];
                            uint32_t zsum = 0; /* the streams' best scores, in both halves */
#pragma unroll
                            for (int f = 0; f < NF; ++f) {
                                const uint4 ro = item_cb[2 * (f * FPB + fr)];
                                const uint4 sc4 = item_cb[2 * (f * FPB + fr) + 1];
                                np[f] = make_uint2(sc4.x, sc4.y);
                                if (!MS)
                                    zsum += sc4.z;
                                load_quad_rows(mw_rsrc, ro, soff, mw[f]);
                            }
                            if (!MS) {
                                asc2[r][fr][0] += zsum;
                                asc2[r][fr][1] += zsum;
                            }
                            quad_chains<NF ? NF : 1, TOPN>(mw, np, asc2[r][fr]);
                        } else
                        for (int f = 0; f < n_feat; ++f) {
                            const uint4 ro = item_cb[2 * (f * FPB + fr)];
                            const uint4 sc4 = item_cb[2 * (f * FPB + fr) + 1];
                            const uint2 np = make_uint2(sc4.x, sc4.y);
                            if (!MS) {
                                asc2[r][fr][0] += sc4.z;
                                asc2[r][fr][1] += sc4.z;
                            }
                            uint32_t mw[1][TOPN];
                            load_quad_rows(mw_rsrc, ro, soff, mw[0]);
                            quad_chains<1, TOPN>(mw, &np, asc2[r][fr]);
                        }
                    }
                }
            }
        }
        STL(2)
        __builtin_amdgcn_s_setprio(3);
        /* the next unit's item (in LDS by now): no registers held across the main loop, no
         * round trip to memory here */
        if (has_next)
            take_item_dma(u_next);
        /* COMPACT: where this unit's scores go -- the utterance of each of its frames (wave-
         * uniform) and, per quad, the four slots' byte offsets in that utterance's compact row
         * (8 bytes, neighbouring lanes read neighbouring quads; the table is the same for all
         * the utterance's frames, so it comes from L2) -- requested here, used after the barrier */
        int c_utt[FPB];
        uint4 c_pos[R][FPB];
        if (COMPACT) {
#pragma unroll
            for (int fr = 0; fr < FPB; ++fr) {
                c_utt[fr] = fr < nfr
                    ? __builtin_amdgcn_readfirstlane(P.utt_of_frame[P.frame_base + t0 + fr]) : 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int q = r * nthr + tid;
                    c_pos[r][fr] = (q < P.n_quads && fr < nfr)
                        ? *reinterpret_cast<const uint4 *>(P.cpos + (size_t)c_utt[fr] * P.slot_stride + 4 * q)
                        : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
                }
            }
        }
        /* block minimum of every frame: wave minimum by DPP, one LDS atomic per (frame, wave);
         * and part 1 of the next unit's set-up, under the same barrier */
#pragma unroll
        for (int fr = 0; fr < FPB; ++fr) {
            /* padding slots carry the weights of their quad's first slot (host), so they cannot
             * win the minimum; quads beyond the model and frames beyond the batch hold 0xffff */
            uint32_t b2 = 0xffffffffu;
#pragma unroll
            for (int r = 0; r < R; ++r)
                b2 = pk_min_u16(b2, pk_min_u16(asc2[r][fr][0], asc2[r][fr][1]));
            const int lo = (int)(b2 & 0xffffu), hi = (int)(b2 >> 16);
            const int wmin = -wave_max_dpp(-(lo < hi ? lo : hi));
            if ((tid & 63) == 0)
                atomicMin(&s_red[slot * FPB + fr], wmin);
        }
        if (has_next)
            norm_item(u_next, slot_next);
        lds_barrier();
        int best[FPB];
#pragma unroll
        for (int fr = 0; fr < FPB; ++fr)
            best[fr] = s_red[slot * FPB + fr];
        const int marked = MS ? s_red[12 + slot] : 0; /* workgroup-uniform */
        if (MS && tid == 0)
            s_red[12 + (it + 2) % 3] = 0; /* the previous unit's marks: every reader is past them */
        STL(3)
        if (COMPACT) {
            /* Scattered 2-byte stores, one per wanted slot, through a buffer resource that spans
             * the frame's compact row; only the lanes that HAVE a wanted slot (9 % of them)
             * execute a store.  What was measured on the way (one box, three rounds each, 2048
             * utterances; the full-row kernel: 134 us per 16 K frames):
             *   - all 64 lanes store and the unwanted slots' offsets lie beyond the row, so that
             *     the address unit drops them (no exec-mask code at all): 148 us -- the address
             *     unit's time goes with the lanes it is handed, dropped or not; halving the
             *     instructions around the stores (dword offsets, d16_hi) changed nothing;
             *   - a wave-local transposition through LDS (the wave's 256 scores side by side, the
             *     plan's compacted list of wanted slots, ONE store per lane and round): 158 us --
             *     two wave-level fences per round and 38 spilt registers;
             *   - this form, a compare and an exec-masked store per slot: 132-135 us, score_ms
             *     33.3 -> 31.4 at 2048 utterances (tools/r05_ab_compact.sh). */
#pragma unroll
            for (int fr = 0; fr < FPB; ++fr) {
                if (fr < nfr) {
                    const int uu = c_utt[fr];
                    const int stride = __builtin_amdgcn_readfirstlane(P.cstride[uu]);
                    const long long ro = P.crow_off[uu]
                        + (long long)(P.frame_base + t0 + fr
                                      - __builtin_amdgcn_readfirstlane(P.cutt_off[uu])) * stride;
                    /* every word of the resource declared wave-uniform: left as vector values
                     * the compiler wraps each store in a waterfall loop (12 instructions) */
                    const uintptr_t rb = reinterpret_cast<uintptr_t>(P.out + ro);
                    const uint32_t rb_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)rb);
                    const uint32_t rb_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(rb >> 32));
                    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
                        reinterpret_cast<void *>(((uintptr_t)rb_hi << 32) | rb_lo), (short)0,
                        stride * 2, 0x00020000);
                    const uint32_t b2 = (uint32_t)best[fr] * 0x10001u;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const uint32_t lo2 = asc2[r][fr][0] - b2, hi2 = asc2[r][fr][1] - b2;
                        const uint4 cp = c_pos[r][fr];
                        /* exec-masked, the high halves with buffer_store_short_d16_hi (no shift) */
                        if (cp.x != 0xffffffffu)
                            __builtin_amdgcn_raw_buffer_store_b16((short)(lo2 & 0xffffu), orsrc, (int)cp.x, 0, 0);
                        if (cp.y != 0xffffffffu)
                            asm volatile("buffer_store_short_d16_hi %0, %1, %2, 0 offen"
                                         :: "v"(lo2), "v"(cp.y), "s"(orsrc) : "memory");
                        if (cp.z != 0xffffffffu)
                            __builtin_amdgcn_raw_buffer_store_b16((short)(hi2 & 0xffffu), orsrc, (int)cp.z, 0, 0);
                        if (cp.w != 0xffffffffu)
                            asm volatile("buffer_store_short_d16_hi %0, %1, %2, 0 offen"
                                         :: "v"(hi2), "v"(cp.w), "s"(orsrc) : "memory");
                    }
                }
            }
        } else
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int q = r * nthr + tid;
            if (q < P.n_quads) {
                /* The quad's first n slots hold the senones s0 .. s0 + n - 1 (prefix layout:
                 * every quad).  n = 4 (19 quads in 20): one 8-byte store per frame, neighbouring
                 * lanes write neighbouring chunks; n < 4 (the end of a run of ids): a 4-byte
                 * store for n & 2, a 2-byte store for n & 1 -- two exec-masked stores at the
                 * most, no per-slot test and no per-slot id.  n = 0 (dense layout only: a quad
                 * that straddles two runs): a store per slot, ids from global memory. */
                /* (what the stores derive from a quad's constants -- offsets, flags, the index
                 * of its ids -- is worked out HERE, every unit: left to the compiler it is
                 * hoisted out of the unit loop and held in registers across the main loop) */
                uint32_t qo = qoff[r];
                asm volatile("" : "+v"(qo));
                const uint32_t n = qo & 7u;
                const uint32_t boff = (qo >> 16) & 0xfffeu; /* 2 s0: bytes into the frame's row */
                /* score - best (src/ptm_mgau.c:394-400; both < 2^15 here, so the int16
                 * arithmetic of the reference cannot wrap); the frames' rows are wave-uniform
                 * addresses, + a 32-bit offset per lane */
                uint2u pk[FPB];
                unsigned char *orow[FPB];
#pragma unroll
                for (int fr = 0; fr < FPB; ++fr) {
                    const uint32_t b2 = (uint32_t)best[fr] * 0x10001u;
                    pk[fr].x = asc2[r][fr][0] - b2;
                    pk[fr].y = asc2[r][fr][1] - b2;
                    orow[fr] = reinterpret_cast<unsigned char *>(P.out + (size_t)(t0 + fr) * P.n_sen);
                }
                if (n == 4) {
#pragma unroll
                    for (int fr = 0; fr < FPB; ++fr)
                        if (fr < nfr)
                            *reinterpret_cast<uint2u *>(orow[fr] + boff) = pk[fr];
                } else if (n != 0) {
                    if (n & 2u) {
#pragma unroll
                        for (int fr = 0; fr < FPB; ++fr)
                            if (fr < nfr)
                                *reinterpret_cast<uint1u *>(orow[fr] + boff) = pk[fr].x;
                    }
                    if (n & 1u) {
                        const uint32_t boff1 = boff + 2 * (n & 2u);
#pragma unroll
                        for (int fr = 0; fr < FPB; ++fr)
                            if (fr < nfr)
                                *reinterpret_cast<uint16_t *>(orow[fr] + boff1)
                                    = (uint16_t)(((n & 2u) ? pk[fr].y : pk[fr].x) & 0xffffu);
                    }
                } else {
                    uint32_t lane = (uint32_t)tid;
                    asm volatile("" : "+v"(lane));
                    const short4 s4 = P.slot_sen[(uint32_t)(r * nthr) + lane];
                    const int sj[4] = { s4.x, s4.y, s4.z, s4.w };
#pragma unroll
                    for (int fr = 0; fr < FPB; ++fr) {
                        if (fr < nfr) {
                            const int16_t v[4]
                                = { (int16_t)(pk[fr].x & 0xffffu), (int16_t)(pk[fr].x >> 16),
                                    (int16_t)(pk[fr].y & 0xffffu), (int16_t)(pk[fr].y >> 16) };
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (sj[j] >= 0)
                                    reinterpret_cast<int16_t *>(orow[fr])[sj[j]] = v[j];
                        }
                    }
                }
            }
        }
        STL(4)
        if (MS && marked != 0) {
            /* frames this form cannot express: redone with the reference's own arithmetic */
            for (int fr = 0; fr < nfr; ++fr)
                if ((marked >> fr) & 1)
                    ms_exact_frame<R, COMPACT>(P, t0 + fr, tid, nthr, reinterpret_cast<int *>(s_stage_cw));
        }
        if (!has_next)
            break;
        /* part 2 of the next unit's set-up into the other half; re-arm the slots: norm `slot`
         * (read before the barrier above at the latest, written again two units on) and red
         * `slot_next` (last read a unit ago, written after the next barrier) */
        stage_item(u_next, slot_next, buf ^ 1);
        if (tid < NORM_W * FPB)
            s_norm[slot * NORM_W * FPB + tid] = MS ? 0 : SSW_WORST_SCORE;
        if (tid < FPB)
            s_red[slot_next * FPB + tid] = INT_MAX;
        u = u_next;
    }
#undef STL
}

/* One frame with an explicit active set: the compallsen = no half of ptm_mgau_frame_eval
 * (src/ptm_mgau.c:264-403).  cb_mask (a bit per codebook, passed by value) is the activity the
 * top-N block was computed with (the history slot's mgau_active): the per-stream normaliser runs
 * over active codebooks only and
 * senones of inactive codebooks see 96 for all their scores (:353-364).  sen_bits marks the
 * senones of the delta list (bridge entries included); the best score is taken over them, and,
 * as in the reference, it is subtracted from ALL n_sen entries, the others starting from 0. */
struct SenoneFrameParams {
    const uint32_t *topn_cw;
    const int4 *topn_sc;
    const uint8_t *mixw, *quad_cb, *logadd8;
    unsigned long long cb_mask[4];
    const uint32_t *sen_bits; /* one bit per senone of the delta list; NULL = every senone */
    const short4 *slot_sen;
    int16_t *out;     /* [n_sen] final scores (may be host-mapped memory: written once, never read) */
    int16_t *raw;     /* [n_sen] device scratch for the un-normalised scores */
    int n_cb, n_feat, n_density, n_sen, slot_stride, n_quads;
};

/* The one-frame vtable call (VERDICT r1 item 4): no stream synchronise, no blocking copy.
 *   1. the exact top-N step of every codebook x stream (a wave each, as ptm_topn_chain_kernel);
 *   2. every group normalises the top-N block for itself (126 items) and combines ONE slot per
 *      thread; the frame's best score by an atomic minimum;
 *   3. score - best, eight senones per thread, written to pinned host memory in 16-byte pieces
 *      (byte-wise accesses to host memory cross the link one by one); the group that finishes
 *      last stores the call's sequence number behind them (system-scope release): the host spins
 *      on that word instead of synchronising the stream.
 * Either as three launches in a row on the stream (the default) or as ONE launch with a
 * device-wide barrier between the parts (PHASE 0; the grid is small -- 32 groups for en-us --
 * hence resident as a whole, which makes a barrier on a counter safe; its spin is bounded).  The
 * two take the same time.  The counter only grows (the host passes the value it had before the
 * call), so nothing has to be reset between calls. */
struct FrameFusedParams {
    ChainParams C;
    SenoneFrameParams S; /* S.out = pinned host memory, S.raw = device scratch */
    unsigned *counter;   /* device */
    int *gbest;          /* device: the frame's best score, INT_MAX between calls */
    int *done;           /* pinned host: set to `seq` when the scores are out */
    unsigned base;       /* value of *counter before this call */
    int seq, run_topn;
};

__device__ __forceinline__ void
small_grid_barrier(unsigned *ctr, unsigned target)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        atomicAdd(ctr, 1u);
        /* bounded (~50 ms): a counter that got out of step must end in an error on the host
         * (no sequence number arrives), never in a kernel that spins for ever */
        for (int spins = 0; spins < (1 << 21)
             && (int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0;
             ++spins)
            __builtin_amdgcn_s_sleep(1);
        __threadfence();
    }
    __syncthreads();
}

/* PHASE 0: the whole call in one launch, with the two device-wide barriers described above.
 * PHASE 1 / 2 / 3: its three parts as launches of their own, one after the other on the stream --
 * measured faster: two dependent kernels follow each other within ~1 us here, a barrier whose
 * atomics and polls cross the XCDs costs ~5 us.  The frame's best score then sits in one of two
 * words by the call's parity, and part 3 re-arms the other one for the next call. */
template <int PHASE>
__global__ void __launch_bounds__(256)
ptm_frame_kernel(FrameFusedParams Q)
{
    __shared__ uint8_t s_tab[SSW_LOGADD_LDS];
    __shared__ int s_norm[SSW_MAX_FEAT];
    __shared__ int s_red[4];
    extern __shared__ __align__(16) unsigned char smem[];
    const SenoneFrameParams &P = Q.S;
    const int n_cbf = P.n_cb * P.n_feat;
    uint32_t *s_ns4 = reinterpret_cast<uint32_t *>(smem);
    uint32_t *s_cw4 = s_ns4 + n_cbf;
    const int tid = threadIdx.x, nthr = blockDim.x, G = gridDim.x;
    int *gbest = Q.gbest + (PHASE == 0 ? 0 : (Q.seq & 1));

    if ((PHASE == 0 && Q.run_topn) || PHASE == 1)
        topn_chain_wave<13, 2, 4>(
            Q.C, __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))),
            threadIdx.x & 63, Q.S.cb_mask);
    if (PHASE == 1)
        return;
    auto cb_on = [&](int cbk) { return (P.cb_mask[cbk >> 6] >> (cbk & 63)) & 1ull; };
    /* what does not depend on the top-N block is fetched first (a dependent round trip to memory
     * costs ~0.8 us here): the thread's slot (the grid covers every slot: one per thread), its
     * senone, whether that is listed, and the activity of the eight senones it writes out */
    const int sl = blockIdx.x * nthr + tid;
    int sen = -1, cb = 0;
    const int c_out = blockIdx.x * nthr + tid; /* chunk of 8 senones this thread writes out */
    uint32_t act8 = 0;
    if (PHASE == 0 || PHASE == 2) {
        logadd_table_to_lds(s_tab, P.logadd8, tid, nthr);
        if (tid < SSW_MAX_FEAT)
            s_norm[tid] = SSW_WORST_SCORE;
        if (sl < P.n_quads * 4) {
            const short4 s4 = P.slot_sen[sl >> 2];
            const int sj[4] = { s4.x, s4.y, s4.z, s4.w };
            sen = sj[sl & 3];
            cb = P.quad_cb[sl >> 2];
            if (sen >= 0 && P.sen_bits != nullptr && !((P.sen_bits[sen >> 5] >> (sen & 31)) & 1u))
                sen = -1;
        }
    }
    if ((PHASE == 0 || PHASE == 3) && c_out < (P.n_sen + 7) / 8) {
        const int left = P.n_sen - c_out * 8; /* senones of this chunk: 8, fewer in the last */
        act8 = P.sen_bits != nullptr ? (P.sen_bits[c_out >> 2] >> (8 * (c_out & 3))) & 0xffu : 0xffu;
        act8 &= left >= 8 ? 0xffu : (1u << left) - 1u;
    }
    if (PHASE == 0)
        small_grid_barrier(Q.counter, Q.base + (unsigned)G);
    else
        __syncthreads();

    int best = INT_MAX;
    if (PHASE == 0 || PHASE == 2) {
        /* codebook_norm (src/ptm_mgau.c:264-295) over the active codebooks, per group */
        for (int i = tid; i < n_cbf; i += nthr)
            if (cb_on(i / P.n_feat))
                atomicMax(&s_norm[i % P.n_feat], P.topn_sc[i].x >> SSW_SENSCR_SHIFT);
        __syncthreads();
        for (int i = tid; i < n_cbf; i += nthr) {
            s_ns4[i] = ptm_norm_pack4(P.topn_sc[i], s_norm[i % P.n_feat], cb_on(i / P.n_feat) != 0ull);
            s_cw4[i] = P.topn_cw[i];
        }
        __syncthreads();
        /* senone_eval (src/ptm_mgau.c:326-403): one slot per thread */
        if (sen >= 0) {
            const int a = ptm_slot_score(P.mixw + sl, P.n_feat, P.n_density, P.slot_stride,
                                         s_cw4 + cb * P.n_feat, s_ns4 + cb * P.n_feat, s_tab);
            P.raw[sen] = (int16_t)a;
            best = a;
        }
        best = -wave_max_dpp(-best);
        if ((tid & 63) == 0)
            s_red[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
            int b = s_red[0];
            for (int w = 1; w < (nthr >> 6); ++w)
                b = s_red[w] < b ? s_red[w] : b;
            if (b != INT_MAX)
                atomicMin(gbest, b);
        }
    }
    if (PHASE == 2)
        return;
    if (PHASE == 0)
        small_grid_barrier(Q.counter, Q.base + 2u * (unsigned)G);

    /* senone_scores[i] -= bestscore for ALL n_sen entries, the unlisted ones starting from 0
     * (src/ptm_mgau.c:392-400) */
    best = __hip_atomic_load(gbest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint4 *hout = reinterpret_cast<uint4 *>(P.out);
    if (c_out < (P.n_sen + 7) / 8) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t pair = 0;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int sn = c_out * 8 + k * 2 + e;
                int16_t cur = 0;
                if ((act8 >> (k * 2 + e)) & 1u)
                    cur = P.raw[sn];
                const int16_t o = (int16_t)((int)cur - best);
                pair |= (uint32_t)(uint16_t)o << (16 * e);
            }
            w[k] = pair;
        }
        hout[c_out] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        const unsigned tk = atomicAdd(Q.counter, 1u);
        const unsigned last = PHASE == 0 ? 3u * (unsigned)G - 1u : (unsigned)G - 1u;
        if (tk - Q.base == last) { /* every group's scores are out */
            if (PHASE == 0)
                *gbest = INT_MAX;
            else
                Q.gbest[(Q.seq + 1) & 1] = INT_MAX; /* the next call's word */
            __hip_atomic_store(Q.done, Q.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

/* K3b: senone_eval + frame normalisation of the ms scorer (src/ms_senone.c:314-362,
 * src/ms_mgau.c:299-321).  Same slot order and quad-per-lane layout as ptm_senone_kernel; the
 * top-N block holds fden = ((int32)dist + 1023) >> 10 per codeword. */
template <int R, int NF> /* NF = streams when known at compile time (0: read from P) */
__global__ void __launch_bounds__(SEN_MAX_THREADS)
ms_senone_kernel(SenoneParams P)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int n_cbf = P.n_cb * P.n_feat;
    /* LDS: static logadd[256] (constant address, folds into the lookups), then the dynamic
     * carve, MsSenoneCarve (ssw_senone_lds.inc) */
    __shared__ uint8_t s_tab[256];
    const MsSenoneCarve carve(n_cbf);
    int4 *s_fd = reinterpret_cast<int4 *>(smem + carve.fd());
    uint32_t *s_cw4 = reinterpret_cast<uint32_t *>(smem + carve.cw4());
    int *s_red = reinterpret_cast<int *>(smem + carve.red());

    const int t = blockIdx.x;
    const int tid = threadIdx.x;
    const int nthr = blockDim.x;
    if (tid < 256)
        s_tab[tid] = P.logadd8[tid];
    if (tid < n_cbf) {
        s_fd[tid] = P.topn_sc[(size_t)t * n_cbf + tid];
        s_cw4[tid] = P.topn_cw[(size_t)t * n_cbf + tid];
    }
    if (P.nfixed != nullptr && t == 0 && tid == 0)
        move_exact_count(P.nfixed, P.nfixed_acc);
    lds_barrier();

    const int n_feat = NF ? NF : P.n_feat;
    int scr[R][4];
    short4 sen4[R];
    int best = INT_MAX;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int q = r * nthr + tid;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            scr[r][j] = 0;
        sen4[r] = make_short4(-1, -1, -1, -1);
        if (q < P.n_quads) {
            const int cb = P.quad_cb[q];
            const uint8_t *mq = P.mixw + (size_t)q * 4;
            sen4[r] = P.slot_sen[q];
#pragma unroll
            for (int f = 0; f < n_feat; ++f)
                ms_quad_scores(mq, f, P.n_density, P.slot_stride, s_cw4[cb * n_feat + f],
                               s_fd[cb * n_feat + f], P.zero, s_tab, scr[r]);
            const int sj[4] = { sen4[r].x, sen4[r].y, sen4[r].z, sen4[r].w };
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = ms_finish(scr[r][j], P.aw); /* (wave-uniform; 1 is the default) */
                scr[r][j] = v;
                if (sj[j] >= 0)
                    best = v < best ? v : best;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        int o = __shfl_xor(best, off, WAVE);
        best = o < best ? o : best;
    }
    if ((tid & 63) == 0)
        s_red[tid >> 6] = best;
    lds_barrier();
    {   /* every wave folds the partials itself: one barrier */
        int b = INT_MAX;
        for (int k = 0; k < (nthr >> 6); ++k)
            b = s_red[k] < b ? s_red[k] : b;
        best = P.raw ? 0 : b;
    }
    int16_t *orow = P.out + (size_t)t * P.n_sen;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int q = r * nthr + tid;
        if (q < P.n_quads) {
            const int sj[4] = { sen4[r].x, sen4[r].y, sen4[r].z, sen4[r].w };
            int16_t v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                v[j] = final_score<true>(scr[r][j], best);
            if (sj[0] >= 0 && sj[1] == sj[0] + 1 && sj[2] == sj[0] + 2 && sj[3] == sj[0] + 3) {
                short4u pk = { v[0], v[1], v[2], v[3] }; /* consecutive ids: one 8-byte store */
                *reinterpret_cast<short4u *>(orow + sj[0]) = pk;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (sj[j] >= 0)
                        orow[sj[j]] = v[j];
            }
        }
    }
}

/* Batch of frames with an active senone list per frame (ssw_align_batch_active): the
 * compallsen = no half of ptm_mgau_frame_eval (src/ptm_mgau.c:264-403), and of
 * ms_cont_mgau_frame_eval (src/ms_mgau.c:322-365), for every frame of a batch.  Frames are
 * grouped in segments that share their list (the second pass of forced alignment only ever grows
 * its set, src/state_align_search.c:186-189).  Per frame, PTM: the per-stream normaliser runs
 * over the active codebooks only (:353-364), the listed senones (bridge entries of
 * acmod_flags2list included) are combined and the best of them is subtracted from ALL n_sen
 * entries, the unlisted ones starting from 0 (:333, :392-400).  ms: only the listed senones are
 * evaluated (senone_eval, src/ms_senone.c:314-362: logmath_add over fden - pdf, negated, / aw,
 * clamped) and written, best of them subtracted with the second clamp; an entry never listed
 * reads 0 (a fresh acmod->senone_scores).
 *
 * Round 4's form (a [n_sen] row per frame assembled in LDS, one workgroup per frame, a binary
 * search per senone of the row to tell listed from unlisted entries, every segment's whole list
 * written out by the host) took 10.6 ms for 256 utterances x 1000 frames against 5.4 ms for the
 * compallsen = yes pipeline that evaluates 11 x the senones, 21.7 ms with word-like windows
 * (profiles/r05_a_align_active.json); its kernels are gone.  Round 5:
 *   - the search's set only grows (src/state_align_search.c:186-189 never clears acmod's bits),
 *     so frame t's REAL senones are a PREFIX of the utterance's senones ordered by the frame
 *     they are first listed in: one list per utterance, one prefix length per segment.  Only
 *     the bridge entries of acmod_flags2list's delta list (a gap above 255 between listed
 *     neighbours lists extra senones, src/acmod.c:966-975) depend on the whole set: a short
 *     list of their own per segment (a few entries);
 *   - a list entry carries its mixture-weight slot and codebook: no look-up before the gathers;
 *   - the scores go to COMPACT rows (ssw_k6_compact.inc): the utterance's own states only, at
 *     the position the alignment kernel reads; a [n_sen] row as acmod's buffer would hold it
 *     (listed: score - best; unlisted: PTM 0 - best, src/ptm_mgau.c:333, :392-400; ms 0) is
 *     written only when the caller asks for it (parity tests), with the listed entries marked
 *     through an LDS row instead of a search. */
struct SenoneActive2Params {
    const uint32_t *topn_cw;
    const int4 *topn_sc;
    const uint8_t *mixw, *logadd8;
    const int32_t *seg_of_frame; /* [n_frames] */
    const int32_t *seg_utt;      /* [n_seg] */
    const int32_t *seg_nreal;    /* [n_seg] prefix of the utterance's real list */
    const int32_t *seg_boff;     /* [n_seg + 1] into bridge_ent */
    const unsigned long long *seg_cbmask;
    const int32_t *utt_real_off; /* [n_utts + 1] into real_ent / real_rank */
    /* the utterance's real senones, slot | codebook << 16, SORTED BY SLOT (neighbouring lanes
     * then gather from neighbouring bytes of a mixture-weight row: a dozen 64-byte sectors per
     * wave-load instead of 64), and for each its rank in the order of first listing: frame t
     * lists the entries with rank < seg_nreal */
    const uint32_t *real_ent;
    const uint16_t *real_rank;
    const uint32_t *bridge_ent;
    /* compact output: the plan's tables (ssw_compact_plan_s) */
    const uint32_t *cpos;
    const long long *crow_off;
    const int32_t *cstride, *cutt_off;
    int16_t *out_c;
    /* optional [n_frames][n_sen] rows as acmod's buffer would hold them */
    int16_t *out_full;
    const int16_t *slot_sen; /* [slot_stride] senone of every slot, -1 = padding */
    int n_frames, n_cb, n_feat, n_density, n_sen, slot_stride;
    int zero, aw; /* ms scorer: logmath zero at shift 10, acoustic weight divisor */
    int cap;      /* entries the LDS score array holds (the longest list of the batch) */
    int frame_base; /* batch frame number of this launch's first frame (a piece of a batch:
                     * topn_* start at it, every other table is indexed by batch frames) */
};

/* One WAVE per frame, four frames per workgroup: the frame's work is a few hundred entries of
 * twelve gathers each, and in the first form (a 256-thread workgroup per frame: five barriers,
 * LDS atomics for the three normalisers, two entries per thread) most of a frame's 11 ns went
 * into waiting at them.  Here a lane takes every 64th entry (seven or eight of them, their
 * gathers in flight together), the normalisers and the best score are wave reductions, and the
 * only workgroup barrier is the one behind the log-add table's fill. */
template <bool MS>
__global__ void __launch_bounds__(256)
senone_active2_kernel(SenoneActive2Params P)
{
    __shared__ uint8_t s_tab[SSW_LOGADD_LDS];
    extern __shared__ __align__(16) unsigned char smem[];
    const int n_cbf = P.n_cb * P.n_feat;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    /* per wave: PTM normalised scores and codewords of every (codebook, stream), 4 x 8 bits
     * each | raw scores of the listed entries | the [n_sen] row (out_full only) */
    const Active2Carve carve(MS, n_cbf, P.cap, P.n_sen, P.out_full != nullptr);
    unsigned char *mine = smem + carve.wave(w);
    uint32_t *s_ns4 = reinterpret_cast<uint32_t *>(mine + carve.ns4());
    uint32_t *s_cw4 = reinterpret_cast<uint32_t *>(mine + carve.cw4());
    int16_t *s_a = reinterpret_cast<int16_t *>(mine + carve.a());
    int16_t *s_row = reinterpret_cast<int16_t *>(mine + carve.row());
    logadd_table_to_lds(s_tab, P.logadd8, tid, 256);
    __syncthreads();
    const int t = P.frame_base + (int)blockIdx.x * 4 + w;
    if (t >= P.frame_base + P.n_frames)
        return;
    const int seg = __builtin_amdgcn_readfirstlane(P.seg_of_frame[t]);
    const int u = __builtin_amdgcn_readfirstlane(P.seg_utt[seg]);
    const int n_real = __builtin_amdgcn_readfirstlane(P.seg_nreal[seg]);
    const int b0 = __builtin_amdgcn_readfirstlane(P.seg_boff[seg]);
    const int r0 = __builtin_amdgcn_readfirstlane(P.utt_real_off[u]);
    const int n_master = __builtin_amdgcn_readfirstlane(P.utt_real_off[u + 1]) - r0;
    const int n_ent = n_master + __builtin_amdgcn_readfirstlane(P.seg_boff[seg + 1]) - b0;
    const uint32_t *real = P.real_ent + r0;
    const uint16_t *rank = P.real_rank + r0;
    const uint32_t *cw = P.topn_cw + (size_t)(t - P.frame_base) * n_cbf;
    const int4 *sc = P.topn_sc + (size_t)(t - P.frame_base) * n_cbf;
    if (!MS) {
        wave_codebook_norm(sc, cw, n_cbf, P.n_feat, P.seg_cbmask[seg], lane, s_ns4, s_cw4);
        wave_sync();
    }
    int best = INT_MAX;
    for (int i = lane; i < n_ent; i += 64) {
        const bool is_b = i >= n_master;
        if (!is_b && (int)rank[i] >= n_real)
            continue; /* not listed yet */
        const uint32_t ent = is_b ? P.bridge_ent[b0 + i - n_master] : real[i];
        const int sl = (int)(ent & 0xffffu), cb = (int)(ent >> 16);
        const int a = MS
            ? ms_slot_score(P.mixw + sl, P.n_feat, P.n_density, P.slot_stride, cw + cb * P.n_feat,
                            sc + cb * P.n_feat, P.zero, P.aw, s_tab)
            : ptm_slot_score(P.mixw + sl, P.n_feat, P.n_density, P.slot_stride,
                             s_cw4 + cb * P.n_feat, s_ns4 + cb * P.n_feat, s_tab);
        s_a[i] = (int16_t)a;
        best = a < best ? a : best;
    }
    best = wave_best_or_zero(best); /* 0: callers always list the alignment's first phone */
    wave_sync();
    /* compact row: the real entries that are states of this utterance */
    int16_t *crow = P.out_c + P.crow_off[u] + (long long)(t - P.cutt_off[u]) * P.cstride[u];
    const uint32_t *cpos = P.cpos + (size_t)u * P.slot_stride;
    for (int i = lane; i < n_master; i += 64) {
        if ((int)rank[i] >= n_real)
            continue;
        const uint32_t cp = cpos[real[i] & 0xffffu];
        if (cp != 0xffffffffu)
            crow[cp >> 1] = final_score<MS>((int)s_a[i], best);
    }
    if (P.out_full != nullptr) {
        for (int sen = lane; sen < P.n_sen; sen += 64)
            s_row[sen] = MS ? (int16_t)0 : (int16_t)(0 - best);
        wave_sync();
        for (int i = lane; i < n_ent; i += 64) {
            const bool is_b = i >= n_master;
            if (!is_b && (int)rank[i] >= n_real)
                continue;
            const uint32_t ent = is_b ? P.bridge_ent[b0 + i - n_master] : real[i];
            s_row[P.slot_sen[ent & 0xffffu]] = final_score<MS>((int)s_a[i], best);
        }
        wave_sync();
        int16_t *orow = P.out_full + (size_t)t * P.n_sen;
        for (int sen = lane; sen < P.n_sen; sen += 64)
            orow[sen] = s_row[sen];
    }
}
