/* ssw_k1a_frames.inc -- K1a: history-free speculative top-N, one lane per frame, with the exact in-wave pass behind it (PTM and ms).
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* K1a fast path: history-free top-N, one lane per frame                                 */
/* ---------------------------------------------------------------------------------- */
/*
 * The reference's top-N list depends on the previous frame only through tie order and
 * boundary membership among EQUAL truncated scores (SURVEY.md A.2).  If the four best
 * densities of a frame truncate to four distinct ints, all greater than the int of every other
 * density, the reference's list is exactly "the four best, best first" whatever it carried in
 * (proof in DESIGN.md).  So every (frame, chain) pair is first evaluated independently:
 *
 *   - a wave owns one (codebook, stream) and 64*FPL frames, FPL frames per lane; the 128
 *     densities stream through SGPRs (wave-uniform scalar loads), the lane's x and x*x stay in
 *     VGPRs, packed over its FPL frames;
 *   - the scan does not compute the reference's value but a key that provably bounds it from
 *     above: the density as a quadratic form in x, 26 fused multiply-adds, with the worst-case
 *     distance to the reference's fp32 value folded into the constant term (host side, see
 *     upload_model) -- half the arithmetic of the reference's sub, mul, mul, sub;
 *   - a running top-5 is kept as 5 floats per frame whose low 7 mantissa bits carry the
 *     codeword (v_and_or + 4 x v_med3 + v_max): 6 VALU ops per density, no cross-lane traffic;
 *   - the 4 best codewords are then recomputed exactly, in the reference's operation order
 *     (records gathered from an LDS copy of the codebook), and sorted; the 5th key bounds every
 *     other density.  When "4 distinct ints > bound" cannot be shown the wave redoes the pair
 *     itself, exactly, before anything is stored (the exact in-wave pass below): the codebook's exact
 *     records are already in LDS, the predecessor frame's final order sits in the neighbouring
 *     lane, and for the tile's first frame the wave re-derives it from the features alone.  No
 *     second kernel, no work list, nothing handed from one wave to another.
 */
__device__ __forceinline__ float
med3f(float a, float b, float c)
{
    return __builtin_amdgcn_fmed3f(a, b, c);
}

#define SSW_REC_LDS_STRIDE 36 /* dwords per exact record in LDS (32 + 4 of padding) */

template <int VECLEN, int FPL, bool MS, bool MASKED = false>
__global__ void __launch_bounds__(256, (FPL == 2 && !MS) ? 4 : 3)
ptm_topn_frames_kernel(const float *__restrict__ rec, const float *__restrict__ recq,
                       const float *__restrict__ recmax, const uint32_t *__restrict__ exlist,
                       const float *__restrict__ feats, FramesParams P)
{
    static_assert(FPL == 1 || FPL == 2, "one or two frames per lane");
    const int lane = threadIdx.x & 63;
    /* Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one).  The (codebook,
     * stream) x tile-group pairs are cut into 8 contiguous chunks, one per XCD, so that the
     * workgroups that stream the same 16 KB of records sit behind the same L2. */
    const int n_pairs = P.n_cbf * P.tile_groups;
    const int chunk = (n_pairs + 7) >> 3;
    const int pair = (int)(blockIdx.x & 7u) * chunk + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= chunk || pair >= n_pairs)
        return;
    const int cbf = pair / P.tile_groups;
    /* (the wave's number declared uniform: frame numbers derived from it stay in SGPRs) */
    const int tile = (pair - cbf * P.tile_groups) * 4
        + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t_base = tile * 64 * FPL;
    /* The workgroup's four waves share the codebook: its 128 exact records (the epilogue
     * re-evaluates 4 of them per frame) are staged in LDS once, rows padded to 36 dwords so that
     * the per-lane row gathers spread over the banks.  From L1 those gathers ran at 64 B/clk
     * per CU and were the epilogue's whole cost. */
    __shared__ float4 s_rec[128 * (SSW_REC_LDS_STRIDE / 4)]; /* typed float4: 16-byte LDS reads */
    const int f = cbf % P.n_feat;
    const float *rec_cbf = rec + (size_t)cbf * 128 * SSW_REC_FLOATS;
    const float *rq_cbf = recq + (size_t)cbf * 128 * SSW_REC_FLOATS;
    /* Everything the prologue needs from memory is requested before anything is waited for: the
     * record block for LDS, the lane's feature rows, the codebook's reference level, and one
     * touch of every 128-byte line of the scan records (so that the scalar loads of the scan
     * find them in L2).  Issued one after the other with the barrier in between, these were
     * three dependent round trips at the moment all 4,032 waves of a step start together. */
    float4 stage[4];
    {
        const float4 *src = reinterpret_cast<const float4 *>(rec_cbf);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            stage[i] = src[i * 256 + (int)threadIdx.x];
    }
    const float d0 = recmax[(size_t)cbf * SSW_REC_FLOATS]; /* the keys are relative to this */
    float touch = rq_cbf[lane * SSW_REC_FLOATS] + rq_cbf[(64 + lane) * SSW_REC_FLOATS];
    int tt[FPL];
    float x[FPL][VECLEN];
    float2v xv[VECLEN], xq[VECLEN]; /* x and x*x of the lane's frames, packed per dimension */
#pragma unroll
    for (int h = 0; h < FPL; ++h) {
        tt[h] = t_base + h * 64 + lane;
        int tl = tt[h] < P.n_frames ? tt[h] : P.n_frames - 1;
        tl = tl < 0 ? 0 : tl;
        const float *xp = feats + (size_t)tl * P.featdim + P.featoff[f];
        /* every lane reads its own row: 16-byte loads (rows are only 4-byte aligned, which
         * global loads allow) cut the number of line look-ups per wave by three */
#pragma unroll
        for (int j = 0; j + 4 <= VECLEN; j += 4) {
            float4u v = *reinterpret_cast<const float4u *>(xp + j);
            x[h][j] = v.x;
            x[h][j + 1] = v.y;
            x[h][j + 2] = v.z;
            x[h][j + 3] = v.w;
        }
#pragma unroll
        for (int j = VECLEN & ~3; j < VECLEN; ++j)
            x[h][j] = xp[j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = i * 256 + (int)threadIdx.x; /* float4 index in the 128 x 32 table */
        s_rec[(e >> 3) * (SSW_REC_LDS_STRIDE / 4) + (e & 7)] = stage[i];
    }
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
#pragma unroll
    for (int j = 0; j < VECLEN; ++j) {
        xv[j].x = x[0][j];
        xv[j].y = x[FPL - 1][j];
        xq[j] = xv[j] * xv[j];
    }

    const float NEG_INF = -__builtin_huge_valf();
    float L[FPL][5];
#pragma unroll
    for (int h = 0; h < FPL; ++h)
#pragma unroll
        for (int k = 0; k < 5; ++k)
            L[h][k] = NEG_INF;

    /* The 128 records stream through SGPRs, double-buffered by hand: the loads of record
     * cw+1 are issued before the arithmetic on record cw and waited for after it.  They are
     * inline asm because SMEM returns out of order (only lgkmcnt(0) is meaningful) and the
     * compiler would otherwise issue and wait in one place; the operand ties keep issue, use
     * and wait in this order, and keep every register of a tuple reserved while its load is
     * in flight. */
    uint32_t keymask;
    asm volatile("v_mov_b32 %0, 0xffffff80" : "=v"(keymask));
    v16f a_lo, a_hi, b_lo, b_hi;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40"
                 : "=&s"(a_lo), "=&s"(a_hi)
                 : "s"(rq_cbf));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a_lo), "+s"(a_hi));

#define SSW_REC_ISSUE(lo, hi, ptr, tie)                                                      \
    asm volatile("s_load_dwordx16 %0, %3, 0x0\n\ts_load_dwordx16 %1, %3, 0x40"              \
                 : "=&s"(lo), "=&s"(hi), "+s"(tie)                                           \
                 : "s"(ptr))
#define SSW_REC_WAIT(lo, hi, vtie) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(lo), "+s"(hi), "+v"(vtie))
#define SSW_KEY_INSERT(d, cwv)                                                               \
    _Pragma("unroll") for (int h = 0; h < FPL; ++h)                                          \
    {                                                                                        \
        float key = __uint_as_float((__float_as_uint(d[h]) & keymask) | (uint32_t)(cwv));    \
        L[h][4] = med3f(L[h][3], L[h][4], key);                                              \
        L[h][3] = med3f(L[h][2], L[h][3], key);                                              \
        L[h][2] = med3f(L[h][1], L[h][2], key);                                              \
        L[h][1] = med3f(L[h][0], L[h][1], key);                                              \
        asm("v_max_f32 %0, %1, %2" : "=v"(L[h][0]) : "v"(L[h][0]), "v"(key));               \
    }
#define SSW_REC_SCAN(lo, hi, cwv)                                                            \
    {                                                                                        \
        float d[FPL];                                                                        \
        if (FPL == 2) {                                                                      \
            float2v dd = { lo[SSW_REC_DET], lo[SSW_REC_DET] };                               \
            _Pragma("unroll") for (int j = 0; j < VECLEN; ++j)                               \
            {                                                                                \
                float2v aa = { lo[j], lo[j] };                                               \
                float2v bb = { hi[j], hi[j] };                                               \
                dd = __builtin_elementwise_fma(aa, xv[j], dd);                               \
                dd = __builtin_elementwise_fma(bb, xq[j], dd);                               \
            }                                                                                \
            d[0] = dd.x;                                                                     \
            d[FPL - 1] = dd.y;                                                               \
        } else {                                                                             \
            float dd = lo[SSW_REC_DET];                                                      \
            _Pragma("unroll") for (int j = 0; j < VECLEN; ++j)                               \
            {                                                                                \
                dd = __builtin_fmaf(lo[j], xv[j].x, dd);                                     \
                dd = __builtin_fmaf(hi[j], xq[j].x, dd);                                     \
            }                                                                                \
            d[0] = dd;                                                                       \
        }                                                                                    \
        SSW_KEY_INSERT(d, cwv)                                                               \
    }

    static_assert(SSW_REC_VAR == 16 && SSW_REC_FLOATS == 32, "record = two 16-dword halves");
    SSW_TL(1)
    for (int cw = 0; cw < 128; cw += 2) {
        const float *rb = rq_cbf + (cw + 1) * SSW_REC_FLOATS;
        SSW_REC_ISSUE(b_lo, b_hi, rb, a_lo);
        SSW_REC_SCAN(a_lo, a_hi, cw);
        SSW_REC_WAIT(b_lo, b_hi, L[FPL - 1][0]);
        const float *ra = rq_cbf + (cw + 2 < 128 ? cw + 2 : 127) * SSW_REC_FLOATS;
        SSW_REC_ISSUE(a_lo, a_hi, ra, b_lo);
        SSW_REC_SCAN(b_lo, b_hi, cw + 1);
        SSW_REC_WAIT(a_lo, a_hi, L[FPL - 1][0]);
    }
#undef SSW_REC_SCAN
    /* The few ill-conditioned densities of this codebook (their scan records are inert: key
     * -3e38) are evaluated the reference's way, from the EXACT records, which stream through the
     * same SGPR double buffer (two codebook x streams of en-us hold 52 and 43 of them: fetched
     * one by one with a dependent load each, their waves ended 40 K cycles after all others and
     * the kernel with them).  Their keys need no bias. */
    {
        const uint32_t *xl = exlist + (size_t)cbf * SSW_EXLIST_STRIDE;
        const int n_ex = __builtin_amdgcn_readfirstlane((int)xl[0]);
#define SSW_REC_EXACT(lo, hi, cwv)                                                           \
    {                                                                                        \
        float2v dd = { lo[SSW_REC_DET], lo[SSW_REC_DET] };                                   \
        _Pragma("unroll") for (int j = 0; j < VECLEN; ++j)                                   \
        {                                                                                    \
            float2v mm = { lo[j], lo[j] };                                                   \
            float2v vv = { hi[j], hi[j] };                                                   \
            float2v diff = xv[j] - mm;                                                       \
            float2v sq = diff * diff;                                                        \
            float2v c = sq * vv;                                                             \
            dd = dd - c;                                                                     \
        }                                                                                    \
        float d[FPL];                                                                        \
        d[0] = dd.x - d0;                                                                    \
        d[FPL - 1] = dd.y - d0;                                                              \
        SSW_KEY_INSERT(d, cwv)                                                               \
    }
        if (n_ex > 0) {
            /* buffers of their own: tying the main loop's tuples into a second loop makes the
             * compiler want a VGPR copy of them ("illegal VGPR to SGPR copy") */
            v16f c_lo, c_hi, e_lo, e_hi;
            /* readfirstlane: the list entries are wave-uniform, which the "s" operands of the
             * loads need the compiler to know */
            int cwa = __builtin_amdgcn_readfirstlane((int)xl[1]), cwb = 0;
            const float *ra = rec_cbf + cwa * SSW_REC_FLOATS;
            asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40"
                         : "=&s"(c_lo), "=&s"(c_hi)
                         : "s"(ra));
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(c_lo), "+s"(c_hi));
            for (int i = 0; i < n_ex; i += 2) {
                cwb = __builtin_amdgcn_readfirstlane((int)xl[1 + (i + 1 < n_ex ? i + 1 : i)]);
                const float *rb = rec_cbf + cwb * SSW_REC_FLOATS;
                SSW_REC_ISSUE(e_lo, e_hi, rb, c_lo);
                SSW_REC_EXACT(c_lo, c_hi, cwa);
                SSW_REC_WAIT(e_lo, e_hi, L[FPL - 1][0]);
                cwa = __builtin_amdgcn_readfirstlane((int)xl[1 + (i + 2 < n_ex ? i + 2 : i)]);
                ra = rec_cbf + cwa * SSW_REC_FLOATS;
                SSW_REC_ISSUE(c_lo, c_hi, ra, e_lo);
                if (i + 1 < n_ex)
                    SSW_REC_EXACT(e_lo, e_hi, cwb);
                SSW_REC_WAIT(c_lo, c_hi, L[FPL - 1][0]);
            }
        }
#undef SSW_REC_EXACT
    }
#undef SSW_REC_ISSUE
#undef SSW_REC_WAIT
#undef SSW_KEY_INSERT
    SSW_TL(2)
    asm volatile("" ::"v"(touch));

    /* results of the lane's frames: codewords packed 4 x 8 bits (best first), raw scores;
     * need[h] = lanes whose pair could not be proven (wave-uniform masks) */
    uint32_t cpk[FPL];
    int s[FPL][4];
    unsigned long long need[FPL];
#pragma unroll
    for (int h = 0; h < FPL; ++h) {
        float dv[4];
        int c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] = (int)(__float_as_uint(L[h][k]) & 127u);
            const float4 *rp = &s_rec[c[k] * (SSW_REC_LDS_STRIDE / 4)];
            float buf[SSW_REC_FLOATS];
            float4v rv[SSW_REC_FLOATS / 4];
#pragma unroll
            for (int q = 0; q < SSW_REC_FLOATS / 4; ++q)
                rv[q] = reinterpret_cast<const float4v *>(rp)[q];
            /* keep the whole 16-byte reads: left alone the compiler narrows these to the 27
             * floats it needs, as 8-byte ds_read2_b32 at half the LDS rate.  One statement for
             * the eight of them: they are in flight together, not waited for one by one */
            asm volatile("" : "+v"(rv[0]), "+v"(rv[1]), "+v"(rv[2]), "+v"(rv[3]), "+v"(rv[4]),
                              "+v"(rv[5]), "+v"(rv[6]), "+v"(rv[7]));
#pragma unroll
            for (int q = 0; q < SSW_REC_FLOATS / 4; ++q) {
                buf[q * 4 + 0] = rv[q].x;
                buf[q * 4 + 1] = rv[q].y;
                buf[q * 4 + 2] = rv[q].z;
                buf[q * 4 + 3] = rv[q].w;
            }
            float dd = buf[SSW_REC_DET];
#pragma unroll
            for (int j = 0; j < VECLEN; ++j) {
                float diff = x[h][j] - buf[j];
                float sq = diff * diff;
                float cc = sq * buf[SSW_REC_VAR + j];
                dd = dd - cc;
            }
            dv[k] = dd;
            /* PTM keeps the truncated density (src/ptm_mgau.c:128-131); the ms scorer keeps the
             * float and later uses ((int32)dist + 1023) >> 10 (src/ms_senone.c:332-335) */
            s[h][k] = MS ? ms_fden(dd) : dens2int(dd);
        }
        /* sorted best first, then the proof: four distinct values above the bound the 5th key
         * puts on every other density (ssw_scan_common.inc) */
        if (MS) {
            /* The ms instances keep the five exchanges as the text they were: through
             * sort4_best_first (as a lambda, a function per exchange, or a lambda written here)
             * their code changes, and SSW_SCAN=fma tools/bench_ms.py lost 0.7 % against the
             * parent's span (profiles/scan_common_ab.json).  Same network, same rule. */
#define CSWAP(a, b)                                                                          \
    {                                                                                        \
        bool sw = dv[b] > dv[a];                                                             \
        int ts = sw ? s[h][b] : s[h][a], tc = sw ? c[b] : c[a];                              \
        float td = sw ? dv[b] : dv[a];                                                       \
        s[h][b] = sw ? s[h][a] : s[h][b];                                                    \
        c[b] = sw ? c[a] : c[b];                                                             \
        dv[b] = sw ? dv[a] : dv[b];                                                          \
        s[h][a] = ts;                                                                        \
        c[a] = tc;                                                                           \
        dv[a] = td;                                                                          \
    }
            CSWAP(0, 1) CSWAP(2, 3) CSWAP(0, 2) CSWAP(1, 3) CSWAP(1, 2)
#undef CSWAP
        } else {
            sort4_best_first<MS>(s[h], c, dv);
        }
        const ScanBound ub = scan_upper_bound(L[h][4], ScanKeysFma{}, d0);
        const bool proven = scan_proven<MS>(s[h], dv, ub);
        cpk[h] = order_pack(c);
        need[h] = __ballot(!proven && tt[h] < P.n_frames);
    }
    /* Exact in-wave pass.  A pair that could not be proven is redone here by the whole wave, in
     * frame order, with the reference's state machine (topn_exact_step = eval_topn + eval_cb,
     * src/ptm_mgau.c:86-225): 128 exact densities, two per lane, from the LDS records; carried
     * order = the previous frame's FINAL order -- the neighbouring lane's registers (proven, or
     * redone a moment ago), the reset history at an utterance's first frame, or, for the tile's
     * first frame, what carried_order_of re-derives.  Rare (0.07 % of the pairs of a bench step),
     * so the branch is wave-uniform and almost never taken. */
    if (P.seg_of_frame != nullptr) { /* pairs of unscanned codebooks are nobody's input */
#pragma unroll
        for (int h = 0; h < FPL; ++h)
            need[h] &= scan_mask_unscanned(P, cbf, tt[h]);
    }
    if ((need[0] | need[FPL - 1]) != 0ull) {
        const float *srow0 = reinterpret_cast<const float *>(s_rec) + lane * SSW_REC_LDS_STRIDE;
        const float *srow1 = srow0 + 64 * SSW_REC_LDS_STRIDE;
        unsigned n_done = 0;
#pragma unroll
        for (int h = 0; h < FPL; ++h) {
            unsigned long long todo = need[h];
            while (todo != 0ull) {
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int t = t_base + h * 64 + l;
                float dvx[2];
                int ivx[2];
                wave_frame_densities<VECLEN, false, !MS>(feats, P.featdim, P.featoff[f], t, srow0, srow1, 0,
                                             dvx, ivx);
                int Lc[4], Ls[4];
                if (MS) {
                    float Ld[4];
                    ms_exact_step(dvx, Lc, Ld);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        Ls[k] = ms_fden(Ld[k]);
                } else if (!topn_self_determined(ivx, lane, Lc, Ls)) {
                    /* (only real ties need the state machine: see ssw_k1a_mfma.inc) */
                    if (bit_test_u(P.utt_start, t)) {
                        start_order(P, cbf, t, Lc);
                    } else if ((h == 0 && l == 0) || !cb_scanned_u(P, cbf / P.n_feat, t - 1)
                               || chain_skipped(P, t - 1)) {
                        /* the tile's first frame, or a frame whose predecessor did not scan this
                         * codebook (what this kernel stored for it is not the reference's state),
                         * or the first frame of an utterance in a chain whose predecessor had an
                         * odd number of frames */
                        carried_order_of<VECLEN, false, MASKED>(P, cbf, feats, P.featoff[f], t - 1, lane, srow0,
                                                 srow1, 0, Lc);
                    } else {
                        /* frame t - 1 is the neighbouring lane; for the second half's lane 0 it
                         * is lane 63 of the first half */
                        const uint32_t pk = l == 0
                            ? (uint32_t)__builtin_amdgcn_readlane((int)cpk[0], 63)
                            : (uint32_t)__builtin_amdgcn_readlane((int)cpk[h], l - 1);
                        order_unpack(pk, Lc);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        Ls[k] = INT_MIN;
                    /* the lane's 4th candidate is a real codeword of this frame: its score is a
                     * valid floor for the scan (topn_exact_step) */
                    /* (a valid floor needs four different candidates: strictly decreasing
                     * scores guarantee that; non-finite features can break it) */
                    const int fl = (s[h][0] > s[h][1] && s[h][1] > s[h][2] && s[h][2] > s[h][3])
                        ? s[h][3] : INT_MIN;
                    topn_exact_step<2, 4>(dvx, ivx, Lc, Ls, true,
                                          __builtin_amdgcn_readlane(fl, l));
                }
                if (lane == l) {
                    cpk[h] = order_pack(Lc);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        s[h][k] = Ls[k];
                }
                ++n_done;
            }
        }
        if (lane == 0)
            atomicAdd(P.n_fixed, (unsigned long long)n_done);
    }
#pragma unroll
    for (int h = 0; h < FPL; ++h) {
        if (tt[h] < P.n_frames) {
            size_t idx = (size_t)tt[h] * P.n_cbf + cbf;
            P.topn_cw[idx] = cpk[h];
            P.topn_sc[idx] = make_int4(s[h][0], s[h][1], s[h][2], s[h][3]);
        }
    }
    SSW_TL(3)
}


/* What the second pass of decoder_alignment starts from after acmod_rewind, per utterance,
 * [n_utts][n_cbf] (src/decoder.c:786-793).  The scorer keeps a ring of two history slots indexed
 * by frame % 2 (n_fast_hist = 2, src/ptm_mgau.c:425-437, :804); frame 0 of the second pass copies
 * slot 1, i.e. the final order of the first pass's last ODD-numbered frame: frame T - 1 of an
 * utterance of even length T, frame T - 2 of one of odd length; an utterance of one frame never
 * wrote slot 1, nor did one without frames: they keep `start` (what the first pass itself started
 * from -- the reset order here, NULL -- or a row per utterance). */
__global__ void __launch_bounds__(128)
gather_last_orders_kernel(const uint32_t *__restrict__ topn_cw, const int *__restrict__ utt_off,
                          int n_cbf, const uint32_t *__restrict__ start, uint32_t *__restrict__ rows)
{
    const int u = blockIdx.x, t0 = utt_off[u], t1 = utt_off[u + 1];
    const int n = t1 - t0;
    const int last_odd = t0 + ((n >> 1) << 1) - 1; /* T even: t1 - 1; T odd: t1 - 2 */
    for (int i = threadIdx.x; i < n_cbf; i += blockDim.x)
        rows[(size_t)u * n_cbf + i] = n >= 2 ? topn_cw[(size_t)last_odd * n_cbf + i]
            : start != nullptr                ? start[(size_t)u * n_cbf + i]
                                              : SSW_ORDER_RESET;
}
