/* ssw_scan_common.inc -- K1a: what the two speculative top-N scans (ssw_k1a_frames.inc on the
 * vector unit, ssw_k1a_mfma.inc on the matrix cores) share, each piece once: the launch
 * parameters, the packed codeword order, the sort of the four candidates, the 5th-key bound and
 * the proof test, and the exact in-wave pass with its helpers (a frame's 128 exact densities,
 * "is this frame's list fixed by its own densities", the order a frame starts from, the walk
 * that re-derives a carried order, masked batches, the ms scorer's step).
 * Part of the single translation unit ssw_kernels.hip (included there, behind ssw_k1a_chain.inc
 * -- topn_exact_step -- and before both scans). */
typedef float float2v __attribute__((ext_vector_type(2)));
typedef float float4u __attribute__((ext_vector_type(4), aligned(4))); /* 4-byte aligned float4 */
typedef short short4u __attribute__((ext_vector_type(4), aligned(2))); /* 2-byte aligned 4 x int16 */
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float float4v __attribute__((ext_vector_type(4)));

struct FramesParams {
    uint32_t *topn_cw;
    int4 *topn_sc;
    const uint32_t *utt_start;   /* bit per frame: first frame of an utterance */
    const uint32_t *carry0;      /* optional [n_cbf]: packed codeword order the batch's FIRST frame
                                  * starts from (the state an earlier call left); NULL = the
                                  * reset history like every other utterance start */
    /* optional [n_utts][n_cbf]: the order EVERY utterance starts from (the second pass of
     * ssw_align_text_batch with two_pass_history: what the utterance's own first pass left);
     * utt_off [n_utts + 1] finds the utterance of a frame */
    const uint32_t *carry_rows;
    const int *utt_off;
    int n_utts;
    /* SSW_SCORE_CARRY_UTTS (one chain over several utterances): bit per frame "this frame's final
     * order is NOT what its successor starts from".  The reference keeps a ring of two history
     * slots indexed by frame % 2 and frame numbers restart at 0 with every utterance
     * (src/ptm_mgau.c:425-437, src/acmod.c:367): frame 0 of the next utterance copies slot 1, the
     * last ODD-numbered frame -- so the last frame of an utterance of odd length is left out of
     * the chain (a one-frame utterance entirely).  NULL = no such frames. */
    const uint32_t *chain_skip;
    unsigned long long *n_fixed; /* running count of pairs that took the exact in-wave pass */
    /* compallsen = no (ssw_align_batch_active): the codebooks acmod's active senone list makes
     * active, frame by frame -- segment of every frame and one bit per codebook and segment
     * (ptm_mgau_calc_cb_active, src/ptm_mgau.c:297-321).  NULL = every codebook, every frame.
     * An inactive codebook is not scanned by the reference, only its carried codewords are
     * re-scored (src/ptm_mgau.c:245-251): its top-N block is not used downstream, but its
     * history is what the next active frame starts from. */
    const int32_t *seg_of_frame;
    const unsigned long long *seg_cbmask;
    int n_frames, n_cbf, n_feat, featdim, tile_groups;
    int featoff[SSW_MAX_FEAT];
    /* matrix-core scan: the launch covers frames [frame_lo, n_frames) (a piece of a large batch,
     * ssw_host_score.inc); every array stays indexed by the batch's frame numbers, and the exact
     * pass may look at frames before frame_lo */
    int frame_lo;
    /* matrix-core scan: the (codebook x stream, tile group) pairs each XCD takes, [xcd_lo[x],
     * xcd_lo[x + 1]): contiguous chunks cut by COST (a density left to the exact form costs its
     * codebook's waves ~45 vector instructions per frame: en-us's first codebook x stream has
     * 28 of them and its waves live twice as long), not by count */
    int xcd_lo[9];
    /* SSW_SCAN_AUDIT=k (AUDIT instances of the matrix-core scan): every k-th wave redoes all of
     * its frames exactly; n_fixed[2] counts the proven pairs so audited, n_fixed[3] those whose
     * exact result differs from the scan's */
    int audit_k;
};

/* The packed order: a frame's four codewords, best first, 8 bits each in a uint32_t (topn_cw, the
 * carry rows).  SSW_ORDER_RESET is the reset history of src/ptm_mgau.c:706-713 (cw = m), the
 * same literal on the device and on the host. */
#define SSW_ORDER_RESET 0x03020100u

__device__ __forceinline__ uint32_t
order_pack(const int (&c)[4])
{
    return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
}

__device__ __forceinline__ void
order_unpack(uint32_t pk, int (&Lc)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k)
        Lc[k] = (int)((pk >> (8 * k)) & 0xffu);
}

#if defined(SSW_TIMELINE) || defined(SSW_TIMELINE_SEN)
__device__ unsigned long long g_timeline[16384 * 6];
#endif
#ifdef SSW_TIMELINE
__device__ unsigned long long g_timeline2[8192 * 8]; /* stamps inside the exact in-wave pass */
#define SSW_TL2(k)                                                                           \
    if (lane == 0) {                                                                         \
        int wv = blockIdx.x * 4 + (threadIdx.x >> 6);                                        \
        if (wv < 8192)                                                                       \
            g_timeline2[wv * 8 + (k)] = __builtin_amdgcn_s_memtime();                       \
    }
#define SSW_TL(k)                                                                            \
    if (lane == 0) {                                                                         \
        int wv = blockIdx.x * 4 + (threadIdx.x >> 6);                                        \
        if (wv < 8192)                                                                       \
            g_timeline[wv * 6 + (k)] = __builtin_amdgcn_s_memtime();                        \
    }
#else
#define SSW_TL(k)
#define SSW_TL2(k)
#endif


/* ---- exact in-wave pass: helpers ------------------------------------------------------ */

/* The exact densities of frame t for the wave's 128 codewords: lane l evaluates codewords l and
 * l + 64 from the workgroup's LDS copy of the codebook's exact records (srow0 / srow1 = the
 * lane's two rows), the feature row is wave-uniform.  Same operation order as everywhere:
 * sub, mul, mul, sub per dimension, each rounded (src/ptm_mgau.c:63-68). */
/* element k of an LDS record row whose 16-byte chunks are stored XOR-swizzled by `sw` (0 = plain) */
__device__ __forceinline__ float
rec_at(const float *row, int k, int sw)
{
    return row[((((k >> 2) ^ sw) << 2) | (k & 3))];
}

/* PACKED (round 4, the matrix-core scan's LDS copy): rows of SSW_REC28_FLOATS = 28 floats --
 * mean 0..12 | det 13 | scale 14..26 | 0 -- seven 16-byte chunks, no swizzle (a stride of 7 chunks
 * spreads the lanes' rows over the 8 bank groups by itself); srow0 / srow1 point at the lane's
 * rows in that layout and sw is ignored. */
#define SSW_REC28_FLOATS 28
/* NANFIX (round 5, PTM scorer): a NaN feature, the reference's way.  eval_cb walks the dimensions
 * in stages (VECLEN % 4 single ones, then groups of four) and leaves the walk when `d >= thresh`
 * fails at the head of a stage (src/ptm_mgau.c:182, :191, :206-211) -- which it does for a NaN d.
 * So a density whose d turns NaN before the LAST stage is "not in topn", while with a NaN only
 * in the last stage's dimensions every density whose partial sum at the head of that stage is
 * >= thresh passes the final `d < thresh` test too (false for a NaN) and is inserted with
 * (int32)NaN = INT32_MIN.  Encoded for topn_exact_step as: iv = INT_MIN, dv = NaN (never
 * admitted) or, NaN in the last stage only, dv = that partial sum (admitted iff dv >=
 * (float)worst; the list's scores are all INT_MIN in such a frame, the carried codewords having
 * been re-scored to (int32)NaN).  The feature row is wave-uniform, so is the (cold) branch. */
template <int VECLEN>
__device__ __forceinline__ int
nan_stage_of(const float *__restrict__ xp)
{
    constexpr int LATE0 = VECLEN >= 4 ? VECLEN - 4 : VECLEN - 1;
    bool early = false, late = false;
#pragma unroll
    for (int j = 0; j < VECLEN; ++j) {
        const float xj = xp[j];
        if (j < LATE0)
            early = early || xj != xj;
        else
            late = late || xj != xj;
    }
    return early ? 1 : late ? 2 : 0;
}

template <int VECLEN, bool PACKED = false, bool NANFIX = true>
__device__ __forceinline__ void
wave_frame_densities(const float *__restrict__ feats, int featdim, int foff, int t,
                     const float *srow0, const float *srow1, int sw, float (&dv)[2], int (&iv)[2])
{
    const float *xp = feats + (size_t)t * featdim + foff;
    /* the lane's two record rows, as 16-byte reads (conflict-free in both LDS layouts: padded
     * rows with sw = 0, unpadded rows with their chunks at chunk ^ sw) */
    constexpr int NF = PACKED ? SSW_REC28_FLOATS : SSW_REC_FLOATS;
    constexpr int DET = PACKED ? 13 : SSW_REC_DET, VAR = PACKED ? 14 : SSW_REC_VAR;
    float r0[NF], r1[NF];
#pragma unroll
    for (int q = 0; q < NF / 4; ++q) {
        const float4 a = reinterpret_cast<const float4 *>(srow0)[PACKED ? q : (q ^ sw)];
        const float4 b = reinterpret_cast<const float4 *>(srow1)[PACKED ? q : (q ^ sw)];
        r0[4 * q] = a.x, r0[4 * q + 1] = a.y, r0[4 * q + 2] = a.z, r0[4 * q + 3] = a.w;
        r1[4 * q] = b.x, r1[4 * q + 1] = b.y, r1[4 * q + 2] = b.z, r1[4 * q + 3] = b.w;
    }
    float d0 = r0[DET], d1 = r1[DET];
#pragma unroll
    for (int j = 0; j < VECLEN; ++j) {
        const float xj = xp[j];
        float diff = xj - r0[j];
        float sq = diff * diff;
        float cc = sq * r0[VAR + j];
        d0 = d0 - cc;
        diff = xj - r1[j];
        sq = diff * diff;
        cc = sq * r1[VAR + j];
        d1 = d1 - cc;
    }
    dv[0] = d0;
    dv[1] = d1;
    iv[0] = dens2int(d0);
    iv[1] = dens2int(d1);
    if (NANFIX && __ballot(d0 != d0) != 0ull) {
        if (__builtin_amdgcn_readfirstlane(nan_stage_of<VECLEN>(xp)) == 2) {
            constexpr int LATE0 = VECLEN >= 4 ? VECLEN - 4 : VECLEN - 1;
            d0 = r0[DET], d1 = r1[DET];
#pragma unroll
            for (int j = 0; j < LATE0; ++j) {
                const float xj = xp[j];
                float diff = xj - r0[j];
                float sq = diff * diff;
                float cc = sq * r0[VAR + j];
                d0 = d0 - cc;
                diff = xj - r1[j];
                sq = diff * diff;
                cc = sq * r1[VAR + j];
                d1 = d1 - cc;
            }
            dv[0] = d0;
            dv[1] = d1;
        }
    }
}

/* True when the frame's top-N list cannot depend on what was carried in: its four best
 * densities truncate to four distinct ints, each above the int of every other density (the
 * claim proved in DESIGN.md section 4).  Lc / Ls then hold that list, best first.  Exact test on
 * all 128 truncated values, used when a wave has to re-derive the order its tile starts from. */
__device__ __forceinline__ bool
topn_self_determined(const int (&iv)[2], int lane, int (&Lc)[4], int (&Ls)[4])
{
    int a0 = iv[0], a1 = iv[1];
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int m = wave_max_dpp(a0 > a1 ? a0 : a1);
        const unsigned long long b0 = __ballot(a0 == m), b1 = __ballot(a1 == m);
        if (r < 4) {
            ok = ok && (__popcll(b0) + __popcll(b1) == 1);
            const int cw = b0 != 0 ? __builtin_ctzll(b0) : 64 + __builtin_ctzll(b1);
            Lc[r] = cw;
            Ls[r] = m;
            if (lane == (cw & 63)) {
                a0 = cw < 64 ? INT_MIN : a0;
                a1 = cw < 64 ? a1 : INT_MIN;
            }
        } else {
            ok = ok && Ls[3] > m;
        }
    }
    return ok;
}

/* The codeword order an utterance's first frame t starts from: the reset history of
 * src/ptm_mgau.c:706-713 (cw = m), or, for the first frame of the batch, what the caller carried
 * in (ssw_score_batch_ex: the reference keeps its history across acmod_rewind and from one
 * utterance to the next, src/ptm_mgau.c:425-448, src/acmod.c:367). */
__device__ __forceinline__ void
start_order(const FramesParams &P, int cbf, int t, int (&Lc)[4])
{
    /* (t and cbf are wave-uniform: so is everything read here) */
    uint32_t pk = (t == 0 && P.carry0 != nullptr)
        ? (uint32_t)__builtin_amdgcn_readfirstlane((int)P.carry0[cbf]) : SSW_ORDER_RESET;
    if (P.carry_rows != nullptr) { /* t is the first frame of an utterance: which one */
        int lo = 0, hi = P.n_utts - 1;
        while (lo < hi) { /* the last u with utt_off[u] <= t and a frame of its own */
            const int mid = (lo + hi + 1) >> 1;
            if (__builtin_amdgcn_readfirstlane(P.utt_off[mid]) <= t)
                lo = mid;
            else
                hi = mid - 1;
        }
        pk = (uint32_t)__builtin_amdgcn_readfirstlane((int)P.carry_rows[(size_t)lo * P.n_cbf + cbf]);
    }
    order_unpack(pk, Lc);
}

/* The final codeword order of frame t_prev as the reference's frame-sequential state machine
 * leaves it, derived from the features alone: walk back to the nearest frame whose list is fixed
 * by its own densities (an utterance's first frame, which starts from the reset history of
 * src/ptm_mgau.c:706-713, or a self-determined frame), then forward again with the exact step.
 * Every wave that needs the order of a frame computes the same thing: the reference's. */
/* is codebook cb scanned in frame t (compallsen = no batches; always, otherwise) */
__device__ __forceinline__ bool
cb_scanned(const FramesParams &P, int cb, int t)
{
    if (P.seg_of_frame == nullptr)
        return true;
    return (P.seg_cbmask[P.seg_of_frame[t]] >> cb) & 1ull;
}

/* cb_scanned for a wave-uniform frame (see bit_test_u) */
__device__ __forceinline__ bool
cb_scanned_u(const FramesParams &P, int cb, int t)
{
    if (P.seg_of_frame == nullptr)
        return true;
    const int seg = __builtin_amdgcn_readfirstlane(P.seg_of_frame[t]);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(P.seg_cbmask + seg);
    return ((uint32_t)__builtin_amdgcn_readfirstlane((int)w[cb >> 5]) >> (cb & 31)) & 1u;
}

/* frame t (wave-uniform) is off the chain its successors follow (FramesParams::chain_skip) */
__device__ __forceinline__ bool
chain_skipped(const FramesParams &P, int t)
{
    return P.chain_skip != nullptr && bit_test_u(P.chain_skip, t);
}

/* Masked batches (a codebook mask per frame: compallsen = no), round 6.  In the first pass of
 * the default configuration a codebook is scanned in a few frames here and there, and the walk
 * below used to evaluate all 128 densities of EVERY frame between the frame in hand and the
 * last one that fixes the list by itself, twice (back, then forward again): a codebook that had
 * been out of the search for 300 frames cost 600 frame evaluations, and a scan launch took up
 * to 1.5 ms where the unmasked one takes 0.12.  But a frame in which the codebook is not scanned
 * only RE-ORDERS the four codewords it carries (eval_topn without eval_cb,
 * src/ptm_mgau.c:236-247: re-scored in carried order, each placed after equal scores -- a
 * stable sort), so (a) walking back, such a frame needs no densities at all: it can never be
 * the frame that fixes the list, and (b) replaying forward, a whole run of such frames leaves
 * the order its LAST frame's four scores dictate whenever those are four different ints; only
 * when two of them tie does the order before that frame matter, and the run is replayed frame
 * by frame as before.  The frames themselves are found 64 at a time (a ballot over the masks). */
__device__ __forceinline__ bool
cb_scanned_or_start_lane(const FramesParams &P, int cb, int t)
{
    const bool scan = (P.seg_cbmask[P.seg_of_frame[t]] >> cb) & 1ull;
    return scan || ((P.utt_start[t >> 5] >> (t & 31)) & 1u);
}

/* the last frame <= t in which the codebook is scanned or an utterance starts (-1: none) */
__device__ __forceinline__ int
last_anchor_at_or_before(const FramesParams &P, int cb, int t, int lane)
{
    for (int base = t; base >= 0; base -= 64) {
        const int tt = base - lane;
        const unsigned long long m = __ballot(tt >= 0 && cb_scanned_or_start_lane(P, cb, tt >= 0 ? tt : 0));
        if (m != 0ull)
            return base - __builtin_ctzll(m);
    }
    return -1;
}

/* the first frame in [t, hi] in which the codebook is scanned (hi + 1: none) */
__device__ __forceinline__ int
next_scanned_at_or_after(const FramesParams &P, int cb, int t, int hi, int lane)
{
    for (int base = t; base <= hi; base += 64) {
        const int tt = base + lane;
        const int tc = tt <= hi ? tt : hi;
        const unsigned long long m
            = __ballot(tt <= hi && ((P.seg_cbmask[P.seg_of_frame[tc]] >> cb) & 1ull) != 0ull);
        if (m != 0ull)
            return base + __builtin_ctzll(m);
    }
    return hi + 1;
}

template <int VECLEN, bool PACKED>
__device__ __forceinline__ void
carried_order_masked(const FramesParams &P, int cbf, const float *__restrict__ feats, int foff,
                     int t_prev, int lane, const float *srow0, const float *srow1, int sw,
                     int (&Lc)[4])
{
    int Ls[4];
    float dv[2];
    int iv[2];
    const int cb = cbf / P.n_feat;
    /* back: to the nearest frame whose list is fixed by its own densities -- a scanned frame
     * with four distinct winners -- or to an utterance's first frame */
    int tb = t_prev;
    for (;;) {
        tb = last_anchor_at_or_before(P, cb, tb, lane);
        if (tb < 0) { /* (frame 0 is a start: not reached) */
            start_order(P, cbf, 0, Lc);
            tb = -1;
            break;
        }
        wave_frame_densities<VECLEN, PACKED>(feats, P.featdim, foff, tb, srow0, srow1, sw, dv, iv);
        const bool scan = cb_scanned_u(P, cb, tb);
        if (bit_test_u(P.utt_start, tb)) {
            start_order(P, cbf, tb, Lc);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                Ls[k] = INT_MIN;
            topn_exact_step<2, 4>(dv, iv, Lc, Ls, scan);
            break;
        }
        if (topn_self_determined(iv, lane, Lc, Ls))
            break;
        --tb; /* (> 0 here: frame 0 is a start) */
    }
    /* forward again */
    int tf = tb + 1;
    while (tf <= t_prev) {
        const int ts = next_scanned_at_or_after(P, cb, tf, t_prev, lane);
        if (ts > tf) {
            /* frames [tf, ts): the codebook is not scanned, its four codewords stay and are
             * re-sorted frame after frame.  The run's last frame first: */
            const int tl = ts - 1;
            int Lc2[4], Ls2[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                Lc2[k] = Lc[k];
                Ls2[k] = INT_MIN;
            }
            wave_frame_densities<VECLEN, PACKED>(feats, P.featdim, foff, tl, srow0, srow1, sw, dv, iv);
            topn_exact_step<2, 4>(dv, iv, Lc2, Ls2, false);
            if (Ls2[0] > Ls2[1] && Ls2[1] > Ls2[2] && Ls2[2] > Ls2[3]) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    Lc[k] = Lc2[k];
            } else { /* a tie in the last frame: the order before it decides */
                for (int tq = tf; tq <= tl; ++tq) {
                    wave_frame_densities<VECLEN, PACKED>(feats, P.featdim, foff, tq, srow0, srow1,
                                                         sw, dv, iv);
                    topn_exact_step<2, 4>(dv, iv, Lc, Ls, false);
                }
            }
            tf = ts;
            continue;
        }
        wave_frame_densities<VECLEN, PACKED>(feats, P.featdim, foff, tf, srow0, srow1, sw, dv, iv);
        topn_exact_step<2, 4>(dv, iv, Lc, Ls, true);
        ++tf;
    }
}

/* MASKED: the kernel instances that masked batches are launched with (the others carry none of
 * the code above: compiled into every instance it cost the headline scan 3 of its 34 us --
 * registers and code size of a path it never takes) */
template <int VECLEN, bool PACKED = false, bool MASKED = false>
__device__ __forceinline__ void
carried_order_of(const FramesParams &P, int cbf, const float *__restrict__ feats, int foff, int t_prev,
                 int lane, const float *srow0, const float *srow1, int sw, int (&Lc)[4])
{
    if (MASKED && P.seg_of_frame != nullptr && P.chain_skip == nullptr) {
        carried_order_masked<VECLEN, PACKED>(P, cbf, feats, foff, t_prev, lane, srow0, srow1, sw, Lc);
        return;
    }
    int Ls[4];
    float dv[2];
    int iv[2];
    const int cb = cbf / P.n_feat;
    /* frames off the chain (chain_skip) are stepped over in both directions */
    while (t_prev >= 0 && chain_skipped(P, t_prev))
        --t_prev;
    if (t_prev < 0) { /* nothing but skipped frames before: what the batch started from */
        start_order(P, cbf, 0, Lc);
        return;
    }
    int tb = t_prev;
    for (;;) {
        wave_frame_densities<VECLEN, PACKED>(feats, P.featdim, foff, tb, srow0, srow1, sw, dv, iv);
        const bool scan = cb_scanned_u(P, cb, tb);
        if (bit_test_u(P.utt_start, tb)) {
            start_order(P, cbf, tb, Lc);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                Ls[k] = INT_MIN;
            topn_exact_step<2, 4>(dv, iv, Lc, Ls, scan);
            break;
        }
        /* a frame in which the codebook is not scanned only re-orders what it carried */
        if (scan && topn_self_determined(iv, lane, Lc, Ls))
            break;
        int tp = tb - 1; /* frame 0 is an utterance start: the walk ends there at the latest */
        while (tp >= 0 && chain_skipped(P, tp))
            --tp;
        if (tp < 0) { /* (a chain that begins with skipped frames only) */
            start_order(P, cbf, 0, Lc);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                Ls[k] = INT_MIN;
            topn_exact_step<2, 4>(dv, iv, Lc, Ls, scan);
            break;
        }
        tb = tp;
    }
    for (int tf = tb + 1; tf <= t_prev; ++tf) {
        if (chain_skipped(P, tf))
            continue;
        wave_frame_densities<VECLEN, PACKED>(feats, P.featdim, foff, tf, srow0, srow1, sw, dv, iv);
        topn_exact_step<2, 4>(dv, iv, Lc, Ls, cb_scanned_u(P, cb, tf));
    }
}

/* compute_dist (src/ms_gauden.c:384-432) on a wave that holds the frame's 128 float densities:
 * the list starts at dist = (float)INT32_MIN; codeword d is admitted when dval >= worst.dist
 * and placed at the first position i with dval >= dist[i].  History-free. */
__device__ __forceinline__ void
ms_exact_step(const float (&dvl)[2], int (&Lc)[4], float (&Ld)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        Ld[k] = -2147483648.0f;
        Lc[k] = 0;
    }
    unsigned long long rem[2] = { ~0ull, ~0ull };
    for (;;) {
        const float thr = Ld[3];
        int cw = -1;
#pragma unroll
        for (int h = 1; h >= 0; --h) {
            const unsigned long long m = __ballot(dvl[h] >= thr) & rem[h];
            if (m != 0)
                cw = h * 64 + __builtin_ctzll(m);
        }
        if (cw < 0)
            break;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h < (cw >> 6))
                rem[h] = 0;
            else if (h == (cw >> 6))
                rem[h] &= ~((2ull << (cw & 63)) - 1ull);
        }
        float dval = 0.0f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float tv = __builtin_bit_cast(
                float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dvl[h]), cw & 63));
            dval = ((cw >> 6) == h) ? tv : dval;
        }
        int pos = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            pos += (Ld[k] > dval) ? 1 : 0;
#pragma unroll
        for (int k = 3; k >= 1; --k)
            if (k > pos) {
                Ld[k] = Ld[k - 1];
                Lc[k] = Lc[k - 1];
            }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k == pos) {
                Ld[k] = dval;
                Lc[k] = cw;
            }
    }
}

/* ---- after the scan: sort, bound, proof ------------------------------------------------ */

/* The four candidates best first, by five compare-exchanges: PTM by truncated score (the list's
 * order, src/ptm_mgau.c:128-131), the ms scorer by the float itself (compute_dist).  Score,
 * codeword and float value move together. */
template <bool MS>
__device__ __forceinline__ void
sort4_best_first(int (&sk)[4], int (&c)[4], float (&dv)[4])
{
    auto cswap = [&](int a, int b) {
        bool sw = MS ? (dv[b] > dv[a]) : (sk[b] > sk[a]);
        int ts = sw ? sk[b] : sk[a], tc = sw ? c[b] : c[a];
        float td = sw ? dv[b] : dv[a];
        sk[b] = sw ? sk[a] : sk[b];
        c[b] = sw ? c[a] : c[b];
        dv[b] = sw ? dv[a] : dv[b];
        sk[a] = ts;
        c[a] = tc;
        dv[a] = td;
    };
    cswap(0, 1), cswap(2, 3), cswap(0, 2), cswap(1, 3), cswap(1, 2);
}

/* Upper bound on the true value of every density outside the four, from the 5th key.  Every key
 * of a scan is an upper bound of its density, relative to d0 (and, on the matrix cores, scaled
 * by a power of two), up to a term proportional to its own size: KEYS::widen (DESIGN.md section
 * 4; ssw_model.c for the matrix-core form).  So: the 5th key with its 7 borrowed label bits pushed
 * towards +inf bounds the keys of all densities outside the four; keys.unscaled() takes it out
 * of the scaled domain (exact); v + widen |v| + 0.001 is increasing in v, so widening the
 * bound of the keys bounds the densities; back to absolute, rounded up.
 * KEYS is the scan's form of key -- ScanKeysFma below, ScanKeysMfma in ssw_k1a_mfma.inc -- and
 * what differs between them is fixed at compile time. */
struct ScanKeysFma {
    /* 26 fused multiply-adds: 104 * 2^-24 */
    static constexpr float widen = 6.198883056640625e-06f;
    __device__ __forceinline__ float unscaled(float ub) const { return ub; }
};

/* (The bound travels in a struct, by reference into scan_proven: a float returned or passed by
 * value is marked as defined, the compiler then makes a plain AND of the `&&` in front of
 * `ub == ub`, and the default instances of the matrix-core scan come out one instruction
 * different from what they were with this text in the kernel.) */
struct ScanBound {
    float ub;
};

template <class KEYS>
__device__ __forceinline__ ScanBound
scan_upper_bound(float key5, const KEYS keys, float d0)
{
    uint32_t kb = __float_as_uint(key5);
    float ub = __uint_as_float((kb & 0x80000000u) ? (kb & ~127u) : (kb | 127u));
    ub = keys.unscaled(ub);
    ub = ub + __builtin_fabsf(ub) * KEYS::widen + 1.0e-3f;
    ub = ub + d0;
    ub = ub + __builtin_fabsf(ub) * 2.384185791015625e-07f;
    return ScanBound{ ub };
}

/* The claim of DESIGN.md section 4 for one pair: the four candidates (sorted) are four distinct
 * values, each above the bound ub of every other density.  PTM compares truncated scores (a NaN
 * bound proves nothing); the ms scorer orders by float (compute_dist), and exact ties are what
 * needs the exact pass. */
template <bool MS>
__device__ __forceinline__ bool
scan_proven(const int (&sk)[4], const float (&dv)[4], const ScanBound &bound)
{
    const float ub = bound.ub;
    if (MS)
        return dv[0] > dv[1] && dv[1] > dv[2] && dv[2] > dv[3] && dv[3] > ub;
    return sk[0] > sk[1] && sk[1] > sk[2] && sk[2] > sk[3] && ub == ub && sk[3] > dens2int(ub);
}

/* Masked batches (P.seg_of_frame != nullptr): pairs of unscanned codebooks are nobody's input.
 * The lanes whose frame t scans this codebook: what a step's need[] is cut down to. */
__device__ __forceinline__ unsigned long long
scan_mask_unscanned(const FramesParams &P, int cbf, int t)
{
    return __ballot(t < P.n_frames && cb_scanned(P, cbf / P.n_feat, t < P.n_frames ? t : 0));
}

/* ---- the exact in-wave pass --------------------------------------------------------------- */

/* Both scans redo a pair they could not prove by the whole wave, in frame order, with the
 * reference's state machine (topn_exact_step = eval_topn + eval_cb, src/ptm_mgau.c:86-225) on the
 * 128 exact densities of wave_frame_densities; lane l of step h owns frame t = t_base + 64 h + l
 * and holds its order in cpk[h].  The `while (todo)` loop, with the choice of the order frame t
 * starts from, stays written in each kernel on purpose: as a function -- the whole loop, the
 * choice alone, even the neighbouring-lane case alone -- it changes the compiled code of the
 * matrix-core scan's default instances (the unchanged text wrapped in a lambda does the same),
 * and those are what every batch runs.  What the two copies must agree on, stated once.  With
 * all 128 exact values on the table, topn_self_determined settles most pairs, history or not;
 * only real ties need the order the frame starts from.  Three cases:
 *   - an utterance's first frame: start_order (the reset history, or what the caller carried in);
 *   - the tile's first frame (h == 0 && l == 0), a frame whose predecessor did not scan this
 *     codebook (what the scan stored for it is not the reference's state), or one whose
 *     predecessor is off the chain (chain_skipped: the first frame of an utterance in a chain
 *     whose predecessor had an odd number of frames): re-derived by carried_order_of;
 *   - otherwise the previous frame's FINAL order, proven or redone a moment ago: the
 *     neighbouring lane's cpk[h], or lane 63 of step 0 for lane 0 of step 1.
 * The kernels differ in three things only: where the utterance-start bit comes from (the
 * matrix-core scan has the words prefetched, the vector-unit scan fetches the bit it needs), the
 * floor handed to topn_exact_step (s3[h]; "strictly decreasing scores"), and what happens to a
 * redone pair (stored at once; kept in registers and stored with the others).  The ms scorer
 * keeps no history: ms_exact_step.  A change to one copy goes into the other. */
