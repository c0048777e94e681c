/* ssw_k11_cont.inc -- K11: the ms scorer on continuous-density models (one codebook per senone).
 * Part of the single translation unit ssw_kernels.hip (included there, in this order).
 *
 * Restates ms_cont_mgau_frame_eval with compallsen = yes (src/ms_mgau.c:299-321) for batches.
 * With sen2cb the identity, gauden_dist of codebook s serves senone s alone, so the density
 * evaluation is the senone evaluation and the two are one kernel:
 *   cont_score_kernel  one lane per senone, CONT_FR frames per lane.  Per stream it walks the
 *                      senone's densities in index order (compute_dist, src/ms_gauden.c:349-432:
 *                      det - sum (x - mean)^2 var, four rounded operations per dimension, the
 *                      file is built without contraction), keeps the topn best of every frame in
 *                      registers (:397-429) -- or, when topn covers the codebook, none: the
 *                      densities are then combined as they come, in index order (compute_dist_all)
 *                      -- and combines them as senone_eval does (src/ms_senone.c:314-362, the
 *                      n_gauden > 1 branch).  It leaves the raw score, / aw and clamped, and folds
 *                      the frame's minimum into one word per frame
 *   cont_norm_kernel   subtracts the frame's minimum with the second clamp (src/ms_mgau.c:313-321)
 *                      and writes the row, once
 *
 * The table is senone-minor: a wave reads 64 neighbouring (mean, scale) pairs, 512 bytes, per
 * dimension, and uses them for CONT_FR frames.  The frames' features are the same for every lane:
 * the workgroup copies them to LDS, [dimension][frame], and a lane reads its four frames' values
 * of a dimension with one broadcast read.
 *
 * The early exit of compute_dist (dval >= worst->dist in the loop condition) changes no result
 * for finite input: every term subtracted is >= 0 and fp32 subtraction is monotone, so a partial
 * sum below the worst entry implies the full sum is below it.  The full sum is computed.
 *
 * Equality with the reference is claimed for finite features under which every codebook takes at
 * least topn densities.  Otherwise: a deterministic row and no fault -- a list entry that no
 * density filled keeps WORST_DIST and density 0 (the reference reads a stale id there), and every
 * index is bounded by construction, not by the data. */

constexpr int CONT_FR = 4;        /* frames per lane and table read */
constexpr int CONT_THREADS = 256; /* senones per workgroup */

struct ContParams {
    int *fmin;          /* [n_frames] the frame's smallest raw score (preset to >= 32767) */
    int16_t *raw;       /* [n_frames][n_sen] raw scores */
    int16_t *out;       /* [n_frames][n_sen] */
    int n_frames, n_sen, n_sp, n_feat, n_density, featdim, aw, zero;
    int featoff[SSW_MAX_FEAT], veclen[SSW_MAX_FEAT];
    unsigned long long toff[SSW_MAX_FEAT]; /* floats before stream f's part of the table */
};

/* compute_dist's insertion (src/ms_gauden.c:418-428) into a list kept best first: the density is
 * taken when v >= the worst entry, and stands before the first entry with v >= entry -- new before
 * equal.  One pass of compare-and-swap: from that entry on, the value carried is the entry
 * displaced, which is >= every entry behind it. */
template <int TOPN>
__device__ __forceinline__ void
cont_insert(float (&dist)[TOPN], int (&id)[TOPN], float v, int d)
{
#pragma unroll
    for (int k = 0; k < TOPN; ++k) {
        const bool take = v >= dist[k]; /* (false for a NaN) */
        const float ov = dist[k];
        const int od = id[k];
        dist[k] = take ? v : ov;
        id[k] = take ? d : od;
        v = take ? ov : v;
        d = take ? od : d;
    }
}

/* TOPN = 0: topn >= n_density, no selection.  grid: (frame tiles, senone blocks). */
template <int TOPN>
__global__ void __launch_bounds__(CONT_THREADS)
cont_score_kernel(const float *__restrict__ tab, const uint8_t *__restrict__ pdf,
                  const uint8_t *__restrict__ logadd8, const float *__restrict__ feats, ContParams P)
{
    __shared__ float4 s_x[SSW_MAX_FEAT * SSW_CONT_MAX_VECLEN]; /* [dimension][frame of the tile] */
    __shared__ uint8_t s_tab[256];
    constexpr int NL = TOPN > 0 ? TOPN : 1;
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * CONT_FR;
    const int sen = blockIdx.y * CONT_THREADS + tid;
    s_tab[tid] = logadd8[tid];
    for (int j = tid; j < P.featdim; j += CONT_THREADS) {
        float x[CONT_FR];
#pragma unroll
        for (int r = 0; r < CONT_FR; ++r) /* (a frame past the batch: nothing is read) */
            x[r] = t0 + r < P.n_frames ? feats[(size_t)(t0 + r) * P.featdim + j] : 0.0f;
        s_x[j] = make_float4(x[0], x[1], x[2], x[3]);
    }
    __syncthreads();

    int scr[CONT_FR];
#pragma unroll
    for (int r = 0; r < CONT_FR; ++r)
        scr[r] = INT_MAX;
    if (sen < P.n_sen) {
#pragma unroll
        for (int r = 0; r < CONT_FR; ++r)
            scr[r] = 0;
        for (int f = 0; f < P.n_feat; ++f) {
            const int vl = P.veclen[f];
            const float4 *xs = s_x + P.featoff[f];
            const size_t rows = 2 * (size_t)vl + 1; /* of n_sp floats per density */
            const float *tf = tab + P.toff[f];
            const uint8_t *pf = pdf + ((size_t)sen * P.n_feat + f) * P.n_density;
            float dist[CONT_FR][NL];
            int id[CONT_FR][NL];
            int fscr[CONT_FR];
#pragma unroll
            for (int r = 0; r < CONT_FR; ++r) {
                fscr[r] = 0;
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    dist[r][k] = -2147483648.0f; /* WORST_DIST */
                    id[r][k] = 0;
                }
            }
            for (int d = 0; d < P.n_density; ++d) {
                const float *td = tf + (size_t)d * rows * P.n_sp;
                const float det = td[2 * (size_t)vl * P.n_sp + sen];
                float acc[CONT_FR] = { det, det, det, det };
#pragma unroll 4
                for (int i = 0; i < vl; ++i) {
                    const float2 mv = *reinterpret_cast<const float2 *>(td + 2 * ((size_t)i * P.n_sp + sen));
                    const float4 x4 = xs[i];
                    const float x[CONT_FR] = { x4.x, x4.y, x4.z, x4.w };
#pragma unroll
                    for (int r = 0; r < CONT_FR; ++r) {
                        const float diff = x[r] - mv.x;
                        const float sq = diff * diff;
                        const float c = sq * mv.y;
                        acc[r] = acc[r] - c;
                    }
                }
                if (TOPN > 0) {
#pragma unroll
                    for (int r = 0; r < CONT_FR; ++r)
                        cont_insert<NL>(dist[r], id[r], acc[r], d);
                } else { /* compute_dist_all: every density, in index order */
                    const int w = (int)pf[d];
#pragma unroll
                    for (int r = 0; r < CONT_FR; ++r) {
                        const int fw = ms_fden(acc[r]) - w;
                        fscr[r] = d == 0 ? fw : ms_logadd(fscr[r], fw, P.zero, s_tab);
                    }
                }
            }
            if (TOPN > 0) {
#pragma unroll
                for (int r = 0; r < CONT_FR; ++r) {
                    fscr[r] = ms_fden(dist[r][0]) - (int)pf[id[r][0]];
#pragma unroll
                    for (int k = 1; k < NL; ++k)
                        fscr[r] = ms_logadd(fscr[r], ms_fden(dist[r][k]) - (int)pf[id[r][k]], P.zero,
                                            s_tab);
                }
            }
#pragma unroll
            for (int r = 0; r < CONT_FR; ++r)
                scr[r] -= fscr[r];
        }
#pragma unroll
        for (int r = 0; r < CONT_FR; ++r) {
            int v = scr[r];
            if (P.aw != 1)
                v = v / P.aw; /* C division truncates toward zero */
            v = clamp_i16(v);
            scr[r] = v;
            if (t0 + r < P.n_frames)
                P.raw[(size_t)(t0 + r) * P.n_sen + sen] = (int16_t)v;
        }
    }
#pragma unroll
    for (int r = 0; r < CONT_FR; ++r) {
        const int best = -wave_max_i32(-scr[r]); /* (lanes past n_sen hold INT_MAX) */
        if ((tid & 63) == 0 && t0 + r < P.n_frames && best != INT_MAX)
            atomicMin(P.fmin + (t0 + r), best);
    }
}

/* grid: one workgroup per frame.  RAW: the rows stay un-normalised (frame_eval over an active
 * list normalises on the host, over the listed senones). */
template <bool RAW>
__global__ void __launch_bounds__(256)
cont_norm_kernel(ContParams P)
{
    const size_t row = (size_t)blockIdx.x * P.n_sen;
    const int best = RAW ? 0 : P.fmin[blockIdx.x];
    for (int s = threadIdx.x; s < P.n_sen; s += 256) {
        P.out[row + s] = final_score<true>((int)P.raw[row + s], best);
    }
}
