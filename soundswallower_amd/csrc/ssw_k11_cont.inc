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
 * and with compallsen = no (src/ms_mgau.c:322-365), for a model that was given the senone-major
 * table (ssw_model_enable_active):
 *   cont_listed_kernel one wave per frame, a group of lanes per LISTED senone; at the end of
 *                      this file, with its argument
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

/* ms_cont_mgau_frame_eval with compallsen = no (src/ms_mgau.c:322-365) for every frame of a
 * batch, each frame with a listed set of its own: only the listed senones' codebooks are
 * evaluated, the normaliser is the best LISTED score, and the rest of the row is left alone.
 * The shape is senone_listed_kernel's (ssw_k7_fpactive.inc): one WAVE per frame, four frames per
 * workgroup, the listed senones taken from the frame's bitmap (bridges are ordinary bits) into
 * LDS, `full` 0 / 1 / 2 exactly as its MS instance.  The bitmap row of frame t is row_of_frame[t]
 * (NULL: t), so that the frames of a segment of an alignment share one row.
 *
 * The table is the SENONE-MAJOR one (ssw_host_model_t::cont_rec_sm): the record of (senone,
 * stream) is contiguous -- per dimension the n_density (mean, scale) pairs, then the dets -- and a
 * listed senone's data is a gather of whole records.  A group of G lanes, G the power of two at
 * or above n_density, serves one listed senone: lane d of the group evaluates density d of every
 * stream (its loads of a dimension are the group's 8 n_density neighbouring bytes), 64 / G senones
 * of the list in flight per wave.
 *
 * Equality with cont_score_kernel, for any input:
 *   distance     acc = det, then per dimension in index order diff = x - mean, sq = diff diff,
 *                c = sq scale, acc -= c: the same four rounded operations on the same floats
 *   selection    cont_select_rank (ssw_cont_select.inc, where the argument stands): the list
 *                cont_insert leaves holds, slot by slot, the eligible densities of rank < topn
 *                and (WORST_DIST, density 0) behind them.  A lane writes its term
 *                ms_fden(dist) - pdf[d] into the slot of its rank; the slots were preset to the
 *                start-up entry's term
 *   combination  the group's first lane runs ms_logadd over the slots in order; with topn >=
 *                n_density every density's term stands in slot d, no eligibility test, as the
 *                TOPN = 0 branch of cont_score_kernel combines them
 *   then         / aw (C division), clamp_i16, the wave's minimum over the listed entries
 *                (wave_best_or_zero), final_score<true>
 * Padding lanes (d >= n_density) and the groups past the list's end hold a NaN distance that no
 * lane ever fetches (cont_select_rank reads densities below n_density of its own group); they
 * load nothing and write no slot.  Every index is bounded by construction, not by the data. */
struct ContListedParams {
    const float *tab;            /* the senone-major table */
    const uint8_t *pdf;          /* [n_sen][n_feat][n_density] */
    const uint8_t *logadd8;
    const float *feats;          /* [n_frames][featdim] */
    const uint32_t *listed;      /* [rows][nw32] */
    const int32_t *row_of_frame; /* NULL, or [n_frames] */
    int16_t *out;                /* [n_frames][n_sen] */
    const int16_t *yes;          /* full == 2: the whole-row scores, laid out like out */
    int n_frames, n_sen, nw32, n_feat, n_density, featdim, aw, zero;
    int topn;                    /* 0: every density, in index order */
    int cap, full;
    int featoff[SSW_MAX_FEAT], veclen[SSW_MAX_FEAT];
    unsigned long long rec_off[SSW_MAX_FEAT]; /* floats before stream f's record in a senone's block */
    unsigned long long sen_floats;            /* floats of a senone's block */
};

/* LOG2G: G = 1 << LOG2G lanes per senone */
template <int LOG2G>
__global__ void __launch_bounds__(256)
cont_listed_kernel(ContListedParams P)
{
    constexpr int G = 1 << LOG2G, NG = 64 / G;
    __shared__ uint8_t s_tab[256];
    extern __shared__ __align__(16) unsigned char fpa_smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const ContListedCarve carve(P.featdim, P.cap);
    unsigned char *mine = fpa_smem + carve.wave(w);
    float *s_x = reinterpret_cast<float *>(mine + carve.x());
    int *s_fw = reinterpret_cast<int *>(mine + carve.fw());
    uint16_t *s_sen = reinterpret_cast<uint16_t *>(mine + carve.sen());
    int16_t *s_a = reinterpret_cast<int16_t *>(mine + carve.a());
    int *s_n = reinterpret_cast<int *>(mine + carve.count());
    s_tab[tid] = P.logadd8[tid];
    if (lane == 0)
        *s_n = 0;
    __syncthreads();
    const int t = (int)blockIdx.x * 4 + w;
    if (t >= P.n_frames)
        return;
    const size_t brow = P.row_of_frame != nullptr ? (size_t)P.row_of_frame[t] : (size_t)t;
    const uint32_t *bits = P.listed + brow * P.nw32;
    /* the listed senones, in any order */
    for (int i = lane; i < P.nw32; i += 64) {
        uint32_t word = bits[i];
        if (32 * i + 32 > P.n_sen) /* (the last word: no senone past the row's end) */
            word &= (1u << (P.n_sen - 32 * i)) - 1u;
        if (word != 0u) {
            int pos = atomicAdd(s_n, __popc(word));
            while (word != 0u) {
                const int b = __builtin_ctz(word);
                word &= word - 1u;
                if (pos < P.cap)
                    s_sen[pos] = (uint16_t)(32 * i + b);
                ++pos;
            }
        }
    }
    for (int j = lane; j < P.featdim; j += 64)
        s_x[j] = P.feats[(size_t)t * P.featdim + j];
    wave_sync();
    const int n_all = *s_n;
    const int n_ent = n_all < P.cap ? n_all : P.cap; /* (cap = n_sen: never short) */
    const int d = lane & (G - 1), grp = lane >> LOG2G, gbase = lane & ~(G - 1);
    const int n_comb = P.topn > 0 ? P.topn : P.n_density; /* <= n_density <= G */
    int best = INT_MAX;
    for (int i0 = 0; i0 < n_ent; i0 += NG) { /* (uniform: the shuffles below need every lane) */
        const int i = i0 + grp;
        const bool live = i < n_ent && d < P.n_density;
        const int sen = i < n_ent ? (int)s_sen[i] : 0;
        const float *ts = P.tab + (size_t)sen * P.sen_floats;
        int scr = 0;
        for (int f = 0; f < P.n_feat; ++f) {
            const int vl = P.veclen[f];
            const float *xs = s_x + P.featoff[f];
            const float *tr = ts + P.rec_off[f];
            const uint8_t *pf = P.pdf + ((size_t)sen * P.n_feat + f) * P.n_density;
            float acc = __builtin_nanf("");
            int wgt = 0;
            if (live) {
                acc = tr[2 * (size_t)vl * P.n_density + d];
                wgt = (int)pf[d];
                const float2 *mv = reinterpret_cast<const float2 *>(tr) + d;
#pragma unroll 4
                for (int j = 0; j < vl; ++j) {
                    const float2 p = mv[(size_t)j * P.n_density];
                    const float diff = xs[j] - p.x;
                    const float sq = diff * diff;
                    const float c = sq * p.y;
                    acc = acc - c;
                }
            }
            int slot = live ? d : -1;
            if (P.topn > 0) {
                const int rank = cont_select_rank(acc, d, P.n_density, [&](int e) {
                    return __shfl(acc, gbase + e, 64);
                });
                slot = live && rank >= 0 && rank < P.topn ? rank : -1;
                /* the start-up entry's term, (WORST_DIST, density 0): lane 0 of the group holds
                 * pdf[0] */
                const int w0 = __shfl(wgt, gbase, 64);
                s_fw[lane] = ms_fden(SSW_CONT_WORST_DIST) - w0;
                wave_sync();
            }
            if (slot >= 0)
                s_fw[gbase + slot] = ms_fden(acc) - wgt;
            wave_sync();
            if (d == 0 && i < n_ent) {
                int fscr = s_fw[gbase];
                for (int k = 1; k < n_comb; ++k)
                    fscr = ms_logadd(fscr, s_fw[gbase + k], P.zero, s_tab);
                scr -= fscr;
            }
            wave_sync(); /* (the slots are rewritten by the next stream) */
        }
        if (d == 0 && i < n_ent) {
            const int a = ms_finish(scr, P.aw);
            s_a[i] = (int16_t)a;
            best = a < best ? a : best;
        }
    }
    best = wave_best_or_zero(best); /* 0: a frame the search has no HMM left in (it fails there) */
    wave_sync();
    int16_t *orow = P.out + (size_t)t * P.n_sen;
    if (P.full == 2) {
        const int16_t *yrow = P.yes + (size_t)t * P.n_sen;
        int delta = INT_MAX; /* the yes score of a best listed senone */
        for (int i = lane; i < n_ent; i += 64)
            if ((int)s_a[i] == best) {
                const int y = yrow[s_sen[i]];
                delta = y < delta ? y : delta;
            }
        delta = -wave_max_dpp(-delta);
        if (delta == INT_MAX)
            delta = 0;
        for (int sen = lane; sen < P.n_sen; sen += 64)
            if (!((bits[sen >> 5] >> (sen & 31)) & 1u)) {
                orow[sen] = (int16_t)clamp_i16((int)yrow[sen] - delta);
            }
    } else if (P.full) { /* the unlisted entries first: listed ones are skipped, no store is overwritten */
        for (int sen = lane; sen < P.n_sen; sen += 64)
            if (!((bits[sen >> 5] >> (sen & 31)) & 1u))
                orow[sen] = (int16_t)0;
    }
    for (int i = lane; i < n_ent; i += 64)
        orow[s_sen[i]] = final_score<true>((int)s_a[i], best);
}
