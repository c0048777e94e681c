/* ssw_k12_feat.inc -- K12: dynamic features of every type, CMN mode, LDA and svspec.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order: last, so
 * that the kernels before it keep their placement in the code object).
 *
 * feat_s2mfc2feat_block_utt (src/feat.c:977-1008) for a batch, in two launches:
 *   feat_stats_kernel   one workgroup per utterance, a lane per cepstral dimension:
 *                       the utterance's mean and, with varnorm, its scale (cmn, src/cmn.c:159-224);
 *                       the prior with cmn = live
 *   feat_chain_kernel   instead of it with cmn = live and a state: ONE workgroup walks the batch's
 *                       utterances in order (cmn_live and its shift, cmn_live_update,
 *                       src/cmn_live.c:60-134)
 *   feat_tile_kernel    frame-parallel over tiles of TF frames (host-built table: utterance, first
 *                       frame; a tile never spans two utterances): the tile's frames and `window`
 *                       on either side into LDS, normalised as they are loaded, then every raw
 *                       dimension by its recipe (SSW_FEAT_RECIPE, ssw_internal.h), the LDA
 *                       (src/lda.c:124-144) and the subvector gather (src/feat.c:346-366).
 * Every float operation is the reference's, rounded once (no contraction), in its order. */
struct FeatTile {
    int utt, first; /* first: the tile's first frame, counted from the batch's frame 0 */
};

struct FeatExParams {
    const float *cep;        /* [n_frames][C] */
    const int *utt_off;      /* [n_utts + 1] */
    const FeatTile *tiles;   /* [gridDim.x] */
    const uint32_t *recipe;  /* [raw_dim] */
    const float *lda_t;      /* [raw_dim][lda_rows], NULL = no LDA */
    const int *sv;           /* [sv_dim], NULL = no svspec */
    float *mean, *scale;     /* [n_utts][C] each */
    float *state;            /* mean[C] | sum[C] | nframe (an int's bits); feat_chain_kernel
                              * writes the same once more behind it: the state it leaves */
    float *out;              /* [n_frames][out_dim] */
    int n_utts, C, window, raw_dim, lda_rows, sv_dim, out_dim, tf;
    int cmn, varnorm;        /* enum ssw_cmn */
};

constexpr int FEATEX_THREADS = 256;
constexpr int FEATEX_STAT_FLOATS = 4096; /* 16 KB of LDS: the frames a workgroup loads together */

/* body(c0, c[lane]) for every frame of an utterance in order, in the lanes below C.  The sums
 * are sequential by definition; the loads are not: the whole workgroup brings a block of
 * FEATEX_STAT_FLOATS / C frames into LDS in one sweep, then the first C lanes walk it.  Every
 * thread of the workgroup calls this (it holds barriers; n and C are the same for all). */
template <typename F>
__device__ __forceinline__ void
feat_for_frames(const float *cep, int n, int C, float *s_blk, F body)
{
    const int rows = FEATEX_STAT_FLOATS / C, tid = threadIdx.x;
    for (int f0 = 0; f0 < n; f0 += rows) {
        const int nb = min(rows, n - f0);
        const float *src = cep + (size_t)f0 * C;
        for (int i = tid; i < nb * C; i += FEATEX_THREADS)
            s_blk[i] = src[i];
        __syncthreads();
        if (tid < C) {
#pragma unroll 8
            for (int r = 0; r < nb; ++r)
                body(s_blk[r * C], s_blk[r * C + tid]);
        }
        __syncthreads();
    }
}

/* sum[lane] += c[f][lane] over the frames with c0 >= 0, frame after frame (src/cmn.c:175-187,
 * src/cmn_live.c:117-129) */
__device__ __forceinline__ void
feat_sum_frames(const float *cep, int n, int C, float *s_blk, float &sum, int &nframe)
{
    feat_for_frames(cep, n, C, s_blk, [&](float c0, float v) {
        const bool counted = !(c0 < 0); /* "skip zero energy frames" */
        sum = counted ? sum + v : sum;
        nframe += counted;
    });
}

__global__ void __launch_bounds__(FEATEX_THREADS)
feat_stats_kernel(FeatExParams P)
{
    __shared__ float s_blk[FEATEX_STAT_FLOATS];
    const int u = blockIdx.x, lane = threadIdx.x, C = P.C;
    const int t0 = P.utt_off[u], n = P.utt_off[u + 1] - t0;
    if (n <= 0)
        return;
    const float *cep = P.cep + (size_t)t0 * C;
    if (P.cmn == SSW_CMN_LIVE) {
        /* a fresh decoder's first utterance: the prior throughout (src/cmn_live.c:125) */
        if (lane < C)
            P.mean[(size_t)u * C + lane] = P.state[lane];
        return;
    }
    float sum = 0.0f;
    int nframe = 0;
    feat_sum_frames(cep, n, C, s_blk, sum, nframe);
    const float mean = sum / nframe; /* float / int, src/cmn.c:190 */
    if (lane < C)
        P.mean[(size_t)u * C + lane] = mean;
    if (!P.varnorm)
        return;
    /* src/cmn.c:206-216: over ALL frames, t = c - mean, var += t * t (two roundings) */
    float var = 0.0f;
    feat_for_frames(cep, n, C, s_blk, [&](float, float v) {
        const float t = v - mean;
        const float tt = t * t;
        var += tt;
    });
    /* (float)sqrt((float64)n_frame / var): a double division and a double square root */
    if (lane < C)
        P.scale[(size_t)u * C + lane] = (float)sqrt((double)n / (double)var);
}

/* cmn_live_shiftwin (hwm_inclusive: nframe >= CMN_WIN_HWM) and cmn_live_update (nframe >
 * CMN_WIN_HWM), src/cmn_live.c:60-104 */
__device__ __forceinline__ void
feat_live_renew(float &mean, float &sum, int &nframe, bool hwm_inclusive)
{
    float sf = 1.0f / nframe;
    mean = sum / nframe;
    if (hwm_inclusive ? nframe >= 800 : nframe > 800) {
        sf = 500 * sf; /* CMN_WIN */
        sum = sum * sf;
        nframe = 500;
    }
}

/* one workgroup; its first C lanes carry the state from utterance to utterance */
__global__ void __launch_bounds__(FEATEX_THREADS)
feat_chain_kernel(FeatExParams P)
{
    __shared__ float s_blk[FEATEX_STAT_FLOATS];
    const int lane = threadIdx.x, C = P.C;
    const bool mine = lane < C;
    float mean = mine ? P.state[lane] : 0.0f, sum = mine ? P.state[C + lane] : 0.0f;
    int nframe = __float_as_int(P.state[2 * C]);
    for (int u = 0; u < P.n_utts; ++u) {
        const int t0 = P.utt_off[u], n = P.utt_off[u + 1] - t0;
        if (mine)
            P.mean[(size_t)u * C + lane] = mean; /* what the utterance's frames have subtracted */
        if (n > 0) {
            feat_sum_frames(P.cep + (size_t)t0 * C, n, C, s_blk, sum, nframe);
            if (nframe > 800) /* CMN_WIN_HWM, src/cmn_live.c:131-133 */
                feat_live_renew(mean, sum, nframe, true);
        }
        if (nframe > 0) /* cmn_live_update at the utterance's end, src/feat.c:944-945 */
            feat_live_renew(mean, sum, nframe, false);
    }
    if (!mine)
        return;
    float *after = P.state + 2 * C + 1; /* the state behind the last utterance, same layout */
    after[lane] = mean;
    after[C + lane] = sum;
    if (lane == 0)
        after[2 * C] = __int_as_float(nframe);
}

__global__ void __launch_bounds__(FEATEX_THREADS)
feat_tile_kernel(FeatExParams P)
{
    extern __shared__ float s_feat[];
    const int tid = threadIdx.x, C = P.C, W = P.window, R = P.raw_dim;
    const FeatTile tile = P.tiles[blockIdx.x];
    const int u = tile.utt, t0 = P.utt_off[u], n = P.utt_off[u + 1] - t0;
    const int f0 = tile.first - t0;                   /* the tile's first frame in its utterance */
    const int nloc = min(P.tf, n - f0);
    const int rows = nloc + 2 * W;
    float *s_cep = s_feat;                            /* [rows][C]: frames f0 - W .. */
    float *s_raw = s_cep + (P.tf + 2 * W) * C;        /* [tf][R], with an LDA or a svspec */
    float *s_y = s_raw + P.tf * R;                    /* [tf][lda_rows], with both */
    const bool direct = P.lda_t == nullptr && P.sv == nullptr;
    const float *cep = P.cep + (size_t)t0 * C;
    const float *mean = P.mean + (size_t)u * C, *scale = P.scale + (size_t)u * C;

    /* the frames, normalised; before the first / after the last frame of the utterance that
     * frame again (src/feat.c:997-1002) */
    for (int idx = tid; idx < rows * C; idx += FEATEX_THREADS) {
        const int r = idx / C, i = idx - r * C;
        int f = f0 - W + r;
        f = f < 0 ? 0 : (f >= n ? n - 1 : f);
        float x = cep[(size_t)f * C + i];
        if (P.cmn == SSW_CMN_BATCH) {
            x = x - mean[i];
            if (P.varnorm)
                x = x * scale[i];
        } else if (P.cmn == SSW_CMN_LIVE) {
            if (!(cep[(size_t)f * C] < 0)) /* "skip zero energy frames", src/cmn_live.c:119-121 */
                x = x - mean[i];
        }
        s_cep[idx] = x;
    }
    __syncthreads();
    /* every raw dimension by its recipe */
    float *out = P.out + (size_t)tile.first * P.out_dim;
    for (int idx = tid; idx < nloc * R; idx += FEATEX_THREADS) {
        const int f = idx / R, k = idx - f * R;
        const uint32_t rc = P.recipe[k];
        const int op = rc & 3, i = (rc >> 2) & 63;
        /* frame f + o of the tile is row f + W + o of s_cep; |o| <= W */
        const int at = (f + W - SSW_FEAT_MAX_WIN) * C + i;
        float v = s_cep[at + (int)((rc >> 8) & 31) * C];
        if (op >= 1)
            v = v - s_cep[at + (int)((rc >> 13) & 31) * C];
        if (op == 2) {
            const float d2 = s_cep[at + (int)((rc >> 18) & 31) * C] - s_cep[at + (int)((rc >> 23) & 31) * C];
            v = v - d2;
        }
        if (direct)
            out[idx] = v; /* (out_dim == R: the tile's rows are one run of floats) */
        else
            s_raw[idx] = v;
    }
    if (direct)
        return;
    __syncthreads();
    const float *pre = s_raw;
    int pre_dim = R;
    if (P.lda_t != nullptr) {
        /* tmp[j] = 0; tmp[j] += x[k] * lda[j][k] for k in order, src/lda.c:135-140: a lane per
         * (frame, j), the matrix read [k][j] (coalesced), x[k] an LDS broadcast */
        const int J = P.lda_rows;
        float *y = P.sv != nullptr ? s_y : nullptr;
        for (int idx = tid; idx < nloc * J; idx += FEATEX_THREADS) {
            const int f = idx / J, j = idx - f * J;
            const float *x = s_raw + f * R;
            float acc = 0.0f;
            for (int k = 0; k < R; ++k) {
                const float prod = x[k] * P.lda_t[k * J + j];
                acc += prod;
            }
            if (y != nullptr)
                y[idx] = acc;
            else
                out[idx] = acc; /* (out_dim == J) */
        }
        if (y == nullptr)
            return;
        __syncthreads();
        pre = s_y;
        pre_dim = J;
    }
    /* feat_subvec_project, src/feat.c:346-366; behind an LDA the row's floats from lda_rows on
     * are the zeros of its tmp buffer (src/lda.c:135, :141) */
    const int S = P.sv_dim;
    for (int idx = tid; idx < nloc * S; idx += FEATEX_THREADS) {
        const int f = idx / S, d = P.sv[idx - f * S];
        out[idx] = d < pre_dim ? pre[f * pre_dim + d] : 0.0f;
    }
}
