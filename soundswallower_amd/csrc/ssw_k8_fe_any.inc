/* ssw_k8_fe_any.inc -- K8 for every configuration fe_init accepts (ssw_fe_batch_any).
 * Part of the single translation unit ssw_kernels.hip (included there, after ssw_k8_fe.inc). */
/* ---------------------------------------------------------------------------------- */
/* K8, any configuration: alpha, remove_dc, any ncep, htk, logspec, smoothspec           */
/* ---------------------------------------------------------------------------------- */
/* What ssw_k8_fe.inc's kernels do not compute.  The filter bank's settings (doublebw, unit_area,
 * round_filters, warping) live in the host's tables alone; fe_noise_kernel serves unchanged.
 *
 *   fe_spectrum_any_kernel<LOG2N, S>  fe_spectrum_kernel with fe_spch_to_frame whole
 *                       (src/fe_sigproc.c:293-319): alpha == 0 takes fe_copy_to_frame, and
 *                       remove_dc subtracts the frame's mean between pre-emphasis and the window
 *                       (fe_hamming_window, :277-285).  The mean is the reference's sum in index
 *                       order over the frame_size doubles, zeros of a short frame included.  Where
 *                       the host proved that no order of summing rounds (ssw_fe_dc_sum_exact: int16
 *                       samples, alpha on a coarse enough grid) the wave reduces its lanes' partial
 *                       sums; elsewhere lane 0 walks the frame in LDS in index order.
 *                       The existing kernel keeps its own copy of the FFT: with that body in a
 *                       function of its own its int16 instantiations came out with other registers
 *   fe_cep_any_kernel   fe_mel_cep and fe_lifter (src/fe_sigproc.c:609-726) for ncep 1 .. 64, every
 *                       transform, logspec and smoothspec, in the reference's types: mfcc_t float,
 *                       powspec_t double, mel_cosine, sqrt_inv_n, sqrt_inv_2n and SQRT_HALF float
 *                       (SQRT_HALF is FLOAT2MFCC(0.707106781186548), include/soundswallower/fe.h:367)
 *                       -> float [frame][out_dim] */
struct FeAnyParams {
    FeParams P;                     /* tab: the same block through ssw_fe_tables_t's fields */
    const ssw_fe_any_tables_t *any;
    int dc;                         /* enum ssw_fe_dc */
};

/* fe_fft_real's stages after the first (src/fe_sigproc.c:459-558), fe_spec_magnitude (:560-585)
 * and fe_mel_spec (:587-607) of one frame per wave, as fe_spectrum_kernel has them; every wave
 * of the workgroup calls it (the barriers) */
template <int LOG2N>
__device__ __forceinline__ void
fe_any_fft_mel(double *x, int lane, bool live, const ssw_fe_rate_t *R, int nfilt, double *mfspec_row)
{
    constexpr int N = 1 << LOG2N, PAIRS = N / 2, GROUPS = N / 4;
    if (live) {
#pragma unroll 8
        for (int t = 0; t < (PAIRS + 63) / 64; ++t) {
            const int i = 2 * (lane + 64 * t);
            if (PAIRS >= 64 || i < N) {
                const double a = x[i], b = x[i + 1];
                x[i] = a + b;
                x[i + 1] = a - b;
            }
        }
    }
    __syncthreads();
    const double *ccc = live ? fe_rate_part<double>(R, R->ccc_off) : nullptr;
    const double *sss = live ? fe_rate_part<double>(R, R->sss_off) : nullptr;
    for (int k = 1; k < LOG2N; ++k) {
        if (live) {
            const int n2 = 1 << k, n4 = 1 << (k - 1);
#pragma unroll 8
            for (int t = 0; t < (GROUPS + 63) / 64; ++t) {
                const int gi = lane + 64 * t;
                if (GROUPS < 64 && gi >= GROUPS)
                    continue;
                const int j = gi & (n4 - 1), i = (gi >> (k - 1)) << (k + 1);
                if (j == 0) {
                    const double a = x[i], b = x[i + n2];
                    x[i] = a + b;
                    x[i + n2] = a - b;
                    x[i + n2 + n4] = -x[i + n2 + n4];
                } else {
                    const int i1 = i + j, i2 = i + n2 - j, i3 = i + n2 + j, i4 = i + n2 + n2 - j;
                    const double cc = ccc[j << (LOG2N - 1 - k)], ss = sss[j << (LOG2N - 1 - k)];
                    const double x1 = x[i1], x2 = x[i2], x3 = x[i3], x4 = x[i4];
                    const double t1 = x3 * cc + x4 * ss;
                    const double t2 = x3 * ss - x4 * cc;
                    x[i4] = x2 - t2;
                    x[i3] = -x2 - t2;
                    x[i2] = x1 - t1;
                    x[i1] = x1 + t1;
                }
            }
        }
        __syncthreads();
    }
    if (live) {
#pragma unroll 8
        for (int t = 0; t < (N / 2 + 1 + 63) / 64; ++t) {
            const int j = lane + 64 * t;
            if (j == 0)
                x[0] = x[0] * x[0];
            else if (j <= N / 2)
                x[j] = x[j] * x[j] + x[N - j] * x[N - j];
        }
    }
    __syncthreads();
    if (live && lane < nfilt) {
        const float *coef = fe_rate_part<float>(R, R->coeff_off);
        const int s0 = R->spec_start[lane], c0 = R->filt_start[lane], wd = R->filt_width[lane];
        double acc = 0.0;
        for (int j = 0; j < wd; ++j)
            acc = acc + x[s0 + j] * (double)coef[c0 + j];
        mfspec_row[lane] = acc;
    }
}

template <int LOG2N, typename S>
__global__ void __launch_bounds__(64 * fe_spec_waves(LOG2N))
fe_spectrum_any_kernel(FeAnyParams A)
{
    constexpr int N = 1 << LOG2N, W = fe_spec_waves(LOG2N);
    static_assert(N >= 64, "one sample per lane at least");
    __shared__ double s_x[W][N];
    const FeParams &P = A.P;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * W + w;
    const bool live = g < P.n_grp_frames; /* wave-uniform; every wave reaches every barrier */
    const int dc = A.dc;                  /* launch-uniform */
    double *x = s_x[w];
    const ssw_fe_rate_t *R = nullptr;
    const double *ham = nullptr;
    int f = 0, size = 0;
    double part = 0.0;
    if (live) {
        const int k = fe_utt_of(P.grp_off, P.n_grp, g);
        const FeUtt U = P.utt[P.grp_utt[k]];
        const int fl = g - P.grp_off[k];
        f = U.f0 + fl;
        R = U.rate;
        size = U.size;
        const long long start = U.start + (long long)U.shift * fl;
        const long long left = U.n - (long long)U.shift * fl;
        const int half = size / 2;
        const int len = left < size ? (int)left : size;
        ham = fe_rate_part<double>(R, R->hamming_off);
        const float alpha_f = A.any->alpha;
        const double alpha = (double)alpha_f;
        const S *pcm = (const S *)P.pcm;
        const double prior = fl == 0 || alpha_f == 0.0f ? 0.0 : fe_sample(pcm, start - 1);
#pragma unroll 8
        for (int t = 0; t < N / 64; ++t) {
            const int i = lane + 64 * t;
            double v = 0.0;
            if (i < len) {
                v = fe_sample(pcm, start + i);
                if (alpha_f != 0.0f) { /* fe_pre_emphasis; else fe_copy_to_frame */
                    const double prev = i == 0 ? prior : fe_sample(pcm, start + i - 1);
                    v = v - prev * alpha;
                }
            }
            if (dc == SSW_FE_DC_NONE) {
                if (i < half)
                    v = v * ham[i];
                else if (i >= size - half && i < size)
                    v = v * ham[size - 1 - i];
            } else {
                part = part + v; /* (zero past len; used when any order is exact) */
            }
            x[__brev((unsigned)i) >> (32 - LOG2N)] = v;
        }
    }
    if (dc != SSW_FE_DC_NONE) {
        __syncthreads();
        if (live) { /* fe_hamming_window with remove_dc */
            double sum;
            if (dc == SSW_FE_DC_ANY_ORDER) {
                sum = part;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1)
                    sum = sum + __shfl_xor(sum, d);
            } else {
                sum = 0.0;
                if (lane == 0)
                    for (int i = 0; i < size; ++i)
                        sum = sum + x[__brev((unsigned)i) >> (32 - LOG2N)];
                sum = __shfl(sum, 0);
            }
            const double mean = sum / (double)size;
            const int half = size / 2;
#pragma unroll 8
            for (int t = 0; t < N / 64; ++t) {
                const int i = lane + 64 * t;
                if (i < size) {
                    const int at = __brev((unsigned)i) >> (32 - LOG2N);
                    double v = x[at] - mean;
                    if (i < half)
                        v = v * ham[i];
                    else if (i >= size - half)
                        v = v * ham[size - 1 - i];
                    x[at] = v;
                }
            }
        }
    }
    __syncthreads();
    fe_any_fft_mel<LOG2N>(x, lane, live, R, A.any->nfilt, P.mfspec + (size_t)f * A.any->nfilt);
}

/* fe_dct2 (src/fe_sigproc.c:677-699) or fe_spec2cep (:647-675): cepstrum i of the log spectrum
 * lm; htk scales C0 by sqrt_inv_2n */
__device__ __forceinline__ float
fe_any_cepstrum(const ssw_fe_any_tables_t *T, const double *lm, int i, bool legacy, bool htk)
{
    const int n = T->nfilt;
    const float *cosrow = T->mel_cosine + i * n;
    float c;
    if (!legacy) {
        if (i == 0) {
            c = (float)lm[0];
            for (int j = 1; j < n; ++j)
                c = (float)((double)c + lm[j]);
            c = c * (htk ? T->sqrt_inv_2n : T->sqrt_inv_n);
        } else {
            c = 0.0f;
            for (int j = 0; j < n; ++j)
                c = (float)((double)c + lm[j] * (double)cosrow[j]);
            c = c * T->sqrt_inv_2n;
        }
    } else {
        if (i == 0) {
            c = (float)(lm[0] / 2);
            for (int j = 1; j < n; ++j)
                c = (float)((double)c + lm[j]);
            c = (float)((double)c / (double)n);
        } else {
            c = 0.0f;
            for (int j = 0; j < n; ++j)
                c = (float)((double)c + lm[j] * (double)cosrow[j] * (double)(j == 0 ? 1 : 2));
            c = (float)((double)c / ((double)n * 2));
        }
    }
    return c;
}

__global__ void __launch_bounds__(FE_CEP_THREADS)
fe_cep_any_kernel(FeAnyParams A)
{
    __shared__ double s_lm[FE_CEP_FRAMES][SSW_FE_MAX_FILT];
    __shared__ float s_cep[FE_CEP_FRAMES][SSW_FE_MAX_CEP];
    const ssw_fe_any_tables_t *T = A.any;
    const int n = T->nfilt, ncep = T->ncep, out_dim = T->out_dim, f0 = blockIdx.x * FE_CEP_FRAMES;
    const int frames = A.P.n_frames - f0 < FE_CEP_FRAMES ? A.P.n_frames - f0 : FE_CEP_FRAMES;
    /* fe_mel_cep: LOG_FLOOR 1e-4 */
    for (int idx = threadIdx.x; idx < frames * n; idx += FE_CEP_THREADS) {
        const int r = idx / n, j = idx - r * n;
        s_lm[r][j] = fe_log(A.P.mfspec[(size_t)(f0 + r) * n + j] + 1e-4);
    }
    __syncthreads();
    if (T->log_spec == SSW_FE_RAW_LOG_SPEC) {
        for (int idx = threadIdx.x; idx < frames * n; idx += FE_CEP_THREADS) {
            const int r = idx / n, j = idx - r * n;
            A.P.cep[(size_t)(f0 + r) * out_dim + j] = (float)s_lm[r][j];
        }
        return;
    }
    const bool smooth = T->log_spec == SSW_FE_SMOOTH_LOG_SPEC; /* fe_dct2 (not htk), then fe_dct3 */
    const bool legacy = !smooth && T->transform == SSW_FE_LEGACY;
    const bool htk = !smooth && T->transform == SSW_FE_HTK;
    for (int idx = threadIdx.x; idx < frames * ncep; idx += FE_CEP_THREADS) {
        const int r = idx / ncep, i = idx - r * ncep;
        float c = fe_any_cepstrum(T, s_lm[r], i, legacy, htk);
        if (smooth) {
            s_cep[r][i] = c;
        } else {
            if (T->lifter_val) /* fe_lifter, :701-712 */
                c = c * T->lifter[i];
            A.P.cep[(size_t)(f0 + r) * out_dim + i] = c;
        }
    }
    if (!smooth)
        return;
    __syncthreads();
    for (int idx = threadIdx.x; idx < frames * n; idx += FE_CEP_THREADS) { /* fe_dct3, :714-726 */
        const int r = idx / n, i = idx - r * n;
        const float sqrt_half = (float)0.707106781186548;
        double v = (double)(s_cep[r][0] * sqrt_half);
        for (int j = 1; j < ncep; ++j)
            v = v + (double)(s_cep[r][j] * T->mel_cosine[j * n + i]);
        v = v * (double)T->sqrt_inv_2n;
        A.P.cep[(size_t)(f0 + r) * out_dim + i] = (float)v;
    }
}
