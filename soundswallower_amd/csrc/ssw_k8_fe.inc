/* ssw_k8_fe.inc -- K8: the MFCC front end, whole utterances.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* K8: PCM -> cepstra (fe_process_int16 / fe_process_float32 + fe_end, whole utterances)  */
/* ---------------------------------------------------------------------------------- */
/* The reference's front end, frame by frame (src/fe_sigproc.c:219-738, src/fe_noise.c:111-327),
 * in its own types: pre-emphasis, window, FFT, power and mel spectra in double, the noise
 * tracker in double, log in double, the DCT with float accumulators rounded after every add.
 * The only operations that are not +, -, *, / or a compare are the log (fe_log, ssw_fe_log.inc:
 * correctly rounded, as a good libm's is for all but a few arguments in 100,000; DESIGN K8) and
 * the conversions.  The tables come from the host (csrc/ssw_model.c), built as fe_init builds them.
 *
 * Framing (src/fe_interface.c:560-712) at any rate: frame f of an utterance of n samples covers
 * samples shift f .. shift f + min(size, n - shift f) - 1, zero-padded to the FFT size N; the
 * last frame is fe_end's overflow frame.  The pre-emphasis's prior sample is 0 for frame 0 and
 * sample shift f - 1 after it (fe_spch_to_frame keeps spch[frame_shift - 1]; the overflow frame
 * starts where the next full frame would), so frames are independent up to the noise tracker.
 * Each utterance's shift, size and table block (ssw_fe_rate_t: window, twiddles, filters) come
 * from its FeUtt record; ssw_fe_batch's are 160, 410 and the 16 kHz block.
 *
 *   fe_spectrum_kernel<LOG2N>  one wave per frame, N = 2^LOG2N = 64 .. 8192, one launch per N
 *                       present in the batch over that group's frames: samples -> pre-emphasis
 *                       -> Hamming, stored straight to bit-reversed LDS positions (fe_fft_real's
 *                       first loop is exactly that permutation), the pair stage and stages
 *                       k = 1..LOG2N-1 with fe_fft_real's butterflies (those of a stage touch
 *                       disjoint points: N/4 per stage, lanes past N/4 idle at N = 64 and 128),
 *                       the power spectrum in place, mel sums in the reference's j order
 *                       -> double mfspec [frame][nfilt]
 *                       fe_spectrum_kernel<LOG2N, S>: S = int16_t, or float for ssw_fe_batch_f32,
 *                       where a sample is (double)(float)(x * 32768.0f), as fe_process_float32
 *                       stores it (fe_sample)
 *   fe_noise_kernel     remove_noise: one wave per utterance, lane = filter, frames in order
 *                       (the tracker is a recurrence); the +-4 gain smoothing by lane shuffles
 *   fe_cep_kernel       log(mfspec + 1e-4), then DCT-II (transform = dct) or fe_spec2cep
 *                       (legacy), then the lifter -> float cep [frame][13] */
struct FeUtt {
    long long start, n;         /* first sample in pcm, samples */
    const ssw_fe_rate_t *rate;  /* the table block of the utterance's (samprate, nfft) */
    int f0, shift, size, pad;   /* first frame in the batch, frame shift and size in samples */
};

struct FeParams {
    const void *pcm;           /* fe_spectrum_kernel's S: int16_t or float */
    const FeUtt *utt;          /* [n_utts] */
    const int *frame_off;      /* [n_utts + 1] */
    const int *grp_utt;        /* fe_spectrum_kernel: the utterances of the launch's FFT size */
    const int *grp_off;        /* [n_grp + 1]: their frames' prefix within the launch */
    const ssw_fe_tables_t *tab;
    double *mfspec;            /* [n_frames][nfilt] */
    float *cep;                /* [n_frames][13] */
    int n_utts, n_frames, n_grp, n_grp_frames;
};

/* frames per workgroup of the spectrum kernel: N doubles of LDS per wave, so 16 KB at N = 512
 * (4 waves), 32 KB at 2048 (2 waves), 64 KB at 8192 (1 wave; 160 KiB per CU) */
__host__ __device__ constexpr int
fe_spec_waves(int log2n)
{
    return log2n <= 10 ? 4 : log2n == 11 ? 2 : 1;
}
constexpr int FE_CEP_FRAMES = 16; /* frames per workgroup of the cepstrum kernel */
constexpr int FE_CEP_THREADS = 256;
static_assert(FE_CEP_FRAMES * SSW_FE_NCEP <= FE_CEP_THREADS, "one thread per cepstrum");

/* the entry that holds frame f: the last u with off[u] <= f (empty entries have
 * off[u] == off[u + 1] and are passed over) */
__device__ __forceinline__ int
fe_utt_of(const int *off, int n, int f)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= f)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

template <typename T>
__device__ __forceinline__ const T *
fe_rate_part(const ssw_fe_rate_t *R, int off)
{
    return (const T *)((const char *)R + off);
}

/* One sample as fe_spch_to_frame reads it from spch: an int16 as it is (fe_process_int16 copies
 * the samples, src/fe_sigproc.c:319-348, 378-411), a float32 as the float it was stored as,
 * spch[i] = sample * FLOAT32_SCALE (32768.0F; src/fe_sigproc.c:350-376, 413-444, and
 * create_overflow_frame for fe_end's frame, src/fe_interface.c:503-510).  The product is by a
 * power of two: exact, subnormal results included (the kernels run with float denormals on),
 * unless it overflows to infinity.  No address is computed from a sample. */
__device__ __forceinline__ double
fe_sample(const int16_t *pcm, long long i)
{
    return (double)pcm[i];
}

__device__ __forceinline__ double
fe_sample(const float *pcm, long long i)
{
    return (double)(float)(pcm[i] * 32768.0f);
}

/* S: the sample type, int16_t (ssw_fe_batch, ssw_fe_batch_ex) or float (ssw_fe_batch_f32).  The
 * type is a parameter of the kernel itself: with the body in a function of its own the int16
 * instantiations at N = 4096 and 8192 came out with other registers than before */
template <int LOG2N, typename S>
__global__ void __launch_bounds__(64 * fe_spec_waves(LOG2N))
fe_spectrum_kernel(FeParams P)
{
    constexpr int N = 1 << LOG2N, W = fe_spec_waves(LOG2N);
    constexpr int PAIRS = N / 2, GROUPS = N / 4; /* pair-stage and per-stage butterflies */
    static_assert(N >= 64, "one sample per lane at least");
    __shared__ double s_x[W][N];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * W + w;      /* frame within the launch's group */
    const bool live = g < P.n_grp_frames;  /* wave-uniform; every wave reaches every barrier */
    double *x = s_x[w];
    const ssw_fe_rate_t *R = nullptr;
    int f = 0;
    if (live) {
        /* fe_spch_to_frame (src/fe_sigproc.c:276-317) into fe_fft_real's bit-reversed order */
        const int k = fe_utt_of(P.grp_off, P.n_grp, g);
        const FeUtt U = P.utt[P.grp_utt[k]];
        const int fl = g - P.grp_off[k];
        f = U.f0 + fl;
        R = U.rate;
        const long long start = U.start + (long long)U.shift * fl;
        const long long left = U.n - (long long)U.shift * fl;
        const int size = U.size, half = size / 2;
        const int len = left < size ? (int)left : size;
        const double *ham = fe_rate_part<double>(R, R->hamming_off);
        const double alpha = (double)P.tab->alpha;
        const S *pcm = (const S *)P.pcm;
        const double prior = fl == 0 ? 0.0 : fe_sample(pcm, start - 1);
#pragma unroll 8
        for (int t = 0; t < N / 64; ++t) {
            const int i = lane + 64 * t;
            double v = 0.0;
            if (i < len) {
                const double prev = i == 0 ? prior : fe_sample(pcm, start + i - 1);
                v = fe_sample(pcm, start + i) - prev * alpha;
            }
            /* fe_hamming_window: the first and last size / 2 samples (an odd size's middle
             * sample is not windowed) */
            if (i < half)
                v = v * ham[i];
            else if (i >= size - half && i < size)
                v = v * ham[size - 1 - i];
            x[__brev((unsigned)i) >> (32 - LOG2N)] = v;
        }
    }
    __syncthreads();
    if (live) { /* fe_fft_real's first stage: pairs */
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
    for (int k = 1; k < LOG2N; ++k) { /* stages 1..LOG2N-1: N/4 butterfly groups each */
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
    if (live) { /* fe_spec_magnitude, src/fe_sigproc.c:560-585, in place: spec[j] -> x[j].
                 * x[j] (j < N/2) is read only by the lane that computes spec[j], and x[N/2] only
                 * by spec[N/2]'s; both read before they write, so no lane reads a point that
                 * another has overwritten */
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
    if (live && lane < P.tab->nfilt) { /* fe_mel_spec, src/fe_sigproc.c:587-607 */
        const float *coef = fe_rate_part<float>(R, R->coeff_off);
        const int s0 = R->spec_start[lane], c0 = R->filt_start[lane], wd = R->filt_width[lane];
        double acc = 0.0;
        for (int j = 0; j < wd; ++j)
            acc = acc + x[s0 + j] * (double)coef[c0 + j];
        P.mfspec[(size_t)f * P.tab->nfilt + lane] = acc;
    }
}

/* fe_remove_noise, src/fe_noise.c:247-327 with fe_lower_envelope :111-128, fe_temp_masking
 * :130-149, fe_weight_smooth :151-176 (SMOOTH_WINDOW 4); state reset per utterance
 * (fe_start_utt -> fe_reset_noise_stats) */
__global__ void __launch_bounds__(64)
fe_noise_kernel(FeParams P)
{
    const double lambda_power = 0.7, lambda_a = 0.995, lambda_b = 0.5, lambda_t = 0.85,
                 mu_t = 0.2, max_gain = 20.0, inv_max_gain = 1.0 / 20.0;
    const double comp_power = 1 - lambda_power, comp_a = 1 - lambda_a, comp_b = 1 - lambda_b;
    const int u = blockIdx.x, lane = threadIdx.x;
    const int f0 = P.frame_off[u], nf = P.frame_off[u + 1] - f0;
    const int n = P.tab->nfilt;
    const bool act = lane < n;
    const int l1 = lane - 4 > 0 ? lane - 4 : 0, l2 = lane + 4 < n - 1 ? lane + 4 : n - 1;
    const double width = (double)(l2 - l1 + 1);
    double *mf = P.mfspec + (size_t)f0 * n + lane;
    double power = 0.0, noise = 0.0, floor_ = 0.0, peak = 0.0;
    /* the recurrence is sequential; the loads are not: CH frames in flight */
    constexpr int CH = 8;
    for (int b = 0; b < nf; b += CH) {
        double v[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k)
            v[k] = act && b + k < nf ? mf[(size_t)(b + k) * n] : 0.0;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            if (b + k >= nf)
                break;
            const double m = v[k];
            double gain = 0.0;
            if (act) {
                if (b + k == 0) { /* noise_stats->undefined */
                    power = m;
                    noise = m / max_gain;
                    floor_ = m / max_gain;
                    peak = 0.0;
                }
                power = lambda_power * power + comp_power * m;
                if (power >= noise)
                    noise = lambda_a * noise + comp_a * power;
                else
                    noise = lambda_b * noise + comp_b * power;
                double signal = power - noise;
                if (signal < 1.0)
                    signal = 1.0;
                if (signal >= floor_)
                    floor_ = lambda_a * floor_ + comp_a * signal;
                else
                    floor_ = lambda_b * floor_ + comp_b * signal;
                const double cur_in = signal;
                peak *= lambda_t;
                if (signal < lambda_t * peak)
                    signal = peak * mu_t;
                if (cur_in > peak)
                    peak = cur_in;
                if (signal < floor_)
                    signal = floor_;
                if (signal < max_gain * power)
                    gain = signal / power;
                else
                    gain = max_gain;
                if (gain < inv_max_gain)
                    gain = inv_max_gain;
            }
            /* coef = gain[l1] + ... + gain[l2], from 0, in that order */
            double coef = 0.0;
#pragma unroll
            for (int d = -4; d <= 4; ++d) {
                const int src = lane + d;
                const double gd = __shfl(gain, src < 0 ? 0 : (src > 63 ? 63 : src));
                if (src >= 0 && src < n)
                    coef += gd;
            }
            if (act)
                mf[(size_t)(b + k) * n] = m * (coef / width);
        }
    }
}

__global__ void __launch_bounds__(FE_CEP_THREADS)
fe_cep_kernel(FeParams P)
{
    __shared__ double s_lm[FE_CEP_FRAMES][SSW_FE_MAX_FILT];
    const ssw_fe_tables_t *T = P.tab;
    const int n = T->nfilt, f0 = blockIdx.x * FE_CEP_FRAMES;
    /* fe_mel_cep, src/fe_sigproc.c:609-646: LOG_FLOOR 1e-4 */
    for (int idx = threadIdx.x; idx < FE_CEP_FRAMES * n; idx += FE_CEP_THREADS) {
        const int r = idx / n, j = idx - r * n;
        if (f0 + r < P.n_frames)
            s_lm[r][j] = fe_log(P.mfspec[(size_t)(f0 + r) * n + j] + 1e-4);
    }
    __syncthreads();
    const int r = threadIdx.x / SSW_FE_NCEP, i = threadIdx.x - r * SSW_FE_NCEP, f = f0 + r;
    if (r >= FE_CEP_FRAMES || f >= P.n_frames)
        return;
    const double *lm = s_lm[r];
    const float *cosrow = T->mel_cosine + i * n;
    float c;
    if (T->transform == SSW_FE_DCT) { /* fe_dct2, src/fe_sigproc.c:677-700 */
        if (i == 0) {
            c = (float)lm[0];
            for (int j = 1; j < n; ++j)
                c = (float)((double)c + lm[j]);
            c = c * T->sqrt_inv_n;
        } else {
            c = 0.0f;
            for (int j = 0; j < n; ++j)
                c = (float)((double)c + lm[j] * (double)cosrow[j]);
            c = c * T->sqrt_inv_2n;
        }
    } else { /* fe_spec2cep (transform = legacy), src/fe_sigproc.c:647-676 */
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
    if (T->lifter_val) /* fe_lifter, src/fe_sigproc.c:701-712: after either transform */
        c = c * T->lifter[i];
    P.cep[(size_t)f * SSW_FE_NCEP + i] = c;
}
