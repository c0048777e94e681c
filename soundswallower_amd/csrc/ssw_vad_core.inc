/* ssw_vad_core.inc -- the arithmetic of the reference's voice activity detector, once, for the
 * host path (ssw_vad.c, C) and the kernel (ssw_k13_vad.inc, HIP) alike.  Each function restates
 * what the cited reference lines compute.  Where every intermediate narrowing to int16 decides
 * bits -- GmmProbability's model update above all -- the restatement goes operation by operation
 * and keeps the reference's names for the intermediates (nmk2, delt, tmp1_s32, ...), so that a
 * line here can be held against the line it cites; the structure around them (working memory in
 * slots, fused resamplers, no per-call arrays) is this project's.
 *
 * The includer defines
 *   VAD_FN            the functions' qualifiers (static inline / __device__ __forceinline__)
 *   SSW_VAD_PITCH     distance, in int16 slots, between consecutive slots of one stream's
 *                     working memory: 1 on the host, the lanes' interleave in LDS on the device
 *   VAD_UNROLL        a pragma in front of loops whose indices must become constants, or nothing
 *   VAD_NOUNROLL      a pragma in front of every other loop, or nothing: unrolled by trip counts
 *                     known only at run time, each keeps scalar registers busy all kernel long
 *
 * A stream's working memory `w` is int16 slots: its ssw_vad_state_t (as int16, the int32 members
 * as two slots, low half first), the narrow-band frame, the four band buffers of
 * WebRtcVad_CalculateFeatures, the frame's features.  No function keeps a per-sample array of
 * its own: on the device that would be scratch memory.
 *
 * Signed overflow the reference allows itself (RTC_NO_SANITIZE in resample_by_2_internal.c and
 * vad_core.c) and narrowing that wraps by design (AllPassFilter) are written in unsigned
 * arithmetic; every (int16_t) cast here is meant to wrap.  Left shifts of values that may be
 * negative are written as products.  (offsetof: the includer has <stddef.h>.) */
typedef int16_t *vad_w_t;
#define VW(w, i) ((w)[(size_t)(i) * SSW_VAD_PITCH])
#define VOFF(member) ((int)(offsetof(ssw_vad_state_t, member) / 2))

enum {
    VAD_STATE_SLOTS = (int)(sizeof(ssw_vad_state_t) / 2),
    VW_NB = VAD_STATE_SLOTS, /* the frame at 8 kHz: up to 240 samples */
    VW_HP120 = VW_NB + 240,  /* hp_120, lp_120, hp_60, lp_60 of vad_filterbank.c:250-251 */
    VW_LP120 = VW_HP120 + 120,
    VW_HP60 = VW_LP120 + 120,
    VW_LP60 = VW_HP60 + 60,
    VW_FEAT = VW_LP60 + 60,  /* features[6], total_energy, one spare */
    VW_SLOTS = VW_FEAT + 8,
    /* GmmProbability's deltaN, deltaS, ngprvec, sgprvec [12] each live in hp_120, which is free
     * once the features are made */
    VW_DELTAN = VW_HP120,
    VW_DELTAS = VW_HP120 + 12,
    VW_NGPR = VW_HP120 + 24,
    VW_SGPR = VW_HP120 + 36,
    VAD_MIN_ENERGY = 10 /* kMinEnergy, vad_core.h:23 */
};

VAD_FN int32_t vad_wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
VAD_FN int32_t vad_wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
VAD_FN int32_t vad_wmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
VAD_FN int16_t vad_s16(int32_t a) { return (int16_t)(uint16_t)(uint32_t)a; }

VAD_FN int32_t
vad_ld32(vad_w_t w, int i)
{
    return (int32_t)((uint32_t)(uint16_t)VW(w, i) | ((uint32_t)(uint16_t)VW(w, i + 1) << 16));
}
VAD_FN void
vad_st32(vad_w_t w, int i, int32_t v)
{
    VW(w, i) = vad_s16(v);
    VW(w, i + 1) = vad_s16((int32_t)((uint32_t)v >> 16));
}

/* WebRtcSpl_CountLeadingZeros32, NormW32, NormU32, GetSizeInBits (spl_inl.h:53-144) */
VAD_FN int
vad_clz(uint32_t n)
{
    return n == 0 ? 32 : __builtin_clz(n);
}
VAD_FN int vad_norm_w32(int32_t a) { return a == 0 ? 0 : vad_clz((uint32_t)(a < 0 ? ~a : a)) - 1; }
VAD_FN int vad_norm_u32(uint32_t a) { return a == 0 ? 0 : vad_clz(a); }
/* WebRtcSpl_DivW32W16 (division_operations.c:39-49): the divisor arrives as an int16 */
VAD_FN int32_t vad_div_w32_w16(int32_t num, int16_t den) { return den != 0 ? num / den : 0x7FFFFFFF; }

/* WebRtcVad_InitCore (vad_core.c:491-545) into a stream's slots */
VAD_FN void
vad_core_init(vad_w_t w)
{
    const int16_t nm[12] = { 6738, 4892, 7065, 6715, 6771, 3369, 7646, 3863, 7820, 7266, 5020, 4362 };
    const int16_t sm[12] = { 8306, 10085, 10078, 11823, 11843, 6309, 9473, 9571, 10879, 7581, 8180, 7483 };
    const int16_t ns[12] = { 378, 1064, 493, 582, 688, 593, 474, 697, 475, 688, 421, 455 };
    const int16_t ss[12] = { 555, 505, 567, 524, 585, 1231, 509, 828, 492, 1540, 1079, 850 };
    int i;
    VAD_NOUNROLL
    for (i = 0; i < VAD_STATE_SLOTS; ++i)
        VW(w, i) = 0;
    VAD_UNROLL
    for (i = 0; i < 12; ++i) {
        VW(w, VOFF(noise_means) + i) = nm[i];
        VW(w, VOFF(speech_means) + i) = sm[i];
        VW(w, VOFF(noise_stds) + i) = ns[i];
        VW(w, VOFF(speech_stds) + i) = ss[i];
    }
    VAD_NOUNROLL
    for (i = 0; i < 96; ++i)
        VW(w, VOFF(low_value_vector) + i) = 10000;
    VAD_NOUNROLL
    for (i = 0; i < 6; ++i)
        VW(w, VOFF(mean_value) + i) = 1600;
    VW(w, VOFF(initialised)) = 42;
}

/* ---- resampling to 8 kHz ------------------------------------------------------------------ */

/* WebRtcVad_Downsampling (vad_sp.c:25-53) over n input samples src[0 .. n), n even, filter state
 * at slots st, st + 2 (int32 each); n / 2 samples to slots dst ... */
VAD_FN void
vad_down2(vad_w_t w, int st, const vad_w_t src, int n, int dst)
{
    int32_t s1 = vad_ld32(w, st), s2 = vad_ld32(w, st + 2);
    int i;
    VAD_NOUNROLL
    for (i = 0; i < n / 2; ++i) {
        const int32_t x0 = VW(src, 2 * i), x1 = VW(src, 2 * i + 1);
        const int16_t t1 = vad_s16((s1 >> 1) + ((5243 * x0) >> 14));
        int16_t t2;
        s1 = x0 - ((5243 * t1) >> 12);
        t2 = vad_s16((s2 >> 1) + ((1392 * x1) >> 14));
        VW(w, dst + i) = vad_s16(t1 + t2);
        s2 = x1 - ((1392 * t2) >> 12);
    }
    vad_st32(w, st, s1);
    vad_st32(w, st + 2, s2);
}

/* WebRtcVad_CalcVad32khz's two cascaded calls (vad_core.c:632-653) as one pass: four inputs ->
 * one output; the 32 -> 16 stage uses states [2..3], the 16 -> 8 stage [0..1] */
VAD_FN void
vad_down4(vad_w_t w, const vad_w_t src, int n, int dst)
{
    int32_t a1 = vad_ld32(w, VOFF(downsampling_filter_states) + 4);
    int32_t a2 = vad_ld32(w, VOFF(downsampling_filter_states) + 6);
    int32_t b1 = vad_ld32(w, VOFF(downsampling_filter_states) + 0);
    int32_t b2 = vad_ld32(w, VOFF(downsampling_filter_states) + 2);
    int i, h;
    VAD_NOUNROLL
    for (i = 0; i < n / 4; ++i) {
        int32_t y[2];
        int16_t t1, t2;
        VAD_UNROLL
        for (h = 0; h < 2; ++h) {
            const int32_t x0 = VW(src, 4 * i + 2 * h), x1 = VW(src, 4 * i + 2 * h + 1);
            t1 = vad_s16((a1 >> 1) + ((5243 * x0) >> 14));
            a1 = x0 - ((5243 * t1) >> 12);
            t2 = vad_s16((a2 >> 1) + ((1392 * x1) >> 14));
            a2 = x1 - ((1392 * t2) >> 12);
            y[h] = vad_s16(t1 + t2);
        }
        t1 = vad_s16((b1 >> 1) + ((5243 * y[0]) >> 14));
        b1 = y[0] - ((5243 * t1) >> 12);
        t2 = vad_s16((b2 >> 1) + ((1392 * y[1]) >> 14));
        b2 = y[1] - ((1392 * t2) >> 12);
        VW(w, dst + i) = vad_s16(t1 + t2);
    }
    vad_st32(w, VOFF(downsampling_filter_states) + 4, a1);
    vad_st32(w, VOFF(downsampling_filter_states) + 6, a2);
    vad_st32(w, VOFF(downsampling_filter_states) + 0, b1);
    vad_st32(w, VOFF(downsampling_filter_states) + 2, b2);
}

/* one sample through the three all-pass sections every filter of resample_by_2_internal.c is
 * made of (e.g. :142-166): s[0..3] the sections' states, c their coefficients; returns s[3] */
VAD_FN int32_t
vad_ap3(int32_t in, int32_t *s, int c0, int c1, int c2)
{
    int32_t diff, t0, t1;
    diff = vad_wadd(vad_wsub(in, s[1]), 1 << 13) >> 14;
    t1 = vad_wadd(s[0], vad_wmul(diff, c0));
    s[0] = in;
    diff = vad_wsub(t1, s[2]) >> 14;
    if (diff < 0)
        diff += 1;
    t0 = vad_wadd(s[1], vad_wmul(diff, c1));
    s[1] = t1;
    diff = vad_wsub(t0, s[3]) >> 14;
    if (diff < 0)
        diff += 1;
    s[3] = vad_wadd(s[2], vad_wmul(diff, c2));
    s[2] = t0;
    return s[3];
}
/* kResampleAllpass[1] ("lower") and [0] ("upper"), resample_by_2_internal.c:21-24 */
#define VAD_AP_LO(in, s) vad_ap3(in, s, 3050, 9368, 15063)
#define VAD_AP_UP(in, s) vad_ap3(in, s, 821, 6110, 12382)

VAD_FN int32_t
vad_fir8(const int32_t *in, int c0, int c1, int c2, int c3, int c4, int c5, int c6, int c7)
{
    int32_t t = 1 << 14;
    t = vad_wadd(t, vad_wmul(c0, in[0]));
    t = vad_wadd(t, vad_wmul(c1, in[1]));
    t = vad_wadd(t, vad_wmul(c2, in[2]));
    t = vad_wadd(t, vad_wmul(c3, in[3]));
    t = vad_wadd(t, vad_wmul(c4, in[4]));
    t = vad_wadd(t, vad_wmul(c5, in[5]));
    t = vad_wadd(t, vad_wmul(c6, in[6]));
    t = vad_wadd(t, vad_wmul(c7, in[7]));
    return t;
}

/* WebRtcSpl_Resample48khzTo8khz (resample_48khz.c:103-132) as one pass over n input samples,
 * n a multiple of 12: twelve samples at 48 kHz -> six at 24 (WebRtcSpl_DownBy2ShortToInt,
 * resample_by_2_internal.c:128-200) -> six low-passed (WebRtcSpl_LPBy2IntToInt, :559-689) -> four
 * at 16 (WebRtcSpl_Resample48khzTo32khz, resample_fractional.c:44-82, whose eight samples of
 * history are S_24_16) -> two at 8 (WebRtcSpl_DownBy2IntToShort, :32-120).  The reference runs
 * each stage over the whole 10 ms block; the stages' filters share no state, so sample by sample
 * gives the same numbers.  The one coupling is LPBy2IntToInt's delay element: its first filter
 * reads state[12], the odd input its fourth filter stored a pair earlier -- so per pair the first
 * filter runs before the fourth.  A block of 480 is 40 groups, and 240 low-passed samples are a
 * multiple of 3, so the interpolator's phase carries over from call to call. */
VAD_FN void
vad_down48(vad_w_t w, const vad_w_t src, int n, int dst)
{
    int32_t s1[8], s2[16], s3[8], s4[8];
    int i, g;
    VAD_UNROLL
    for (i = 0; i < 8; ++i) {
        s1[i] = vad_ld32(w, VOFF(s_48_24) + 2 * i);
        s3[i] = vad_ld32(w, VOFF(s_24_16) + 2 * i);
        s4[i] = vad_ld32(w, VOFF(s_16_8) + 2 * i);
    }
    VAD_UNROLL
    for (i = 0; i < 16; ++i)
        s2[i] = vad_ld32(w, VOFF(s_24_24) + 2 * i);
    VAD_NOUNROLL
    for (g = 0; g < n / 12; ++g) {
        int32_t in[14], o[4];
        VAD_UNROLL
        for (i = 0; i < 8; ++i)
            in[i] = s3[i];
        VAD_UNROLL
        for (i = 0; i < 3; ++i) {
            int32_t y[2], e, od;
            int h;
            VAD_UNROLL
            for (h = 0; h < 2; ++h) {
                const int32_t x0 = VW(src, 12 * g + 4 * i + 2 * h);
                const int32_t x1 = VW(src, 12 * g + 4 * i + 2 * h + 1);
                const int32_t lo = VAD_AP_LO(x0 * 32768 + 16384, s1) >> 1;
                const int32_t up = VAD_AP_UP(x1 * 32768 + 16384, s1 + 4) >> 1;
                y[h] = vad_wadd(lo, up);
            }
            /* the pair (y[0], y[1]) at 24 kHz through the half-band low-pass */
            e = VAD_AP_LO(s2[12], s2) >> 1;
            in[8 + 2 * i] = vad_wadd(e, VAD_AP_UP(y[0], s2 + 4) >> 1) >> 15;
            od = VAD_AP_LO(y[0], s2 + 8) >> 1;
            in[8 + 2 * i + 1] = vad_wadd(od, VAD_AP_UP(y[1], s2 + 12) >> 1) >> 15;
        }
        /* kCoefficients48To32 (resample_fractional.c:21-24): two blocks of 3 in, 2 out */
        o[0] = vad_fir8(in + 0, 778, -2050, 1087, 23285, 12903, -3783, 441, 222);
        o[1] = vad_fir8(in + 1, 222, 441, -3783, 12903, 23285, 1087, -2050, 778);
        o[2] = vad_fir8(in + 3, 778, -2050, 1087, 23285, 12903, -3783, 441, 222);
        o[3] = vad_fir8(in + 4, 222, 441, -3783, 12903, 23285, 1087, -2050, 778);
        VAD_UNROLL
        for (i = 0; i < 8; ++i)
            s3[i] = in[6 + i];
        VAD_UNROLL
        for (i = 0; i < 2; ++i) {
            const int32_t lo = VAD_AP_LO(o[2 * i], s4) >> 1;
            const int32_t up = VAD_AP_UP(o[2 * i + 1], s4 + 4) >> 1;
            int32_t t = vad_wadd(lo, up) >> 15;
            t = t > 32767 ? 32767 : t < -32768 ? -32768 : t;
            VW(w, dst + 2 * g + i) = (int16_t)t;
        }
    }
    VAD_UNROLL
    for (i = 0; i < 8; ++i) {
        vad_st32(w, VOFF(s_48_24) + 2 * i, s1[i]);
        vad_st32(w, VOFF(s_24_16) + 2 * i, s3[i]);
        vad_st32(w, VOFF(s_16_8) + 2 * i, s4[i]);
    }
    VAD_UNROLL
    for (i = 0; i < 16; ++i)
        vad_st32(w, VOFF(s_24_24) + 2 * i, s2[i]);
}

/* n samples of the caller's audio at the detector's rate -> samples of the narrow-band frame
 * from slot VW_NB + nb_pos on; n is a multiple of 1, 2, 4 or 12 by rate.  Returns how many. */
VAD_FN int
vad_ingest(vad_w_t w, int rate, const vad_w_t src, int n, int nb_pos)
{
    int i;
    if (rate == 8000) {
        VAD_NOUNROLL
        for (i = 0; i < n; ++i)
            VW(w, VW_NB + nb_pos + i) = VW(src, i);
        return n;
    }
    if (rate == 16000) { /* WebRtcVad_CalcVad16khz, vad_core.c:655-670 */
        vad_down2(w, VOFF(downsampling_filter_states), src, n, VW_NB + nb_pos);
        return n / 2;
    }
    if (rate == 32000) {
        vad_down4(w, src, n, VW_NB + nb_pos);
        return n / 4;
    }
    vad_down48(w, src, n, VW_NB + nb_pos);
    return n / 6;
}

/* ---- features (vad_filterbank.c) ------------------------------------------------------------ */

/* AllPassFilter (vad_filterbank.c:81-105): every second sample of slots in ... -> n samples */
VAD_FN void
vad_allpass(vad_w_t w, int in, int n, int coef, int st, int out)
{
    int32_t state32 = (int32_t)VW(w, st) * 65536;
    int i;
    VAD_NOUNROLL
    for (i = 0; i < n; ++i) {
        const int32_t x = VW(w, in + 2 * i);
        const int16_t t16 = vad_s16(vad_wadd(state32, coef * x) >> 16);
        VW(w, out + i) = t16;
        state32 = vad_wmul(vad_wsub(x * 16384, coef * t16), 2);
    }
    VW(w, st) = vad_s16(state32 >> 16);
}

/* SplitFilter (vad_filterbank.c:118-139); kAllPassCoefsQ15 = { 20972, 5571 } */
VAD_FN void
vad_split(vad_w_t w, int in, int n, int band, int hp, int lp)
{
    const int half = n >> 1;
    int i;
    vad_allpass(w, in, half, 20972, VOFF(upper_state) + band, hp);
    vad_allpass(w, in + 1, half, 5571, VOFF(lower_state) + band, lp);
    VAD_NOUNROLL
    for (i = 0; i < half; ++i) {
        const int16_t h = VW(w, hp + i), l = VW(w, lp + i);
        VW(w, hp + i) = vad_s16(h - l);
        VW(w, lp + i) = vad_s16(l + h);
    }
}

/* HighPassFilter (vad_filterbank.c:39-70) */
VAD_FN void
vad_highpass(vad_w_t w, int in, int n, int out)
{
    int16_t f0 = VW(w, VOFF(hp_filter_state) + 0), f1 = VW(w, VOFF(hp_filter_state) + 1);
    int16_t f2 = VW(w, VOFF(hp_filter_state) + 2), f3 = VW(w, VOFF(hp_filter_state) + 3);
    int i;
    VAD_NOUNROLL
    for (i = 0; i < n; ++i) {
        const int16_t x = VW(w, in + i);
        int32_t t = 6631 * x;
        t += -13262 * f0;
        t += 6631 * f1;
        f1 = f0;
        f0 = x;
        t -= -7756 * f2;
        t -= 5620 * f3;
        f3 = f2;
        f2 = vad_s16(t >> 14);
        VW(w, out + i) = f2;
    }
    VW(w, VOFF(hp_filter_state) + 0) = f0;
    VW(w, VOFF(hp_filter_state) + 1) = f1;
    VW(w, VOFF(hp_filter_state) + 2) = f2;
    VW(w, VOFF(hp_filter_state) + 3) = f3;
}

/* LogOfEnergy (vad_filterbank.c:152-241) over WebRtcSpl_Energy (energy.c:20-39) and
 * WebRtcSpl_GetScalingSquare (get_scaling_square.c:20-46): the band is read twice, because every
 * square is shifted by a scaling taken from the band's maximum BEFORE it is summed */
VAD_FN void
vad_log_energy(vad_w_t w, int in, int n, int offset, int16_t *total_energy, int feat)
{
    int16_t smax = -1, log_energy;
    int nbits = 32 - vad_clz((uint32_t)n), t, scaling, tot_rshifts, i;
    uint32_t energy = 0;
    VAD_NOUNROLL
    for (i = 0; i < n; ++i) {
        const int16_t v = VW(w, in + i);
        const int16_t sabs = v > 0 ? v : vad_s16(-(int32_t)v);
        smax = sabs > smax ? sabs : smax;
    }
    t = vad_norm_w32((int32_t)smax * smax);
    scaling = smax == 0 ? 0 : t > nbits ? 0 : nbits - t;
    VAD_NOUNROLL
    for (i = 0; i < n; ++i) {
        const int32_t v = VW(w, in + i);
        energy += (uint32_t)((v * v) >> scaling);
    }
    tot_rshifts = scaling;
    if (energy == 0) {
        VW(w, feat) = (int16_t)offset;
        return;
    }
    {
        const int normalizing_rshifts = 17 - vad_norm_u32(energy);
        int32_t log2_energy = 14336; /* kLogEnergyIntPart */
        tot_rshifts += normalizing_rshifts;
        if (normalizing_rshifts < 0)
            energy <<= -normalizing_rshifts;
        else
            energy >>= normalizing_rshifts;
        log2_energy = vad_s16(log2_energy + (int16_t)((energy & 0x00003FFF) >> 4));
        /* kLogConst = 24660 */
        log_energy = vad_s16(((24660 * log2_energy) >> 19) + ((tot_rshifts * 24660) >> 9));
        if (log_energy < 0)
            log_energy = 0;
    }
    VW(w, feat) = vad_s16(log_energy + offset);
    if (*total_energy <= VAD_MIN_ENERGY) {
        if (tot_rshifts >= 0)
            *total_energy = vad_s16(*total_energy + VAD_MIN_ENERGY + 1);
        else
            *total_energy = vad_s16(*total_energy + (int16_t)(energy >> -tot_rshifts));
    }
}

/* WebRtcVad_CalculateFeatures (vad_filterbank.c:243-329) over the n samples at VW_NB: features to
 * VW_FEAT + 0..5, total_energy to VW_FEAT + 6 and returned; kOffsetVector = 368 368 272 176 176 176 */
VAD_FN int16_t
vad_features(vad_w_t w, int n)
{
    int16_t total = 0;
    const int half = n >> 1;
    vad_split(w, VW_NB, n, 0, VW_HP120, VW_LP120);
    vad_split(w, VW_HP120, half, 1, VW_HP60, VW_LP60);
    vad_log_energy(w, VW_HP60, half >> 1, 176, &total, VW_FEAT + 5);
    vad_log_energy(w, VW_LP60, half >> 1, 176, &total, VW_FEAT + 4);
    vad_split(w, VW_LP120, half, 2, VW_HP60, VW_LP60);
    vad_log_energy(w, VW_HP60, half >> 1, 176, &total, VW_FEAT + 3);
    vad_split(w, VW_LP60, half >> 1, 3, VW_HP120, VW_LP120);
    vad_log_energy(w, VW_HP120, half >> 2, 272, &total, VW_FEAT + 2);
    vad_split(w, VW_LP120, half >> 2, 4, VW_HP60, VW_LP60);
    vad_log_energy(w, VW_HP60, half >> 3, 368, &total, VW_FEAT + 1);
    vad_highpass(w, VW_LP60, half >> 3, VW_HP120);
    vad_log_energy(w, VW_HP120, half >> 3, 368, &total, VW_FEAT + 0);
    VW(w, VW_FEAT + 6) = total;
    return total;
}

/* ---- the decision (vad_gmm.c, vad_sp.c, vad_core.c) ----------------------------------------- */

/* WebRtcVad_GaussianProbability (vad_gmm.c:29-82) */
VAD_FN int32_t
vad_gaussian(int16_t input, int16_t mean, int16_t std, int16_t *delta)
{
    int16_t t16, inv_std, inv_std2, exp_value = 0;
    int32_t t32;
    t32 = 131072 + (std >> 1);
    inv_std = vad_s16(vad_div_w32_w16(t32, std));
    t16 = inv_std >> 2;
    inv_std2 = vad_s16((t16 * t16) >> 2);
    t16 = vad_s16(input * 8);
    t16 = vad_s16(t16 - mean);
    *delta = vad_s16((inv_std2 * t16) >> 10);
    t32 = (*delta * t16) >> 9;
    if (t32 < 22005) { /* kCompVar */
        t16 = vad_s16((5909 * t32) >> 12); /* kLog2Exp */
        t16 = vad_s16(-(int32_t)t16);
        exp_value = vad_s16(0x0400 | (t16 & 0x03FF));
        t16 = vad_s16(t16 ^ 0xFFFF);
        t16 >>= 10;
        t16 = vad_s16(t16 + 1);
        exp_value = vad_s16(exp_value >> t16);
    }
    return inv_std * exp_value;
}

/* WebRtcVad_FindMinimum (vad_sp.c:58-176) */
VAD_FN int16_t
vad_find_minimum(vad_w_t w, int16_t feature_value, int channel)
{
    const int age = VOFF(index_vector) + (channel << 4);
    const int val = VOFF(low_value_vector) + (channel << 4);
    const int32_t frame_counter = vad_ld32(w, VOFF(frame_counter));
    int i, j, position = -1;
    int16_t current_median = 1600, alpha = 0, mean;
    int32_t t32;
    VAD_NOUNROLL
    for (i = 0; i < 16; ++i) {
        if (VW(w, age + i) != 100) {
            VW(w, age + i) = vad_s16(VW(w, age + i) + 1);
        } else {
            VAD_NOUNROLL
            for (j = i; j < 15; ++j) {
                VW(w, val + j) = VW(w, val + j + 1);
                VW(w, age + j) = VW(w, age + j + 1);
            }
            VW(w, age + 15) = 101;
            VW(w, val + 15) = 10000;
        }
    }
    /* the reference's tree of comparisons (vad_sp.c:94-142): compare with slot base + step - 1
     * and halve the step, which is that tree for any contents, sorted or not */
    if (feature_value < VW(w, val + 7) || feature_value < VW(w, val + 15)) {
        int base = 0, step;
        VAD_NOUNROLL
        for (step = 8; step >= 1; step >>= 1)
            if (!(feature_value < VW(w, val + base + step - 1)))
                base += step;
        position = base;
    }
    if (position > -1) {
        VAD_NOUNROLL
        for (i = 15; i > position; --i) {
            VW(w, val + i) = VW(w, val + i - 1);
            VW(w, age + i) = VW(w, age + i - 1);
        }
        VW(w, val + position) = feature_value;
        VW(w, age + position) = 1;
    }
    if (frame_counter > 2)
        current_median = VW(w, val + 2);
    else if (frame_counter > 0)
        current_median = VW(w, val + 0);
    mean = VW(w, VOFF(mean_value) + channel);
    if (frame_counter > 0)
        alpha = current_median < mean ? 6553 : 32439; /* kSmoothingDown, kSmoothingUp */
    t32 = (alpha + 1) * mean;
    t32 += (32767 - alpha) * current_median;
    t32 += 16384;
    mean = vad_s16(t32 >> 15);
    VW(w, VOFF(mean_value) + channel) = mean;
    return mean;
}

/* WeightedAverage (vad_core.c:101-111) over the two Gaussians of a channel; w0, w1 the weights */
VAD_FN int32_t
vad_weighted_average(vad_w_t w, int data, int16_t offset, int w0, int w1)
{
    int32_t avg;
    VW(w, data) = vad_s16(VW(w, data) + offset);
    avg = VW(w, data) * w0;
    VW(w, data + 6) = vad_s16(VW(w, data + 6) + offset);
    avg += VW(w, data + 6) * w1;
    return avg;
}

/* the mode's thresholds at the frame length in use (WebRtcVad_set_mode_core, vad_core.c:548-602;
 * GmmProbability's choice by frame length, :157-173) */
typedef struct vad_thresholds_s {
    int16_t overhead1, overhead2, individual, total;
} vad_thresholds_t;

VAD_FN int16_t
vad_tab(int which, int i)
{
    /* kNoiseDataWeights, kSpeechDataWeights [12]; kSpectrumWeight, kMinimumDifference,
     * kMaximumSpeech, kMaximumNoise [6] (vad_core.c:20-41), as one switch so that no table
     * has to live in device memory */
    const int16_t nw[12] = { 34, 62, 72, 66, 53, 25, 94, 66, 56, 62, 75, 103 };
    const int16_t sw[12] = { 48, 82, 45, 87, 50, 47, 80, 46, 83, 41, 78, 81 };
    const int16_t md[6] = { 544, 544, 576, 576, 576, 576 };
    const int16_t ms[6] = { 11392, 11392, 11520, 11520, 11520, 11520 };
    const int16_t mn[6] = { 9216, 9088, 8960, 8832, 8704, 8576 };
    switch (which) {
    case 0: return nw[i];
    case 1: return sw[i];
    case 2: return (int16_t)(6 + 2 * i);
    case 3: return md[i];
    case 4: return ms[i];
    default: return mn[i];
    }
}

/* GmmProbability (vad_core.c:133-488) on the features at VW_FEAT; returns its vadflag (0, 1, or
 * 2 + over_hang during the hang-over) */
VAD_FN int16_t
vad_gmm(vad_w_t w, int16_t total_power, const vad_thresholds_t th)
{
    int16_t vadflag = 0;
    int channel, k;
    if (total_power > VAD_MIN_ENERGY) {
        int32_t sum_llr = 0;
        int16_t maxspe = 12800;
        VAD_NOUNROLL
        for (channel = 0; channel < 6; ++channel) {
            const int16_t feat = VW(w, VW_FEAT + channel);
            int32_t h0_test = 0, h1_test = 0, np0 = 0, sp0 = 0;
            int16_t shifts_h0, shifts_h1, llr, h0, h1, d;
            VW(w, VW_NGPR + channel) = 0;
            VW(w, VW_NGPR + channel + 6) = 0;
            VW(w, VW_SGPR + channel) = 0;
            VW(w, VW_SGPR + channel + 6) = 0;
            VAD_UNROLL
            for (k = 0; k < 2; ++k) {
                const int g = channel + k * 6;
                int32_t p;
                p = vad_tab(0, g) * vad_gaussian(feat, VW(w, VOFF(noise_means) + g),
                                                 VW(w, VOFF(noise_stds) + g), &d);
                VW(w, VW_DELTAN + g) = d;
                if (k == 0)
                    np0 = p;
                h0_test += p;
                p = vad_tab(1, g) * vad_gaussian(feat, VW(w, VOFF(speech_means) + g),
                                                 VW(w, VOFF(speech_stds) + g), &d);
                VW(w, VW_DELTAS + g) = d;
                if (k == 0)
                    sp0 = p;
                h1_test += p;
            }
            shifts_h0 = (int16_t)(h0_test == 0 ? 31 : vad_norm_w32(h0_test));
            shifts_h1 = (int16_t)(h1_test == 0 ? 31 : vad_norm_w32(h1_test));
            llr = (int16_t)(shifts_h0 - shifts_h1);
            sum_llr += llr * vad_tab(2, channel);
            if (llr * 4 > th.individual)
                vadflag = 1;
            h0 = vad_s16(h0_test >> 12);
            if (h0 > 0) {
                const int32_t t = (int32_t)(((uint32_t)np0 & 0xFFFFF000u) << 2);
                const int16_t n0 = vad_s16(vad_div_w32_w16(t, h0));
                VW(w, VW_NGPR + channel) = n0;
                VW(w, VW_NGPR + channel + 6) = vad_s16(16384 - n0);
            } else {
                VW(w, VW_NGPR + channel) = 16384;
            }
            h1 = vad_s16(h1_test >> 12);
            if (h1 > 0) {
                const int32_t t = (int32_t)(((uint32_t)sp0 & 0xFFFFF000u) << 2);
                const int16_t s0 = vad_s16(vad_div_w32_w16(t, h1));
                VW(w, VW_SGPR + channel) = s0;
                VW(w, VW_SGPR + channel + 6) = vad_s16(16384 - s0);
            }
        }
        vadflag |= (sum_llr >= th.total);

        VAD_NOUNROLL
        for (channel = 0; channel < 6; ++channel) {
            const int16_t feat = VW(w, VW_FEAT + channel);
            const int nmo = VOFF(noise_means) + channel, smo = VOFF(speech_means) + channel;
            const int nw0 = vad_tab(0, channel), nw1 = vad_tab(0, channel + 6);
            const int sw0 = vad_tab(1, channel), sw1 = vad_tab(1, channel + 6);
            const int16_t feature_minimum = vad_find_minimum(w, feat, channel);
            int32_t noise_global_mean = vad_weighted_average(w, nmo, 0, nw0, nw1);
            int32_t speech_global_mean;
            int16_t tmp1_s16 = vad_s16(noise_global_mean >> 6), tmp2_s16, tmp_s16, diff;
            VAD_UNROLL
            for (k = 0; k < 2; ++k) {
                const int g = channel + k * 6;
                const int16_t nmk = VW(w, VOFF(noise_means) + g);
                const int16_t smk = VW(w, VOFF(speech_means) + g);
                int16_t nsk = VW(w, VOFF(noise_stds) + g), ssk = VW(w, VOFF(speech_stds) + g);
                const int16_t deltaN = VW(w, VW_DELTAN + g), deltaS = VW(w, VW_DELTAS + g);
                const int16_t ngpr = VW(w, VW_NGPR + g), sgpr = VW(w, VW_SGPR + g);
                int16_t nmk2 = nmk, nmk3, delt, ndelt, smk2, maxmu;
                int32_t tmp1_s32, tmp2_s32;
                if (!vadflag) {
                    delt = vad_s16((ngpr * deltaN) >> 11);
                    nmk2 = vad_s16(nmk + (int16_t)((delt * 655) >> 22)); /* kNoiseUpdateConst */
                }
                ndelt = vad_s16(feature_minimum * 16 - tmp1_s16);
                nmk3 = vad_s16(nmk2 + (int16_t)((ndelt * 154) >> 9)); /* kBackEta */
                tmp_s16 = (int16_t)((k + 5) << 7);
                if (nmk3 < tmp_s16)
                    nmk3 = tmp_s16;
                tmp_s16 = (int16_t)((72 + k - channel) << 7);
                if (nmk3 > tmp_s16)
                    nmk3 = tmp_s16;
                VW(w, VOFF(noise_means) + g) = nmk3;
                if (vadflag) {
                    const int16_t min_mean = k == 0 ? 640 : 768; /* kMinimumMean */
                    delt = vad_s16((sgpr * deltaS) >> 11);
                    tmp_s16 = vad_s16((delt * 6554) >> 21); /* kSpeechUpdateConst */
                    smk2 = vad_s16(smk + ((tmp_s16 + 1) >> 1));
                    maxmu = vad_s16(maxspe + 640);
                    if (smk2 < min_mean)
                        smk2 = min_mean;
                    if (smk2 > maxmu)
                        smk2 = maxmu;
                    VW(w, VOFF(speech_means) + g) = smk2;
                    tmp_s16 = vad_s16((smk + 4) >> 3);
                    tmp_s16 = vad_s16(feat - tmp_s16);
                    tmp1_s32 = (deltaS * tmp_s16) >> 3;
                    tmp2_s32 = tmp1_s32 - 4096;
                    tmp_s16 = sgpr >> 2;
                    tmp1_s32 = vad_wmul(tmp_s16, tmp2_s32);
                    tmp2_s32 = tmp1_s32 >> 4;
                    if (tmp2_s32 > 0) {
                        tmp_s16 = vad_s16(vad_div_w32_w16(tmp2_s32, vad_s16(ssk * 10)));
                    } else {
                        tmp_s16 = vad_s16(vad_div_w32_w16(vad_wsub(0, tmp2_s32), vad_s16(ssk * 10)));
                        tmp_s16 = vad_s16(-(int32_t)tmp_s16);
                    }
                    tmp_s16 = vad_s16(tmp_s16 + 128);
                    ssk = vad_s16(ssk + (tmp_s16 >> 8));
                    if (ssk < 384) /* kMinStd */
                        ssk = 384;
                    VW(w, VOFF(speech_stds) + g) = ssk;
                } else {
                    tmp_s16 = vad_s16(feat - (nmk >> 3));
                    tmp1_s32 = (deltaN * tmp_s16) >> 3;
                    tmp1_s32 -= 4096;
                    tmp_s16 = vad_s16((ngpr + 2) >> 2);
                    /* OverflowingMulS16ByS32ToS32 (vad_core.c:117-120): it wraps */
                    tmp2_s32 = vad_wmul(tmp_s16, tmp1_s32);
                    tmp1_s32 = tmp2_s32 >> 14;
                    if (tmp1_s32 > 0) {
                        tmp_s16 = vad_s16(vad_div_w32_w16(tmp1_s32, nsk));
                    } else {
                        tmp_s16 = vad_s16(vad_div_w32_w16(vad_wsub(0, tmp1_s32), nsk));
                        tmp_s16 = vad_s16(-(int32_t)tmp_s16);
                    }
                    tmp_s16 = vad_s16(tmp_s16 + 32);
                    nsk = vad_s16(nsk + (tmp_s16 >> 6));
                    if (nsk < 384)
                        nsk = 384;
                    VW(w, VOFF(noise_stds) + g) = nsk;
                }
            }
            noise_global_mean = vad_weighted_average(w, nmo, 0, nw0, nw1);
            speech_global_mean = vad_weighted_average(w, smo, 0, sw0, sw1);
            diff = vad_s16((int16_t)(speech_global_mean >> 9) - (int16_t)(noise_global_mean >> 9));
            if (diff < vad_tab(3, channel)) {
                tmp_s16 = vad_s16(vad_tab(3, channel) - diff);
                tmp1_s16 = vad_s16((13 * tmp_s16) >> 2);
                tmp2_s16 = vad_s16((3 * tmp_s16) >> 2);
                speech_global_mean = vad_weighted_average(w, smo, tmp1_s16, sw0, sw1);
                noise_global_mean = vad_weighted_average(w, nmo, vad_s16(-(int32_t)tmp2_s16), nw0, nw1);
            }
            maxspe = vad_tab(4, channel);
            tmp2_s16 = vad_s16(speech_global_mean >> 7);
            if (tmp2_s16 > maxspe) {
                tmp2_s16 = vad_s16(tmp2_s16 - maxspe);
                VW(w, smo) = vad_s16(VW(w, smo) - tmp2_s16);
                VW(w, smo + 6) = vad_s16(VW(w, smo + 6) - tmp2_s16);
            }
            tmp2_s16 = vad_s16(noise_global_mean >> 7);
            if (tmp2_s16 > vad_tab(5, channel)) {
                tmp2_s16 = vad_s16(tmp2_s16 - vad_tab(5, channel));
                VW(w, nmo) = vad_s16(VW(w, nmo) - tmp2_s16);
                VW(w, nmo + 6) = vad_s16(VW(w, nmo + 6) - tmp2_s16);
            }
        }
        vad_st32(w, VOFF(frame_counter), vad_wadd(vad_ld32(w, VOFF(frame_counter)), 1));
    }
    /* the hang-over (vad_core.c:471-486) */
    if (!vadflag) {
        const int16_t oh = VW(w, VOFF(over_hang));
        if (oh > 0) {
            vadflag = vad_s16(2 + oh);
            VW(w, VOFF(over_hang)) = vad_s16(oh - 1);
        }
        VW(w, VOFF(num_of_speech)) = 0;
    } else {
        const int16_t ns = vad_s16(VW(w, VOFF(num_of_speech)) + 1);
        if (ns > 6) { /* kMaxSpeechFrames */
            VW(w, VOFF(num_of_speech)) = 6;
            VW(w, VOFF(over_hang)) = th.overhead2;
        } else {
            VW(w, VOFF(num_of_speech)) = ns;
            VW(w, VOFF(over_hang)) = th.overhead1;
        }
    }
    return vadflag;
}

/* WebRtcVad_CalcVad8khz (vad_core.c:672-685) on the n narrow-band samples at VW_NB, then
 * WebRtcVad_Process's squashing (webrtc_vad.c:86-88): what vad_classify returns */
VAD_FN int
vad_decide(vad_w_t w, int n, const vad_thresholds_t th)
{
    const int16_t total = vad_features(w, n);
    return vad_gmm(w, total, th) > 0 ? 1 : 0;
}
