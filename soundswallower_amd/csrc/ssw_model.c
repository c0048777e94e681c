/*
 * ssw_model.c -- host-side model loading for the MI355X acoustic path (plain C).
 *
 * Reads the Sphinx-3 binary model files and derives every table exactly as SoundSwallower
 * derives it at load time (file:line citations are relative to the SoundSwallower tree):
 *   s3 container, byte order, checksum   src/s3file.c:210-327, 366-445, 551-570
 *   means / variances + precompute       src/ms_gauden.c:105-202, 217-258
 *   sendump / mixture_weights            src/ptm_mgau.c:456-692, src/ms_senone.c:103-198
 *   transition matrices                  src/tmat.c:125-227
 *   binary mdef                          src/bin_mdef.c:333-540
 *   integer log tables                   src/logmath.c:60-164, 282-301
 * Load-time arithmetic is double precision libm (log, sqrt) followed by integer truncation,
 * as in the reference; the results are data for the kernels.
 */
#include "ssw_internal.h"

#include <ctype.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static __thread char tls_err[512];

void
ssw_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tls_err, sizeof(tls_err), fmt, ap);
    va_end(ap);
}

const char *
ssw_last_error(void)
{
    return tls_err;
}

int
ssw_abi_version(void)
{
    return SSW_ABI_VERSION;
}

void
ssw_config_defaults(ssw_config_t *cfg)
{
    cfg->logbase = 1.0001;
    cfg->varfloor = 1e-4;
    cfg->mixwfloor = 1e-7;
    cfg->tmatfloor = 1e-4;
    cfg->topn = 4;
    cfg->ds = 1;
    cfg->aw = 1;
    cfg->device = -1;
}

/* ---------------------------------------------------------------------------------- */
/* Front-end settings: feat_params.json, read the way config_parse_json reads it         */
/* (src/config.c:441-510: a flat JSON object, every value a string or a primitive), over */
/* the defaults of config_defs.h FE_OPTIONS (include/soundswallower/config_defs.h:       */
/* 299-412).                                                                             */
/* ---------------------------------------------------------------------------------- */
void
ssw_fe_config_defaults(ssw_fe_config_t *c)
{
    memset(c, 0, sizeof(*c));
    c->samprate = 16000;
    c->wlen = 0.025625;
    c->alpha = 0.97;
    c->lowerf = 133.33334;
    c->upperf = 6855.4976;
    c->frate = 100;
    c->nfft = 0;
    c->ncep = 13;
    c->nfilt = 40;
    c->lifter = 0;
    c->transform = SSW_FE_LEGACY;
    c->remove_noise = 0;
    c->unit_area = 1;
    c->round_filters = 1;
}

/* ---------------------------------------------------------------------------------- */
/* feat_params.json                                                                     */
/* ---------------------------------------------------------------------------------- */
/* one JSON token: a string (unescaped into out) or a primitive (number, true, false, null);
 * returns the position after it, NULL on a syntax error */
static const char *
json_token(const char *p, char *out, size_t cap, int *is_string)
{
    size_t n = 0;
    while (isspace((unsigned char)*p))
        ++p;
    if (*p == '"') {
        *is_string = 1;
        for (++p; *p && *p != '"'; ++p) {
            char ch = *p;
            if (ch == '\\') {
                ++p;
                switch (*p) {
                case 'n': ch = '\n'; break;
                case 't': ch = '\t'; break;
                case 'r': ch = '\r'; break;
                case 'b': ch = '\b'; break;
                case 'f': ch = '\f'; break;
                case '\0': return NULL;
                default: ch = *p; break; /* \" \\ \/ (\uXXXX is not needed by any key here) */
                }
            }
            if (n + 1 < cap)
                out[n++] = ch;
        }
        if (*p != '"')
            return NULL;
        out[n] = '\0';
        return p + 1;
    }
    *is_string = 0;
    while (*p && *p != ',' && *p != '}' && !isspace((unsigned char)*p)) {
        if (n + 1 < cap)
            out[n++] = *p;
        ++p;
    }
    out[n] = '\0';
    return n ? p : NULL;
}

static int
parse_bool(const char *v, int32_t *out)
{
    if (!strcmp(v, "true") || !strcmp(v, "yes") || !strcmp(v, "1") || !strcmp(v, "TRUE")
        || !strcmp(v, "YES"))
        *out = 1;
    else if (!strcmp(v, "false") || !strcmp(v, "no") || !strcmp(v, "0") || !strcmp(v, "FALSE")
             || !strcmp(v, "NO"))
        *out = 0;
    else
        return -1;
    return 0;
}

static int
parse_num(const char *v, double *out)
{
    char *end;
    double x = strtod(v, &end);
    if (end == v || *end != '\0')
        return -1;
    *out = x;
    return 0;
}

static int
parse_int(const char *v, int32_t *out)
{
    double x;
    if (parse_num(v, &x) < 0 || x != (double)(int32_t)x)
        return -1;
    *out = (int32_t)x;
    return 0;
}

/* what feat_params.json says about the front end: the settings, and the strings that have no
 * place in ssw_fe_config_t (NULL: not wanted) */
typedef struct {
    ssw_fe_config_t *c;
    ssw_fe_strings_t *s;
} fe_keys_t;

/* one key of the front end's; unknown keys are ignored (they belong to other modules) */
static int
fe_set_key(fe_keys_t *k, const char *key, const char *v, int is_string)
{
    ssw_fe_config_t *c = k->c;
    double d;
    if (key[0] == '-') /* command-line spelling */
        ++key;
#define NUM(name, field)                                                                    \
    if (!strcmp(key, name))                                                                 \
        return parse_num(v, &d) < 0 ? -1 : (c->field = d, 0);
#define INT(name, field)                                                                    \
    if (!strcmp(key, name))                                                                 \
        return parse_int(v, &c->field);
#define BOOL(name, field)                                                                   \
    if (!strcmp(key, name))                                                                 \
        return parse_bool(v, &c->field);
    NUM("samprate", samprate)
    NUM("wlen", wlen)
    NUM("alpha", alpha)
    NUM("lowerf", lowerf)
    NUM("upperf", upperf)
    INT("frate", frate)
    INT("nfft", nfft)
    INT("ncep", ncep)
    INT("nfilt", nfilt)
    INT("lifter", lifter)
    BOOL("remove_noise", remove_noise)
    BOOL("unit_area", unit_area)
    BOOL("round_filters", round_filters)
    BOOL("dither", dither)
    BOOL("remove_dc", remove_dc)
    BOOL("doublebw", doublebw)
    BOOL("smoothspec", smoothspec)
    BOOL("logspec", logspec)
#undef NUM
#undef INT
#undef BOOL
    if (!strcmp(key, "transform")) {
        if (!strcmp(v, "legacy"))
            c->transform = SSW_FE_LEGACY;
        else if (!strcmp(v, "dct"))
            c->transform = SSW_FE_DCT;
        else if (!strcmp(v, "htk"))
            c->transform = SSW_FE_HTK;
        else
            return -1;
        return 0;
    }
    if (!strcmp(key, "warp_params")) { /* null or "" = no warping (the default) */
        c->warp = is_string ? v[0] != '\0' : strcmp(v, "null") != 0;
        if (k->s != NULL)
            snprintf(k->s->warp_params, sizeof(k->s->warp_params), "%s", c->warp ? v : "");
        return 0;
    }
    if (k->s != NULL && !strcmp(key, "warp_type")) {
        snprintf(k->s->warp_type, sizeof(k->s->warp_type), "%s", v);
        return 0;
    }
    if (k->s != NULL && !strcmp(key, "input_endian")) {
        snprintf(k->s->input_endian, sizeof(k->s->input_endian), "%s", v);
        return 0;
    }
    return 0;
}

/* a flat JSON object: set(ctx, key, value, is_string) for every pair, which returns -1 for a
 * value it cannot use.  0 read, 1 no such file, -1 unusable (message in err) */
typedef int (*json_key_fn)(void *ctx, const char *key, const char *val, int is_string);

static int
json_object_read(const char *path, json_key_fn set, void *ctx, char *err, size_t err_len)
{
    FILE *f = fopen(path, "rb");
    char *buf = NULL, key[128], val[1100];
    const char *p;
    long len;
    int is_string, rv = -1;

    err[0] = '\0';
    if (f == NULL)
        return 1; /* no file: the defaults */
    if (fseek(f, 0, SEEK_END) != 0 || (len = ftell(f)) < 0 || len > (1 << 20)
        || fseek(f, 0, SEEK_SET) != 0 || (buf = (char *)malloc((size_t)len + 1)) == NULL
        || fread(buf, 1, (size_t)len, f) != (size_t)len) {
        snprintf(err, err_len, "%s: cannot read", path);
        goto done;
    }
    buf[len] = '\0';
    p = buf;
    while (isspace((unsigned char)*p))
        ++p;
    if (*p++ != '{') {
        snprintf(err, err_len, "%s: not a JSON object", path);
        goto done;
    }
    for (;;) {
        while (isspace((unsigned char)*p))
            ++p;
        if (*p == '}')
            break;
        if ((p = json_token(p, key, sizeof(key), &is_string)) == NULL || !is_string) {
            snprintf(err, err_len, "%s: expected a key", path);
            goto done;
        }
        while (isspace((unsigned char)*p))
            ++p;
        if (*p++ != ':' || (p = json_token(p, val, sizeof(val), &is_string)) == NULL) {
            snprintf(err, err_len, "%s: bad value of \"%s\"", path, key);
            goto done;
        }
        if (set(ctx, key, val, is_string) < 0) {
            snprintf(err, err_len, "%s: cannot use \"%s\" as the value of \"%s\"", path, val, key);
            goto done;
        }
        while (isspace((unsigned char)*p))
            ++p;
        if (*p == ',')
            ++p;
        else if (*p != '}') {
            snprintf(err, err_len, "%s: expected ',' or '}' after \"%s\"", path, key);
            goto done;
        }
    }
    rv = 0;
done:
    free(buf);
    fclose(f);
    return rv;
}

static int
fe_set_key_cb(void *ctx, const char *key, const char *v, int is_string)
{
    return fe_set_key((fe_keys_t *)ctx, key, v, is_string);
}

void
ssw_fe_strings_defaults(ssw_fe_strings_t *s)
{
    memset(s, 0, sizeof(*s));
    strcpy(s->warp_type, "inverse_linear"); /* config_defs.h:294, :385-393 */
    strcpy(s->input_endian, "little");      /* config_defs.h: "input_endian" */
}

int
ssw_fe_config_read_strings(const char *path, ssw_fe_config_t *c, ssw_fe_strings_t *s, char *err,
                           size_t err_len)
{
    fe_keys_t k;
    int rv;
    k.c = c;
    k.s = s;
    rv = json_object_read(path, fe_set_key_cb, &k, err, err_len);
    if (rv == 0)
        c->from_file = 1;
    return rv;
}

int
ssw_fe_config_read(const char *path, ssw_fe_config_t *c, char *err, size_t err_len)
{
    return ssw_fe_config_read_strings(path, c, NULL, err, err_len);
}

/* ---------------------------------------------------------------------------------- */
/* Front-end checks and tables, built exactly as fe_init builds them                     */
/* (src/fe_interface.c:86-330, src/fe_sigproc.c:70-252, :447-457): the same float /      */
/* double types operand by operand, libm for cos, sin, log10, pow and sqrt.  The kernels */
/* (ssw_k8_fe.inc) only read them.                                                       */
/* ---------------------------------------------------------------------------------- */
/* the checks of ssw_fe_batch (ex = 0: only its 16 kHz framing) and of ssw_fe_batch_ex (ex = 1:
 * the framing is ssw_fe_framing's, per rate) */
static int
fe_config_check(const ssw_fe_config_t *c, int ex)
{
    if (c->transform == SSW_FE_HTK) {
        ssw_set_error("front end: transform = htk is not supported (legacy or dct)");
        return -1;
    }
    if (c->transform != SSW_FE_LEGACY && c->transform != SSW_FE_DCT) {
        ssw_set_error("front end: unknown transform %d", c->transform);
        return -1;
    }
    if (c->dither || c->remove_dc || c->doublebw || c->smoothspec || c->logspec || c->warp) {
        ssw_set_error("front end: %s is not supported",
                      c->dither ? "dither" : c->remove_dc ? "remove_dc" : c->doublebw ? "doublebw"
                      : c->smoothspec ? "smoothspec" : c->logspec ? "logspec"
                      : "frequency warping (warp_params)");
        return -1;
    }
    if (!ex && (c->samprate != 16000 || c->frate != 100 || (float)c->wlen != (float)0.025625
                || (c->nfft != 0 && c->nfft != 512))) {
        ssw_set_error("front end: only samprate 16000, frate 100, wlen 0.025625 and a 512-point "
                      "FFT are supported (got %g, %d, %g, %d)", c->samprate, c->frate, c->wlen,
                      c->nfft);
        return -1;
    }
    if (c->ncep != 13 || (float)c->alpha != (float)0.97) {
        ssw_set_error("front end: only ncep 13 and alpha 0.97 are supported (got %d, %g)",
                      c->ncep, c->alpha);
        return -1;
    }
    if (!c->unit_area || !c->round_filters) {
        ssw_set_error("front end: only unit_area = yes and round_filters = yes are supported");
        return -1;
    }
    if (c->nfilt < 1 || c->nfilt > SSW_FE_MAX_FILT || c->lifter < 0) {
        ssw_set_error("front end: nfilt must be 1..%d and lifter >= 0 (got %d, %d)",
                      SSW_FE_MAX_FILT, c->nfilt, c->lifter);
        return -1;
    }
    /* (ssw_fe_framing checks upperf against each rate, with the reference's + 1) */
    if (!(c->lowerf >= 0) || !(c->lowerf < c->upperf) || (!ex && !(c->upperf <= c->samprate / 2))) {
        ssw_set_error("front end: need 0 <= lowerf < upperf <= samprate / 2 (got %g, %g)",
                      c->lowerf, c->upperf);
        return -1;
    }
    return 0;
}

int
ssw_fe_config_check(const ssw_fe_config_t *c)
{
    return fe_config_check(c, 0);
}

int
ssw_fe_config_check_ex(const ssw_fe_config_t *c)
{
    return fe_config_check(c, 1);
}

/* minimum_samprate, src/fe_interface.c:55-81 */
static int
fe_minimum_samprate(double upperf)
{
    static const int rates[] = {8000, 11025, 16000, 22050, 32000, 44100, 48000};
    const int nyquist = (int)(upperf * 2);
    size_t i;
    for (i = 0; i < sizeof(rates) / sizeof(rates[0]); ++i)
        if (rates[i] >= nyquist)
            return rates[i];
    return 16000; /* the reference's fallback */
}

/* fe_parse_general_params and fe_init, src/fe_interface.c:83-160, 255-301: the same float and
 * int types, the same refusals, and this front end's own FFT limit */
int
ssw_fe_framing(const ssw_fe_config_t *c, double samprate, ssw_fe_framing_t *f)
{
    float sr, wlen = (float)c->wlen;
    int window;
    /* "samprate" is an integer setting (config_defs.h:320-323) */
    if (!(samprate >= 0) || samprate != floor(samprate) || samprate > 1e7) {
        ssw_set_error("front end: samprate %g is not a whole number of hertz (0 .. 10^7)", samprate);
        return -1;
    }
    f->samprate = samprate == 0 ? fe_minimum_samprate(c->upperf) : (int32_t)samprate;
    sr = (float)f->samprate;
    if (c->frate > 32767 || c->frate > sr || c->frate < 1) {
        ssw_set_error("front end: frate %d must be 1 .. min(samprate %d, 32767)", c->frate,
                      f->samprate);
        return -1;
    }
    if (!(wlen * sr < (float)SSW_FE_MAX_NFFT * 2)) {
        ssw_set_error("front end: a window of %g samples (wlen %g at samprate %d) needs an FFT "
                      "above the %d points this front end supports", (double)(wlen * sr), c->wlen,
                      f->samprate, SSW_FE_MAX_NFFT);
        return -1;
    }
    window = (int)(wlen * sr);
    if (c->nfft == 0) {
        f->fft_order = 0;
        f->fft_size = 1;
        while (f->fft_size < window) {
            ++f->fft_order;
            f->fft_size <<= 1;
        }
    } else {
        if (c->nfft < 1 || (c->nfft & (c->nfft - 1)) != 0) {
            ssw_set_error("front end: nfft %d is not a power of 2", c->nfft);
            return -1;
        }
        if (c->nfft < window) {
            ssw_set_error("front end: nfft %d is smaller than the window of %d samples at "
                          "samprate %d", c->nfft, window, f->samprate);
            return -1;
        }
        f->fft_size = c->nfft;
        for (f->fft_order = 0; (1 << f->fft_order) < c->nfft; ++f->fft_order)
            ;
    }
    f->frame_shift = (int)(sr / c->frate + 0.5);
    f->frame_size = (int)(wlen * sr + 0.5);
    if (f->frame_shift <= 1) {
        ssw_set_error("front end: frame shift %d samples (samprate %d / frate %d) must be above 1",
                      f->frame_shift, f->samprate, c->frate);
        return -1;
    }
    if (f->frame_size < f->frame_shift) {
        ssw_set_error("front end: frame size %d (wlen) is smaller than frame shift %d (frate) at "
                      "samprate %d", f->frame_size, f->frame_shift, f->samprate);
        return -1;
    }
    if (f->frame_size > f->fft_size) {
        ssw_set_error("front end: nfft %d is smaller than the frame size %d at samprate %d",
                      f->fft_size, f->frame_size, f->samprate);
        return -1;
    }
    if (f->fft_size < SSW_FE_MIN_NFFT || f->fft_size > SSW_FE_MAX_NFFT) {
        ssw_set_error("front end: a %d-point FFT at samprate %d is outside the %d .. %d points "
                      "this front end supports", f->fft_size, f->samprate, SSW_FE_MIN_NFFT,
                      SSW_FE_MAX_NFFT);
        return -1;
    }
    if ((float)c->upperf > sr / 2 + 1.0) { /* upper_filt_freq is a float32 */
        ssw_set_error("front end: upperf %g is above samprate / 2 + 1 (samprate %d)", c->upperf,
                      f->samprate);
        return -1;
    }
    return 0;
}

/* One warping function at one rate: what fe_warp_set and the type's set_parameters leave in the
 * reference's statics (src/fe_warp.c:99-144, src/fe_warp_inverse_linear.c:95-133,
 * src/fe_warp_affine.c:96-134, src/fe_warp_piecewise_linear.c:105-159).  NULL = neutral. */
typedef struct {
    int id;
    float p[2], final_piece[2], nyquist;
} fe_warp_t;

/* NULL when fe is neutral, else w filled in for samprate */
static const fe_warp_t *
fe_warp_at(const struct ssw_fe_s *fe, float samprate, fe_warp_t *w)
{
    if (fe == NULL || !fe->warp_on)
        return NULL;
    memset(w, 0, sizeof(*w));
    w->id = fe->warp_id;
    w->p[0] = fe->warp_p[0];
    w->p[1] = fe->warp_p[1];
    w->nyquist = samprate / 2;
    if (w->id == SSW_FE_WARP_PIECEWISE_LINEAR && w->p[1] < samprate) {
        /* the line through (F, aF) and (N, N); F = 0 means 0.85 samprate */
        if (w->p[1] == 0)
            w->p[1] = samprate * 0.85f;
        w->final_piece[0] = (w->nyquist - w->p[0] * w->p[1]) / (w->nyquist - w->p[1]);
        w->final_piece[1] = w->nyquist * w->p[1] * (w->p[0] - 1.0f) / (w->nyquist - w->p[1]);
    }
    return w;
}

/* fe_warp_unwarped_to_warped */
static float
fe_warp_fwd(const fe_warp_t *w, float linear)
{
    float temp;
    if (w == NULL)
        return linear;
    switch (w->id) {
    case SSW_FE_WARP_INVERSE_LINEAR:
        return linear / w->p[0];
    case SSW_FE_WARP_AFFINE:
        temp = linear * w->p[0];
        temp += w->p[1];
        return temp;
    default:
        if (linear < w->p[1])
            return linear * w->p[0];
        return w->final_piece[0] * linear + w->final_piece[1];
    }
}

/* fe_warp_warped_to_unwarped (a result above Nyquist only makes the reference warn) */
static float
fe_warp_inv(const fe_warp_t *w, float nonlinear)
{
    float temp;
    if (w == NULL)
        return nonlinear;
    switch (w->id) {
    case SSW_FE_WARP_INVERSE_LINEAR:
        return nonlinear * w->p[0];
    case SSW_FE_WARP_AFFINE:
        temp = nonlinear - w->p[1];
        temp /= w->p[0];
        return temp;
    default:
        if (nonlinear < w->p[0] * w->p[1]) {
            temp = nonlinear / w->p[0];
        } else {
            temp = nonlinear - w->final_piece[1];
            temp /= w->final_piece[0];
        }
        return temp;
    }
}

static float
fe_mel(const fe_warp_t *w, float x) /* fe_mel, src/fe_sigproc.c:70-76 */
{
    float warped = fe_warp_fwd(w, x);
    return (float)(2595.0 * log10(1.0 + warped / 700.0));
}

static float
fe_melinv(const fe_warp_t *w, float x) /* fe_melinv, src/fe_sigproc.c:78-83 */
{
    float warped = (float)(700.0 * (pow(10.0, x / 2595.0) - 1.0));
    return fe_warp_inv(w, warped);
}

/* the three edge frequencies of filter i, src/fe_sigproc.c:120-132 */
static void
filter_edges(const fe_warp_t *w, int i, float melbw, float melmin, float fftfreq, int doublewide,
             int round_filters, float fr[3])
{
    int j;
    for (j = 0; j < 3; ++j) {
        if (doublewide)
            fr[j] = fe_melinv(w, (i + j * 2) * melbw + melmin);
        else
            fr[j] = fe_melinv(w, (i + j) * melbw + melmin);
        if (round_filters)
            fr[j] = ((int)(fr[j] / fftfreq + 0.5)) * fftfreq;
    }
}

/* fe_compute_melcosine, src/fe_sigproc.c:201-236: cosines [ncep][nfilt], the DCT's normalisers,
 * and the lifter (integer lifter_val / 2, as there; 1 when it is off) */
static void
fe_melcosine(int nfilt, int ncep, int lifter_val, float *mel_cosine, float *lifter,
             float *sqrt_inv_n, float *sqrt_inv_2n)
{
    double freqstep = M_PI / nfilt;
    int i, j;
    for (i = 0; i < ncep; ++i)
        for (j = 0; j < nfilt; ++j)
            mel_cosine[i * nfilt + j] = (float)cos(freqstep * i * (j + 0.5));
    *sqrt_inv_n = (float)sqrt(1.0 / nfilt);
    *sqrt_inv_2n = (float)sqrt(2.0 / nfilt);
    for (i = 0; i < ncep; ++i)
        lifter[i] = lifter_val ? (float)(1 + lifter_val / 2 * sin(i * M_PI / lifter_val)) : 1.0f;
}

/* the settings are checked (ssw_fe_config_check or _ex) before */
int
ssw_fe_tables_build(const ssw_fe_config_t *c, ssw_fe_tables_t *t)
{
    memset(t, 0, sizeof(*t));
    t->nfilt = c->nfilt;
    t->ncep = c->ncep;
    t->transform = c->transform;
    t->remove_noise = c->remove_noise;
    t->lifter_val = c->lifter;
    t->alpha = (float)c->alpha;
    fe_melcosine(t->nfilt, t->ncep, t->lifter_val, t->mel_cosine, t->lifter, &t->sqrt_inv_n,
                 &t->sqrt_inv_2n);
    return 0;
}

/* ssw_fe_tables_build for a resolved configuration: any ncep, and what the cepstrum kernel of
 * ssw_k8_fe_any.inc needs to know besides */
void
ssw_fe_any_tables_build(const struct ssw_fe_s *fe, ssw_fe_any_tables_t *t)
{
    const ssw_fe_config_t *c = &fe->cfg;
    memset(t, 0, sizeof(*t));
    t->nfilt = c->nfilt;
    t->ncep = c->ncep;
    t->transform = c->transform;
    t->remove_noise = c->remove_noise;
    t->lifter_val = c->lifter;
    t->alpha = (float)c->alpha;
    t->log_spec = fe->log_spec;
    t->remove_dc = c->remove_dc;
    t->out_dim = fe->out_dim;
    fe_melcosine(t->nfilt, t->ncep, t->lifter_val, t->mel_cosine, t->lifter, &t->sqrt_inv_n,
                 &t->sqrt_inv_2n);
}

/* fe: NULL for ssw_fe_batch(_ex, _f32)'s family of settings (no warping, single bandwidth) */
static ssw_fe_rate_t *
fe_rate_build(const ssw_fe_config_t *c, const ssw_fe_framing_t *f, int finite,
              const struct ssw_fe_s *fe)
{
    const float samprate = (float)f->samprate;
    const float lowerf = (float)c->lowerf, upperf = (float)c->upperf;
    const int doublewide = fe != NULL && c->doublebw;
    fe_warp_t warp;
    const fe_warp_t *w = fe_warp_at(fe, samprate, &warp);
    ssw_fe_rate_t h, *t;
    double *ham, *ccc, *sss;
    float *coeffs;
    int i, j, n_coeffs = 0;
    float melmin = fe_mel(w, lowerf), melmax = fe_mel(w, upperf);
    float melbw = (melmax - melmin) / (c->nfilt + 1);
    float fftfreq = samprate / (float)f->fft_size;

    if (doublewide) { /* src/fe_sigproc.c:103-113 */
        melmin -= melbw;
        melmax += melbw;
        if (fe_melinv(w, melmin) < 0 || fe_melinv(w, melmax) > samprate / 2) {
            ssw_set_error("front end: doublebw: the outer filter edges %g and %g Hz are outside "
                          "0 .. %g (samprate %d / 2)", (double)fe_melinv(w, melmin),
                          (double)fe_melinv(w, melmax), (double)(samprate / 2), f->samprate);
            return NULL;
        }
    }
    memset(&h, 0, sizeof(h));
    h.samprate = f->samprate;
    h.frame_shift = f->frame_shift;
    h.frame_size = f->frame_size;
    h.fft_size = f->fft_size;
    h.fft_order = f->fft_order;
    h.nfilt = c->nfilt;
    /* fe_build_melfilters, src/fe_sigproc.c:85-182: the widths first */
    for (i = 0; i < c->nfilt; ++i) {
        float fr[3];
        filter_edges(w, i, melbw, melmin, fftfreq, doublewide, c->round_filters, fr);
        h.spec_start[i] = -1;
        h.filt_width[i] = 0;
        for (j = 0; j < f->fft_size / 2 + 1; ++j) {
            float hz = j * fftfreq;
            if (hz < fr[0])
                continue;
            else if (hz > fr[2] || j == f->fft_size / 2) {
                h.filt_width[i] = j - h.spec_start[i];
                h.filt_start[i] = n_coeffs;
                n_coeffs += h.filt_width[i];
                break;
            }
            if (h.spec_start[i] == -1)
                h.spec_start[i] = j;
        }
        if (h.spec_start[i] < 0 || h.filt_width[i] < 1) {
            ssw_set_error("front end: mel filter %d of %d (lowerf %g, upperf %g) covers no DFT "
                          "point", i, c->nfilt, c->lowerf, c->upperf);
            return NULL;
        }
    }
    h.n_coeffs = n_coeffs;
    h.hamming_off = (int32_t)sizeof(ssw_fe_rate_t);
    h.ccc_off = h.hamming_off + (int32_t)sizeof(double) * (f->frame_size / 2);
    h.sss_off = h.ccc_off + (int32_t)sizeof(double) * (f->fft_size / 4);
    h.coeff_off = h.sss_off + (int32_t)sizeof(double) * (f->fft_size / 4);
    h.bytes = (h.coeff_off + (int32_t)sizeof(float) * n_coeffs + 7) & ~7;
    if ((t = (ssw_fe_rate_t *)calloc(1, (size_t)h.bytes)) == NULL) {
        ssw_set_error("front end: out of host memory");
        return NULL;
    }
    *t = h;
    ham = (double *)((char *)t + h.hamming_off);
    ccc = (double *)((char *)t + h.ccc_off);
    sss = (double *)((char *)t + h.sss_off);
    coeffs = (float *)((char *)t + h.coeff_off);
    /* fe_create_hamming, src/fe_sigproc.c:241-252 */
    for (i = 0; i < f->frame_size / 2; ++i)
        ham[i] = 0.54 - 0.46 * cos(2 * M_PI * i / ((double)f->frame_size - 1.0));
    /* fe_create_twiddle, src/fe_sigproc.c:447-457 */
    for (i = 0; i < f->fft_size / 4; ++i) {
        double a = 2 * M_PI * i / f->fft_size;
        ccc[i] = cos(a);
        sss[i] = sin(a);
    }
    /* the coefficients */
    n_coeffs = 0;
    for (i = 0; i < c->nfilt; ++i) {
        float fr[3];
        filter_edges(w, i, melbw, melmin, fftfreq, doublewide, c->round_filters, fr);
        for (j = 0; j < h.filt_width[i]; ++j) {
            float hz = (h.spec_start[i] + j) * fftfreq;
            float loslope = (hz - fr[0]) / (fr[1] - fr[0]);
            float hislope = (fr[2] - hz) / (fr[2] - fr[1]);
            if (c->unit_area) {
                loslope *= 2 / (fr[2] - fr[0]);
                hislope *= 2 / (fr[2] - fr[0]);
            }
            coeffs[n_coeffs++] = loslope < hislope ? loslope : hislope;
        }
        /* edges rounded onto one DFT point divide by zero: the reference's cepstra are NaN */
        for (j = 0; finite && j < h.filt_width[i]; ++j)
            if (!isfinite(coeffs[h.filt_start[i] + j])) {
                ssw_set_error("front end: mel filter %d of %d (lowerf %g, upperf %g) is narrower "
                              "than one DFT point (%g Hz) at samprate %d, nfft %d", i, c->nfilt,
                              c->lowerf, c->upperf, (double)fftfreq, f->samprate, f->fft_size);
                free(t);
                return NULL;
            }
    }
    return t;
}

ssw_fe_rate_t *
ssw_fe_rate_build(const ssw_fe_config_t *c, const ssw_fe_framing_t *f, int finite)
{
    return fe_rate_build(c, f, finite, NULL);
}

ssw_fe_rate_t *
ssw_fe_any_rate_build(const struct ssw_fe_s *fe, const ssw_fe_framing_t *f)
{
    return fe_rate_build(&fe->cfg, f, 1, fe);
}

/* fe_parse_general_params, fe_parse_melfb_params and fe_warp_set (src/fe_interface.c:84-210,
 * src/fe_warp.c:99-131) for everything that does not depend on the rate */
int
ssw_fe_resolve(const ssw_fe_config_t *cfg, const char *warp_type, const char *warp_params,
               struct ssw_fe_s *fe)
{
    static const char *const names[] = {"inverse_linear", "affine", "piecewise_linear"};
    static const char *const aliases[] = {"inverse", "linear", "piecewise"};
    const ssw_fe_config_t *c = &fe->cfg;
    const char *p;
    int i, n_param, given = warp_params != NULL && warp_params[0] != '\0';

    memset(fe, 0, sizeof(*fe));
    fe->cfg = *cfg;
    if (warp_type == NULL)
        warp_type = names[0];
    if (c->transform != SSW_FE_LEGACY && c->transform != SSW_FE_DCT && c->transform != SSW_FE_HTK) {
        ssw_set_error("front end: unknown transform %d", c->transform);
        return -1;
    }
    if (c->dither) {
        ssw_set_error("front end: dither is not supported: its random stream belongs to a "
                      "process's lifetime");
        return -1;
    }
    if (c->ncep < 1 || c->ncep > SSW_FE_MAX_CEP || c->nfilt < 1 || c->nfilt > SSW_FE_MAX_FILT) {
        ssw_set_error("front end: ncep must be 1..%d and nfilt 1..%d (got %d, %d)", SSW_FE_MAX_CEP,
                      SSW_FE_MAX_FILT, c->ncep, c->nfilt);
        return -1;
    }
    if (c->lifter < 0) {
        ssw_set_error("front end: lifter must be >= 0 (got %d)", c->lifter);
        return -1;
    }
    if (!isfinite((float)c->alpha)) {
        ssw_set_error("front end: alpha %g is not a finite float32", c->alpha);
        return -1;
    }
    if (!(c->lowerf >= 0) || !(c->lowerf < c->upperf)) {
        ssw_set_error("front end: need 0 <= lowerf < upperf (got %g, %g)", c->lowerf, c->upperf);
        return -1;
    }
    for (i = 0; i < 3 && strcmp(warp_type, names[i]) != 0 && strcmp(warp_type, aliases[i]) != 0; ++i)
        ;
    if (i == 3) {
        ssw_set_error("front end: Unimplemented warping function %s", warp_type);
        return -1;
    }
    fe->warp_id = i;
    if (c->warp && !given) {
        ssw_set_error("front end: warp is set but no warp_params are given");
        return -1;
    }
    if (given && strlen(warp_params) >= sizeof(fe->warp_params)) {
        ssw_set_error("front end: warp_params is longer than %d characters",
                      (int)sizeof(fe->warp_params) - 1);
        return -1;
    }
    snprintf(fe->warp_type, sizeof(fe->warp_type), "%s", names[i]);
    snprintf(fe->warp_params, sizeof(fe->warp_params), "%s", given ? warp_params : "");
    fe->cfg.warp = given;
    /* set_parameters: atof of up to N_PARAM blank-separated tokens, the rest ignored; slope 0 is
     * neutral */
    n_param = fe->warp_id == SSW_FE_WARP_INVERSE_LINEAR ? 1 : 2;
    for (p = fe->warp_params, i = 0; given && i < n_param; ++i) {
        p += strspn(p, " \t");
        if (*p == '\0')
            break;
        fe->warp_p[i] = (float)atof(p);
        p += strcspn(p, " \t");
    }
    fe->warp_on = given && fe->warp_p[0] != 0;
    fe->log_spec = c->smoothspec ? SSW_FE_SMOOTH_LOG_SPEC : c->logspec ? SSW_FE_RAW_LOG_SPEC
                                                                       : SSW_FE_CEPSTRA;
    fe->out_dim = fe->log_spec ? c->nfilt : c->ncep; /* fe_get_output_size */
    fe->plain = !given && ssw_fe_config_check_ex(c) == 0;
    return 0;
}

/* Frame sample i after pre-emphasis is x[i] - x[i - 1] alpha with |x| <= 2^15 whole numbers and
 * alpha = k 2^q (k odd): a multiple of 2^g, g = min(q, 0), of size at most 2^15 (1 + |alpha|).
 * Every sum of some of a frame's n samples is then a multiple of 2^g of size at most
 * B = n 2^15 (1 + |alpha|); where B < 2^(53 + g) a double holds each of them exactly, so no
 * addition in any order rounds and every order gives the reference's sum.  float32 samples have
 * no such grid. */
int
ssw_fe_dc_sum_exact(float alpha, int32_t frame_size, int f32)
{
    int e, g = 0;
    double m;
    if (f32 || !isfinite(alpha))
        return 0;
    if (alpha != 0) {
        m = frexp(fabs((double)alpha), &e); /* |alpha| = m 2^e, m in [0.5, 1) */
        while (m != floor(m)) {              /* -> k 2^q */
            m *= 2;
            --e;
        }
        g = e < 0 ? e : 0;
    }
    if (53 + g < 0)
        return 0;
    return (double)frame_size * 32768.0 * (1.0 + fabs((double)alpha)) < ldexp(1.0, 53 + g);
}

int64_t
ssw_fe_frames_of(int64_t n)
{
    ssw_fe_framing_t f;
    f.frame_size = SSW_FE_FRAME;
    f.frame_shift = SSW_FE_SHIFT;
    return ssw_fe_frames_at(&f, n);
}

/* fe_process_int16 + fe_end over n samples (src/fe_interface.c:560-712): the full frames, then
 * fe_end's frame of the samples left over, when there are any */
int64_t
ssw_fe_frames_at(const ssw_fe_framing_t *f, int64_t n)
{
    int64_t full;
    if (n < 0)
        return -1;
    if (n == 0)
        return 0;
    if (n < f->frame_size)
        return 1;
    full = 1 + (n - f->frame_size) / f->frame_shift;
    return full + (n - full * f->frame_shift > 0);
}

/* ---------------------------------------------------------------------------------- */
/* Integer log domain (logmath_t).  Only what load time needs: log(), ln_to_log() at a  */
/* given shift, and the 8-bit add table at shift 10.                                   */
/* ---------------------------------------------------------------------------------- */
typedef struct {
    double inv_ln_base;
    double base;
} lbase_t;

static int
ilog(const lbase_t *b, int shift, double p)
{
    if (p <= 0)
        return (int)((int32_t)0x80000000 >> (shift + 2)); /* logmath zero, logmath.c:84 */
    return (int)(log(p) * b->inv_ln_base) >> shift;      /* logmath.c:288 */
}

static int
iln_to_log(const lbase_t *b, int shift, double ln_p)
{
    return (int)(ln_p * b->inv_ln_base) >> shift; /* logmath.c:300 */
}

/* Add table for (base, shift): entry d = round(log_base(1 + base^-d')) >> shift for the first
 * unshifted d' that lands in slot d (logmath.c:101-161).  Returns the entry count the
 * reference would allocate (>= 256) or -1 when entries need more than 8 bits. */
static int
build_logadd8(const lbase_t *b, int shift, uint8_t out[256])
{
    uint32_t maxyx = (uint32_t)(log(2.0) / log(b->base) + 0.5) >> shift;
    double byx = 1.0;
    uint32_t i, size;
    uint8_t seen[256];

    if (maxyx >= 256)
        return -1;
    memset(out, 0, 256);
    memset(seen, 0, sizeof(seen));
    for (i = 0;; ++i) {
        double lobyx = log(1.0 + byx) * b->inv_ln_base;
        int32_t k = (int32_t)(lobyx + 0.5 * (1 << shift)) >> shift;
        uint32_t slot = i >> shift;
        /* the reference keeps a slot's first value and treats a stored 0 as "empty" */
        if (slot < 256 && out[slot] == 0)
            out[slot] = (uint8_t)k;
        if (k <= 0)
            break;
        byx /= b->base;
    }
    size = (i >> shift);
    if (size < 255)
        size = 255;
    (void)seen;
    return (int)size + 1;
}

/* ---------------------------------------------------------------------------------- */
/* Byte cursor over a whole file                                                       */
/* ---------------------------------------------------------------------------------- */
typedef struct {
    uint8_t *base;
    size_t size, at;
    int swap, summing;
    uint32_t sum;
    const char *name;
} rd_t;

static int
rd_open(rd_t *r, const char *path)
{
    FILE *fp = fopen(path, "rb");
    long sz;
    memset(r, 0, sizeof(*r));
    r->name = path;
    if (fp == NULL) {
        ssw_set_error("%s: cannot open", path);
        return -1;
    }
    if (fseek(fp, 0, SEEK_END) != 0 || (sz = ftell(fp)) < 0) {
        fclose(fp);
        ssw_set_error("%s: cannot size", path);
        return -1;
    }
    rewind(fp);
    r->base = (uint8_t *)malloc(sz ? (size_t)sz : 1);
    r->size = (size_t)sz;
    if (r->base == NULL || fread(r->base, 1, r->size, fp) != r->size) {
        fclose(fp);
        free(r->base);
        r->base = NULL;
        ssw_set_error("%s: read failed", path);
        return -1;
    }
    fclose(fp);
    return 0;
}

static void
rd_close(rd_t *r)
{
    free(r->base);
    r->base = NULL;
}

static uint32_t
flip32(uint32_t v)
{
    return ((v & 0xffu) << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
}

/* n 32-bit words -> dst, honouring byte order and the rolling checksum
 * (sum = rotl(sum, 20) + word, src/s3file.c:383-387) */
static int
rd_words(rd_t *r, void *dst, size_t n)
{
    uint32_t *w = (uint32_t *)dst;
    size_t i;
    if (r->size - r->at < 4 * n) {
        ssw_set_error("%s: truncated (wanted %zu words at offset %zu)", r->name, n, r->at);
        return -1;
    }
    memcpy(w, r->base + r->at, 4 * n);
    r->at += 4 * n;
    if (r->swap)
        for (i = 0; i < n; ++i)
            w[i] = flip32(w[i]);
    if (r->summing) {
        uint32_t s = r->sum;
        for (i = 0; i < n; ++i)
            s = ((s << 20) | (s >> 12)) + w[i];
        r->sum = s;
    }
    return 0;
}

static int
rd_i32(rd_t *r, int32_t *v)
{
    return rd_words(r, v, 1);
}

/* "s3\n" text header: `name value` lines up to `endhdr`, then the 0x11223344 marker.
 * A `chksum0` line (any value) switches the trailing checksum on (src/s3file.c:289-290). */
static int
rd_s3_header(rd_t *r)
{
    int want_sum = 0;
    uint32_t mark;
    if (r->size < 3 || memcmp(r->base, "s3\n", 3) != 0) {
        ssw_set_error("%s: missing s3 signature", r->name);
        return -1;
    }
    r->at = 3;
    for (;;) {
        const char *line = (const char *)r->base + r->at;
        const char *eol = memchr(line, '\n', r->size - r->at);
        size_t len, a, z;
        if (r->at >= r->size) {
            ssw_set_error("%s: header runs off the end", r->name);
            return -1;
        }
        len = eol ? (size_t)(eol - line) : r->size - r->at;
        r->at += eol ? len + 1 : len;
        for (a = 0; a < len && (line[a] == ' ' || line[a] == '\t' || line[a] == '\r'); ++a)
            ;
        for (z = a; z < len && !(line[z] == ' ' || line[z] == '\t' || line[z] == '\r'); ++z)
            ;
        if (z == a) {
            ssw_set_error("%s: empty header line", r->name);
            return -1;
        }
        if (line[a] == '#')
            continue;
        if (z - a <= 6 && memcmp(line + a, "endhdr", z - a) == 0)
            break;
        if (z - a == 7 && memcmp(line + a, "chksum0", 7) == 0)
            want_sum = 1;
    }
    if (rd_words(r, &mark, 1) < 0)
        return -1;
    if (mark != 0x11223344u) {
        if (flip32(mark) != 0x11223344u) {
            ssw_set_error("%s: bad byte-order marker %08x", r->name, mark);
            return -1;
        }
        r->swap = 1;
    }
    r->summing = want_sum;
    r->sum = 0;
    return 0;
}

static int
rd_s3_finish(rd_t *r)
{
    uint32_t expect, got;
    if (!r->summing)
        return 0;
    got = r->sum;
    r->summing = 0;
    if (rd_words(r, &expect, 1) < 0)
        return -1;
    if (expect != got) {
        ssw_set_error("%s: checksum mismatch (file %08x, computed %08x)", r->name, expect, got);
        return -1;
    }
    return 0;
}

/* ---------------------------------------------------------------------------------- */
/* Dynamic features: the FEAT_OPTIONS keys of feat_params.json (include/soundswallower/ */
/* config_defs.h:418-450) and the configuration feat_init_s3file makes of them          */
/* (src/feat.c:732-927).  The kernels (ssw_k12_feat.inc) only read the tables.          */
/* ---------------------------------------------------------------------------------- */
void
ssw_feat_config_defaults(ssw_feat_config_t *c)
{
    memset(c, 0, sizeof(*c));
    strcpy(c->feat, "1s_c_d_dd");
    c->ceplen = 13;
    c->cmn = SSW_CMN_LIVE;
    strcpy(c->cmninit, "40,3,-1");
}

/* a string setting: null = unset */
static int
feat_set_str(char *dst, size_t cap, const char *v, int is_string)
{
    if (!is_string && !strcmp(v, "null"))
        v = "";
    if (strlen(v) >= cap)
        return -1;
    strcpy(dst, v);
    return 0;
}

static int
feat_set_key(void *ctx, const char *key, const char *v, int is_string)
{
    ssw_feat_config_t *c = (ssw_feat_config_t *)ctx;
    if (key[0] == '-') /* command-line spelling */
        ++key;
    if (!strcmp(key, "feat"))
        return v[0] == '\0' ? -1 : feat_set_str(c->feat, sizeof(c->feat), v, 1);
    if (!strcmp(key, "ceplen"))
        return parse_int(v, &c->ceplen);
    if (!strcmp(key, "ldadim"))
        return parse_int(v, &c->ldadim);
    if (!strcmp(key, "varnorm"))
        return parse_bool(v, &c->varnorm);
    if (!strcmp(key, "cmninit"))
        return feat_set_str(c->cmninit, sizeof(c->cmninit), v, is_string);
    if (!strcmp(key, "lda"))
        return feat_set_str(c->lda, sizeof(c->lda), v, is_string);
    if (!strcmp(key, "svspec"))
        return feat_set_str(c->svspec, sizeof(c->svspec), v, is_string);
    if (!strcmp(key, "cmn")) {
        /* cmn_type_from_str, src/cmn.c:55-79: "Unknown CMN type" is fatal there */
        if (!strcmp(v, "none"))
            c->cmn = SSW_CMN_NONE;
        else if (!strcmp(v, "batch") || !strcmp(v, "current"))
            c->cmn = SSW_CMN_BATCH;
        else if (!strcmp(v, "live") || !strcmp(v, "prior"))
            c->cmn = SSW_CMN_LIVE;
        else
            return -1;
        return 0;
    }
    return 0;
}

int
ssw_feat_config_read_err(const char *path, ssw_feat_config_t *c, char *err, size_t err_len)
{
    const int rv = json_object_read(path, feat_set_key, c, err, err_len);
    if (rv == 0)
        c->from_file = 1;
    return rv;
}

int
ssw_feat_config_read(const char *path, ssw_feat_config_t *c)
{
    char err[600];
    int rv;
    if (path == NULL || c == NULL) {
        ssw_set_error("bad arguments to ssw_feat_config_read");
        return -1;
    }
    rv = ssw_feat_config_read_err(path, c, err, sizeof(err));
    if (rv < 0)
        ssw_set_error("%s", err);
    return rv;
}

void
ssw_feat_plan_free(ssw_feat_plan_t *p)
{
    free(p->recipe);
    free(p->lda_t);
    free(p->sv);
    p->recipe = NULL;
    p->lda_t = NULL;
    p->sv = NULL;
}

/* the generic type "n,n,...[:window]" as src/feat.c:827-884 scans it: commas between the first
 * and the last character become blanks, a colon there ends the list and atoi reads the window
 * behind it, every blank-separated word is a stream width read with %u */
static int
feat_plan_generic(const char *type, int32_t ceplen, ssw_feat_plan_t *p)
{
    char mtype[64], wd[64];
    const size_t len = strlen(type);
    const char *strp;
    size_t i;
    int k = 0, n = 0, l;
    long long cepsize = 0;

    if (len == 0 || len >= sizeof(mtype))
        goto bad;
    strcpy(mtype, type);
    for (i = 1; i + 1 < len; ++i) {
        if (mtype[i] == ',') {
            mtype[i] = ' ';
            ++k;
        } else if (mtype[i] == ':') {
            mtype[i] = '\0';
            p->window = atoi(mtype + i + 1);
            break;
        }
    }
    ++k;
    if (p->window < 0 || p->window > SSW_FEAT_MAX_WIN) {
        ssw_set_error("feat = %s: a window of %d frames (supported: 0..%d)", type, p->window,
                      SSW_FEAT_MAX_WIN);
        return -1;
    }
    if (k > SSW_MAX_FEAT) {
        ssw_set_error("feat = %s: %d streams (supported: at most %d)", type, k, SSW_MAX_FEAT);
        return -1;
    }
    p->n_stream = k;
    strp = mtype;
    while (sscanf(strp, "%63s%n", wd, &l) == 1) {
        unsigned int w;
        strp += l;
        if (n >= k || sscanf(wd, "%u", &w) != 1 || w == 0 || w > SSW_FEAT_MAX_CEP)
            goto bad;
        cepsize += w;
        p->stream_len[n++] = (int32_t)w * (2 * p->window + 1);
    }
    if (n != k || cepsize != ceplen)
        goto bad;
    p->cepsize = ceplen;
    return 0;
bad:
    ssw_set_error("feat = %s: Bad feature type argument (ceplen %d)", type, ceplen);
    return -1;
}

/* feat_read_lda_s3file, src/lda.c:84-122: a 3-d float array of which matrix 0 is used, its
 * checksum verified, as wide as the stream; dim <= 0 or beyond the rows = every row.  The used
 * rows go into p->lda_t transposed, [column][row]. */
static int
feat_plan_read_lda(const char *path, int32_t dim, ssw_feat_plan_t *p)
{
    rd_t r;
    int32_t dims[3], total, rows, j, k;
    float *data = NULL;

    if (rd_open(&r, path) < 0)
        return -1;
    if (rd_s3_header(&r) < 0 || rd_words(&r, dims, 3) < 0 || rd_i32(&r, &total) < 0)
        goto bad;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || dims[1] > (1 << 20) || dims[2] > (1 << 20)
        || (int64_t)total != (int64_t)dims[0] * dims[1] * dims[2] || total > (1 << 26)) {
        ssw_set_error("%s: %d values do not make a %d x %d x %d transform", path, total, dims[0],
                      dims[1], dims[2]);
        goto bad;
    }
    data = (float *)malloc(sizeof(float) * (size_t)total);
    if (data == NULL) {
        ssw_set_error("out of memory");
        goto bad;
    }
    if (rd_words(&r, data, (size_t)total) < 0 || rd_s3_finish(&r) < 0)
        goto bad;
    if (dims[2] != p->stream_len[0]) {
        ssw_set_error("%s: LDA matrix dimension %d doesn't match feature stream size %d", path,
                      dims[2], p->stream_len[0]);
        goto bad;
    }
    rows = (dim > dims[1] || dim <= 0) ? dims[1] : dim;
    if (rows > SSW_FEAT_MAX_LDA_ROWS) {
        ssw_set_error("%s: %d rows of the LDA matrix are used (supported: at most %d)", path, rows,
                      SSW_FEAT_MAX_LDA_ROWS);
        goto bad;
    }
    p->lda_t = (float *)malloc(sizeof(float) * (size_t)rows * (size_t)dims[2]);
    if (p->lda_t == NULL) {
        ssw_set_error("out of memory");
        goto bad;
    }
    for (j = 0; j < rows; ++j)
        for (k = 0; k < dims[2]; ++k)
            p->lda_t[(size_t)k * rows + j] = data[(size_t)j * dims[2] + k];
    p->lda_rows = rows;
    free(data);
    rd_close(&r);
    return 0;
bad:
    free(data);
    rd_close(&r);
    return -1;
}

/* parse_subvecs and feat_set_subvecs, src/feat.c:181-341: subvectors apart by '/', in each a
 * comma-separated list of dimensions or ranges a-b; a dimension may not come twice in one
 * subvector.  `pre` is feat_dimension (the LDA's rows, else the stream's length). */
static int
feat_plan_svspec(const char *str, int32_t pre, ssw_feat_plan_t *p)
{
    const char *s = str;
    /* (a subvector starts with at most `pre` <= raw_dim entries before it and adds at most
     * raw_dim distinct ones before the total is checked) */
    int32_t *sv = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * p->raw_dim + 1));
    int n_sv = 0, n_dim = 0, first = 0;

    if (sv == NULL) {
        ssw_set_error("out of memory");
        return -1;
    }
    for (;;) {
        int n, n2, l, q;
        if (sscanf(s, "%d%n", &n, &l) != 1) {
            ssw_set_error("svspec '%s': Couldn't read int32 @pos %d", str, (int)(s - str));
            goto bad;
        }
        s += l;
        n2 = n;
        if (*s == '-') {
            ++s;
            if (sscanf(s, "%d%n", &n2, &l) != 1) {
                ssw_set_error("svspec '%s': Couldn't read int32 @pos %d", str, (int)(s - str));
                goto bad;
            }
            s += l;
        }
        if (n < 0 || n > n2) {
            ssw_set_error("svspec '%s': Bad subrange spec ending @pos %d", str, (int)(s - str));
            goto bad;
        }
        if (n2 >= p->raw_dim) {
            /* (the reference reads past the frame's row here) */
            ssw_set_error("svspec '%s': dimension %d ending @pos %d is beyond the %d the stream has",
                          str, n2, (int)(s - str), p->raw_dim);
            goto bad;
        }
        for (; n <= n2; ++n) {
            for (q = first; q < n_dim; ++q)
                if (sv[q] == n) {
                    ssw_set_error("svspec '%s': Duplicate dimension ending @pos %d", str,
                                  (int)(s - str));
                    goto bad;
                }
            sv[n_dim++] = n; /* (no duplicates in a subvector: at most raw_dim entries each) */
        }
        if (*s == ',') {
            ++s;
            continue;
        }
        if (*s != '\0' && *s != '/') {
            ssw_set_error("svspec '%s': Bad delimiter @pos %d", str, (int)(s - str));
            goto bad;
        }
        if (n_sv >= SSW_MAX_FEAT) {
            ssw_set_error("svspec '%s': more than %d subvectors", str, SSW_MAX_FEAT);
            goto bad;
        }
        p->sv_len[n_sv++] = n_dim - first;
        first = n_dim;
        if (n_dim > pre) {
            ssw_set_error("svspec '%s': Total dimensionality of subvector specification %d "
                          "> feature dimensionality %d", str, n_dim, pre);
            goto bad;
        }
        if (*s == '\0')
            break;
        ++s;
    }
    p->sv = sv;
    p->n_sv = n_sv;
    p->sv_dim = n_dim;
    return 0;
bad:
    free(sv);
    return -1;
}

int
ssw_feat_plan_build(const ssw_feat_config_t *c, ssw_feat_plan_t *p)
{
    const char *type = c->feat;
    int32_t cepsize = c->ceplen == 0 ? 13 : c->ceplen; /* src/feat.c:741-742 */
    int32_t kind, i, j, k, w, C;
    uint32_t *r;
    enum { K_S2_4X, K_S3_1X39, K_C_D_DD, K_C_D_LD_DD, K_C_D, K_C, K_COPY };

    memset(p, 0, sizeof(*p));
    if (memchr(c->feat, '\0', sizeof(c->feat)) == NULL || memchr(c->cmninit, '\0', sizeof(c->cmninit)) == NULL
        || memchr(c->lda, '\0', sizeof(c->lda)) == NULL || memchr(c->svspec, '\0', sizeof(c->svspec)) == NULL) {
        ssw_set_error("feature configuration: a string setting is not terminated");
        return -1;
    }
    if (cepsize < 1 || cepsize > SSW_FEAT_MAX_CEP) {
        ssw_set_error("feature configuration: ceplen %d (supported: 1..%d)", cepsize, SSW_FEAT_MAX_CEP);
        return -1;
    }
    if (c->cmn != SSW_CMN_NONE && c->cmn != SSW_CMN_BATCH && c->cmn != SSW_CMN_LIVE) {
        ssw_set_error("feature configuration: Unknown CMN type %d", c->cmn);
        return -1;
    }
    /* the reference's chain of comparisons, in its order (src/feat.c:749-884) */
    p->n_stream = 1;
    p->cepsize = cepsize;
    if (strcmp(type, "s2_4x") == 0) {
        if (cepsize != 13) {
            ssw_set_error("feat = s2_4x: s2_4x features require cepsize == 13 (ceplen is %d)", cepsize);
            return -1;
        }
        kind = K_S2_4X;
        p->n_stream = 4;
        p->stream_len[0] = 12;
        p->stream_len[1] = 24;
        p->stream_len[2] = 3;
        p->stream_len[3] = 12;
        p->window = 4;
    } else if (strcmp(type, "s3_1x39") == 0 || strcmp(type, "1s_12c_12d_3p_12dd") == 0) {
        if (cepsize != 13) {
            ssw_set_error("feat = %s: s3_1x39 features require cepsize == 13 (ceplen is %d)", type,
                          cepsize);
            return -1;
        }
        kind = K_S3_1X39;
        p->stream_len[0] = 39;
        p->window = 3;
    } else if (strncmp(type, "1s_c_d_dd", 9) == 0) {
        kind = K_C_D_DD;
        p->stream_len[0] = cepsize * 3;
        p->window = 3; /* FEAT_DCEP_WIN + 1 */
    } else if (strncmp(type, "1s_c_d_ld_dd", 12) == 0) {
        kind = K_C_D_LD_DD;
        p->stream_len[0] = cepsize * 4;
        p->window = 4; /* FEAT_DCEP_WIN * 2 */
    } else if (strncmp(type, "cep_dcep", 8) == 0 || strncmp(type, "1s_c_d", 6) == 0) {
        kind = K_C_D;
        p->stream_len[0] = cepsize * 2;
        p->window = 2;
    } else if (strncmp(type, "cep", 3) == 0 || strncmp(type, "1s_c", 4) == 0) {
        kind = K_C;
        p->stream_len[0] = cepsize;
        p->window = 0;
    } else if (strncmp(type, "1s_3c", 5) == 0 || strncmp(type, "1s_4c", 5) == 0) {
        kind = K_COPY;
        p->window = strncmp(type, "1s_3c", 5) == 0 ? 3 : 4;
        p->stream_len[0] = cepsize * (2 * p->window + 1);
    } else {
        kind = K_COPY;
        if (feat_plan_generic(type, cepsize, p) < 0)
            return -1;
    }
    for (j = 0; j < p->n_stream; ++j)
        p->raw_dim += p->stream_len[j];
    p->cmn = c->cmn;
    p->varnorm = c->varnorm != 0;
    if (p->cmn == SSW_CMN_LIVE && p->varnorm) {
        /* cmn_live, src/cmn_live.c:114-115: fatal at the first utterance */
        ssw_set_error("feature configuration: Variance normalization not implemented in live mode "
                      "decode (varnorm with cmn = live)");
        return -1;
    }
    /* cmn_set_repr, src/cmn.c:112-140 */
    if (p->cmn != SSW_CMN_NONE && c->cmninit[0]) {
        char vals[sizeof(c->cmninit)], *s = vals, *cc;
        int nvals = 0;
        strcpy(vals, c->cmninit);
        while (nvals < cepsize && (cc = strchr(s, ',')) != NULL) {
            *cc = '\0';
            p->prior_mean[nvals] = (float)atof(s);
            p->prior_sum[nvals] = p->prior_mean[nvals] * 500; /* CMN_WIN */
            s = cc + 1;
            ++nvals;
        }
        if (nvals < cepsize && *s != '\0') {
            p->prior_mean[nvals] = (float)atof(s);
            p->prior_sum[nvals] = p->prior_mean[nvals] * 500;
        }
        p->prior_nframe = 500;
    }
    /* the recipe of every raw dimension, as the compute_feat functions write them
     * (src/feat.c:437-712) */
    r = p->recipe = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)p->raw_dim);
    if (r == NULL) {
        ssw_set_error("out of memory");
        return -1;
    }
    C = cepsize;
#define COPY(i, o) SSW_FEAT_RECIPE(0, i, o, 0, 0, 0)
#define DELTA(i, o) SSW_FEAT_RECIPE(1, i, o, -(o), 0, 0)
#define DDELTA(i) SSW_FEAT_RECIPE(2, i, 3, -1, 1, -3)
    switch (kind) {
    case K_S2_4X: /* cep 1..12 | short and long delta | c0, its delta and delta-delta | dd */
        for (i = 0; i < 12; ++i) {
            r[i] = COPY(i + 1, 0);
            r[12 + i] = DELTA(i + 1, 2);
            r[24 + i] = DELTA(i + 1, 4);
            r[39 + i] = DDELTA(i + 1);
        }
        r[36] = COPY(0, 0);
        r[37] = DELTA(0, 2);
        r[38] = DDELTA(0);
        break;
    case K_S3_1X39: /* cep 1..12 | delta | c0, its delta and delta-delta | dd */
        for (i = 0; i < 12; ++i) {
            r[i] = COPY(i + 1, 0);
            r[12 + i] = DELTA(i + 1, 2);
            r[27 + i] = DDELTA(i + 1);
        }
        r[24] = COPY(0, 0);
        r[25] = DELTA(0, 2);
        r[26] = DDELTA(0);
        break;
    case K_C_D_DD:
        for (i = 0; i < C; ++i) {
            r[i] = COPY(i, 0);
            r[C + i] = DELTA(i, 2);
            r[2 * C + i] = DDELTA(i);
        }
        break;
    case K_C_D_LD_DD:
        for (i = 0; i < C; ++i) {
            r[i] = COPY(i, 0);
            r[C + i] = DELTA(i, 2);
            r[2 * C + i] = DELTA(i, 4);
            r[3 * C + i] = DDELTA(i);
        }
        break;
    case K_C_D:
        for (i = 0; i < C; ++i) {
            r[i] = COPY(i, 0);
            r[C + i] = DELTA(i, 2);
        }
        break;
    case K_C:
        for (i = 0; i < C; ++i)
            r[i] = COPY(i, 0);
        break;
    default: /* feat_copy: frames -window .. window of every stream's part, side by side */
        for (j = 0, k = 0, i = 0; j < p->n_stream; ++j) {
            const int32_t sl = p->stream_len[j] / (2 * p->window + 1);
            int32_t e;
            for (w = -p->window; w <= p->window; ++w)
                for (e = 0; e < sl; ++e)
                    r[k++] = COPY(i + e, w);
            i += sl;
        }
        break;
    }
#undef COPY
#undef DELTA
#undef DDELTA
    p->out_dim = p->raw_dim;
    if (c->lda[0]) {
        if (p->n_stream != 1) {
            ssw_set_error("feature configuration: LDA incompatible with multi-stream features "
                          "(n_stream = %d)", p->n_stream);
            goto bad;
        }
        if (feat_plan_read_lda(c->lda, c->ldadim, p) < 0)
            goto bad;
        p->out_dim = p->lda_rows;
    }
    if (c->svspec[0]) {
        if (p->n_stream != 1) {
            ssw_set_error("feature configuration: Subvector specifications require single-stream "
                          "features! (n_stream = %d)", p->n_stream);
            goto bad;
        }
        if (feat_plan_svspec(c->svspec, p->out_dim, p) < 0)
            goto bad;
        p->out_dim = p->sv_dim;
    }
    return 0;
bad:
    ssw_feat_plan_free(p);
    return -1;
}

/* ---------------------------------------------------------------------------------- */
/* Gaussians                                                                           */
/* ---------------------------------------------------------------------------------- */
static float *
read_gauss_file(const char *path, int32_t shape[3], int32_t veclen[SSW_MAX_FEAT])
{
    rd_t r;
    int32_t total, per_density = 0, i;
    float *data = NULL;

    if (rd_open(&r, path) < 0)
        return NULL;
    if (rd_s3_header(&r) < 0 || rd_words(&r, shape, 3) < 0)
        goto bad;
    if (shape[1] < 1 || shape[1] > SSW_MAX_FEAT || shape[0] < 1 || shape[2] < 1) {
        ssw_set_error("%s: unsupported shape %d x %d x %d", path, shape[0], shape[1], shape[2]);
        goto bad;
    }
    if (rd_words(&r, veclen, (size_t)shape[1]) < 0 || rd_i32(&r, &total) < 0)
        goto bad;
    for (i = 0; i < shape[1]; ++i)
        per_density += veclen[i];
    if (total != shape[0] * shape[2] * per_density) {
        ssw_set_error("%s: %d values do not match %d x %d x %d", path, total, shape[0],
                      shape[2], per_density);
        goto bad;
    }
    data = (float *)malloc(sizeof(float) * (size_t)total);
    if (data == NULL || rd_words(&r, data, (size_t)total) < 0 || rd_s3_finish(&r) < 0)
        goto bad;
    rd_close(&r);
    return data;
bad:
    free(data);
    rd_close(&r);
    return NULL;
}

/* The read step: means and variances as the files hold them (mean0, var0), the shape, and
 * working copies (mean, var) for precompute_gaussians. */
static int
read_gaussians(ssw_host_model_t *h, const char *means, const char *vars)
{
    int32_t sm[3], sv[3], vlv[SSW_MAX_FEAT], f;
    size_t n;

    if ((h->mean0 = read_gauss_file(means, sm, h->veclen)) == NULL)
        return -1;
    if ((h->var0 = read_gauss_file(vars, sv, vlv)) == NULL)
        return -1;
    if (memcmp(sm, sv, sizeof(sm)) != 0 || memcmp(h->veclen, vlv, sizeof(int32_t) * sm[1])) {
        ssw_set_error("means and variances have different shapes");
        return -1;
    }
    h->n_cb = sm[0];
    h->n_feat = sm[1];
    h->n_density = sm[2];
    for (f = 0, h->veclen_total = 0; f < h->n_feat; ++f) {
        h->featoff[f] = h->veclen_total;
        h->veclen_total += h->veclen[f];
    }
    n = (size_t)h->n_cb * h->n_density * (size_t)h->veclen_total;
    h->det = (float *)malloc(sizeof(float) * (size_t)h->n_cb * h->n_feat * h->n_density);
    h->mean = (float *)malloc(sizeof(float) * n);
    h->var = (float *)malloc(sizeof(float) * n);
    if (h->det == NULL || h->mean == NULL || h->var == NULL) {
        ssw_set_error("out of memory reading the Gaussians");
        return -1;
    }
    memcpy(h->mean, h->mean0, sizeof(float) * n);
    memcpy(h->var, h->var0, sizeof(float) * n);
    return 0;
}

/* The precompute step (gauden_dist_precompute, src/ms_gauden.c:211-247) over h->var, which holds
 * un-precomputed variances: floor, det, scaled variance. */
static void
precompute_gaussians(ssw_host_model_t *h, const lbase_t *lb)
{
    const float vfloor = (float)h->cfg.varfloor; /* float32 parameter, ms_gauden.c:218 */
    float *vp = h->var, *dp = h->det;
    int32_t c, f, d, j;

    /* Walk the file order once: per density, det = sum_j (float)ilog(1/sqrt(2 pi var_j))
     * accumulated in float32; var_j <- (float)iln_to_log(1/(2 var_j)); floor first. */
    h->n_floored = 0;
    for (c = 0; c < h->n_cb; ++c)
        for (f = 0; f < h->n_feat; ++f)
            for (d = 0; d < h->n_density; ++d) {
                float acc = 0;
                for (j = 0; j < h->veclen[f]; ++j, ++vp) {
                    if (*vp < vfloor) {
                        *vp = vfloor;
                        h->n_floored++;
                    }
                    acc += (float)ilog(lb, 0, 1.0 / sqrt(*vp * 2.0 * M_PI));
                    *vp = (float)iln_to_log(lb, 0, 1.0 / (*vp * 2.0));
                }
                *dp++ = acc;
            }
}

/* ---------------------------------------------------------------------------------- */
/* Transition matrices                                                                 */
/* ---------------------------------------------------------------------------------- */
static void
renorm(float *v, int n)
{
    double s = 0.0, k;
    int i;
    for (i = 0; i < n; ++i)
        s += v[i];
    if (s == 0.0)
        return;
    k = 1.0 / s;
    for (i = 0; i < n; ++i)
        v[i] = (float)(v[i] * k);
}

static int
load_tmat(ssw_host_model_t *h, const lbase_t *lb, const char *path)
{
    rd_t r;
    int32_t dims[4], t, i, k;
    float row[16];

    if (rd_open(&r, path) < 0)
        return -1;
    if (rd_s3_header(&r) < 0 || rd_words(&r, dims, 4) < 0)
        goto bad;
    if (dims[2] != dims[1] + 1 || dims[2] > 16 || dims[3] != dims[0] * dims[1] * dims[2]) {
        ssw_set_error("%s: unsupported transition shape %d x %d x %d", path, dims[0], dims[1],
                      dims[2]);
        goto bad;
    }
    h->tp_n_tmat = dims[0];
    h->tp_n_state = dims[1];
    h->tp = (uint8_t *)malloc((size_t)dims[3]);
    for (t = 0; t < dims[0]; ++t)
        for (i = 0; i < dims[1]; ++i) {
            if (rd_words(&r, row, (size_t)dims[2]) < 0)
                goto bad;
            renorm(row, dims[2]);
            for (k = 0; k < dims[2]; ++k) /* floor only non-zero arcs, vector.c:116-123 */
                if (row[k] != 0.0 && row[k] < h->cfg.tmatfloor)
                    row[k] = (float)h->cfg.tmatfloor;
            renorm(row, dims[2]);
            for (k = 0; k < dims[2]; ++k) {
                int q = (-ilog(lb, 0, row[k])) >> SSW_SENSCR_SHIFT; /* tmat.c:206 */
                h->tp[((size_t)t * dims[1] + i) * dims[2] + k] = (uint8_t)(q > 255 ? 255 : q);
            }
        }
    if (rd_s3_finish(&r) < 0)
        goto bad;
    rd_close(&r);
    return 0;
bad:
    rd_close(&r);
    return -1;
}

/* ---------------------------------------------------------------------------------- */
/* Binary model definition                                                             */
/* ---------------------------------------------------------------------------------- */
static uint32_t
peek32(const rd_t *r, size_t at)
{
    uint32_t v;
    memcpy(&v, r->base + at, 4);
    return r->swap ? flip32(v) : v;
}

static uint16_t
peek16(const rd_t *r, size_t at)
{
    uint16_t v;
    memcpy(&v, r->base + at, 2);
    return r->swap ? (uint16_t)((v << 8) | (v >> 8)) : v;
}

static int
load_mdef(ssw_host_model_t *h, const char *path)
{
    rd_t r;
    int32_t magic, ver, desc_len, hd[10], n_tree, i, j;
    size_t names, at, phones, n_sseq_words;

    if (rd_open(&r, path) < 0)
        return -1;
    if (rd_i32(&r, &magic) < 0)
        goto bad;
    if ((uint32_t)magic == 0x424d4446u)
        r.swap = 1;
    else if ((uint32_t)magic != 0x46444d42u) {
        ssw_set_error("%s: not a BMDF file", path);
        goto bad;
    }
    if (rd_i32(&r, &ver) < 0 || rd_i32(&r, &desc_len) < 0)
        goto bad;
    if (ver > 1 || desc_len < 0 || r.at + (size_t)desc_len > r.size) {
        ssw_set_error("%s: unsupported BMDF version/descriptor", path);
        goto bad;
    }
    r.at += (size_t)desc_len;
    if (rd_words(&r, hd, 10) < 0)
        goto bad;
    h->n_ciphone = hd[0];
    h->n_phone = hd[1];
    h->n_emit_state = hd[2];
    h->n_ci_sen = hd[3];
    h->n_sen = hd[4];
    h->n_tmat = hd[5];
    h->n_sseq = hd[6];
    n_tree = hd[8];
    if (h->n_emit_state < 1) {
        ssw_set_error("%s: mixed-topology mdef not supported", path);
        goto bad;
    }
    /* the counts size every table below: a damaged header must not become an allocation of
     * -1 elements or an index past a row */
    if (h->n_ciphone < 1 || h->n_ciphone > 255 || h->n_phone < h->n_ciphone || h->n_sen < 1
        || h->n_sen > 0xffff || h->n_ci_sen < 0 || h->n_ci_sen > h->n_sen || h->n_tmat < 1
        || h->n_sseq < 1 || n_tree < 0 || h->n_emit_state > 16) {
        ssw_set_error("%s: implausible header (%d CI phones, %d phones, %d states, %d senones, "
                      "%d tmats, %d senone sequences, %d tree nodes)", path, h->n_ciphone,
                      h->n_phone, h->n_emit_state, h->n_sen, h->n_tmat, h->n_sseq, n_tree);
        goto bad;
    }
    /* CI names: n_ciphone NUL-terminated strings, block padded to 4 bytes */
    names = at = r.at;
    h->sil = -1;
    h->ciname = (char **)calloc((size_t)h->n_ciphone, sizeof(char *));
    if (h->ciname == NULL)
        goto oom;
    for (i = 0; i < h->n_ciphone; ++i) {
        const char *nm = (const char *)r.base + at;
        size_t l = strnlen(nm, r.size - at);
        if (at + l >= r.size)
            goto trunc;
        if (l == 3 && memcmp(nm, "SIL", 3) == 0)
            h->sil = i;
        h->ciname[i] = (char *)malloc(l + 1);
        if (h->ciname[i] == NULL)
            goto oom;
        memcpy(h->ciname[i], nm, l + 1);
        at += l + 1;
    }
    at = names + ((at - names + 3) / 4) * 4;
    if (at + (size_t)n_tree * 8 > r.size)
        goto trunc;
    h->n_cd_tree = n_tree;
    h->cd_tree = (struct ssw_cd_node_s *)malloc(sizeof(*h->cd_tree) * (size_t)(n_tree ? n_tree : 1));
    if (h->cd_tree == NULL)
        goto oom;
    for (i = 0; i < n_tree; ++i) {
        h->cd_tree[i].ctx = (int16_t)peek16(&r, at + 8 * (size_t)i);
        h->cd_tree[i].n_down = (int16_t)peek16(&r, at + 8 * (size_t)i + 2);
        h->cd_tree[i].down_or_pid = (int32_t)peek32(&r, at + 8 * (size_t)i + 4);
    }
    phones = at + (size_t)n_tree * 8;
    at = phones + (size_t)h->n_phone * 12;
    if (at + 4 > r.size)
        goto trunc;
    n_sseq_words = peek32(&r, at);
    at += 4;
    if (at + 2 * n_sseq_words > r.size || n_sseq_words < (size_t)h->n_sseq * h->n_emit_state)
        goto trunc;
    h->sseq = (uint16_t *)malloc(2 * n_sseq_words);
    if (h->sseq == NULL)
        goto oom;
    for (i = 0; (size_t)i < n_sseq_words; ++i)
        h->sseq[i] = peek16(&r, at + 2 * (size_t)i);
    for (i = 0; i < h->n_sseq * h->n_emit_state; ++i)
        if (h->sseq[i] >= h->n_sen) { /* would index past a score row on the device */
            ssw_set_error("%s: senone sequence %d names senone %d of %d", path,
                          i / h->n_emit_state, h->sseq[i], h->n_sen);
            goto bad;
        }

    h->phone_ssid = (int32_t *)malloc(sizeof(int32_t) * (size_t)h->n_phone);
    h->phone_tmat = (int32_t *)malloc(sizeof(int32_t) * (size_t)h->n_phone);
    h->sen2cb = (int16_t *)malloc(sizeof(int16_t) * (size_t)h->n_sen);
    h->ci_filler = (uint8_t *)calloc((size_t)h->n_ciphone, 1);
    if (!h->phone_ssid || !h->phone_tmat || !h->sen2cb || !h->ci_filler)
        goto oom;
    for (i = 0; i < h->n_sen; ++i)
        h->sen2cb[i] = -1;
    for (i = 0; i < h->n_ciphone && i < h->n_phone; ++i)
        h->ci_filler[i] = r.base[phones + (size_t)i * 12 + 8]; /* info.ci.filler */
    for (i = 0; i < h->n_phone; ++i) {
        size_t e = phones + (size_t)i * 12;
        int base = (i < h->n_ciphone) ? i : r.base[e + 9]; /* first context byte = base phone */
        h->phone_ssid[i] = (int32_t)peek32(&r, e);
        h->phone_tmat[i] = (int32_t)peek32(&r, e + 4);
        if (h->phone_ssid[i] < 0 || h->phone_ssid[i] >= h->n_sseq)
            continue;
        for (j = 0; j < h->n_emit_state; ++j) {
            int s = h->sseq[(size_t)h->phone_ssid[i] * h->n_emit_state + j];
            if (s < h->n_sen && h->sen2cb[s] < 0) /* first owner wins, bin_mdef.c:505-506 */
                h->sen2cb[s] = (int16_t)base;
        }
    }
    rd_close(&r);
    return 0;
oom:
    ssw_set_error("%s: out of memory", path);
    goto bad;
trunc:
    ssw_set_error("%s: truncated", path);
bad:
    rd_close(&r);
    return -1;
}

/* ---------------------------------------------------------------------------------- */
/* Mixture weights                                                                     */
/* ---------------------------------------------------------------------------------- */
static int
has_prefix(const uint8_t *s, size_t n, const char *key, int *val)
{
    size_t k = strlen(key);
    if (n > k && memcmp(s, key, k) == 0) {
        *val = atoi((const char *)s + k);
        return 1;
    }
    return 0;
}

static int
load_sendump(ssw_host_model_t *h, const char *path)
{
    rd_t r;
    int32_t len, rows, cols;
    int feats = h->n_feat, dens = h->n_density, sens = h->n_sen, clusters = 0, bits = 8, f, d, s;
    uint8_t codebook[16];
    size_t stride;

    if (rd_open(&r, path) < 0)
        return -1;
    /* title: its length also reveals the byte order */
    if (rd_i32(&r, &len) < 0)
        goto bad;
    if (len < 1 || len > 999) {
        len = (int32_t)flip32((uint32_t)len);
        if (len < 1 || len > 999) {
            ssw_set_error("%s: implausible title length", path);
            goto bad;
        }
        r.swap = 1;
    }
    if (r.at + (size_t)len > r.size || r.base[r.at + len - 1] != 0)
        goto trunc;
    r.at += (size_t)len;
    /* header string */
    if (rd_i32(&r, &len) < 0)
        goto bad;
    if (len < 1 || r.at + (size_t)len > r.size || r.base[r.at + len - 1] != 0)
        goto trunc;
    r.at += (size_t)len;
    /* key/value strings, terminated by a zero length */
    for (;;) {
        if (rd_i32(&r, &len) < 0)
            goto bad;
        if (len == 0)
            break;
        if (len < 0 || r.at + (size_t)len > r.size)
            goto trunc;
        (void)(has_prefix(r.base + r.at, (size_t)len, "feature_count ", &feats)
               || has_prefix(r.base + r.at, (size_t)len, "mixture_count ", &dens)
               || has_prefix(r.base + r.at, (size_t)len, "model_count ", &sens)
               || has_prefix(r.base + r.at, (size_t)len, "cluster_count ", &clusters)
               || has_prefix(r.base + r.at, (size_t)len, "cluster_bits ", &bits));
        r.at += (size_t)len;
    }
    rows = dens;
    cols = sens;
    if (clusters == 0 && (rd_i32(&r, &rows) < 0 || rd_i32(&r, &cols) < 0))
        goto bad;
    if (feats != h->n_feat || dens != h->n_density || sens != h->n_sen || rows != dens) {
        ssw_set_error("%s: sendump is %d x %d x %d, model is %d x %d x %d", path, feats, dens,
                      sens, h->n_feat, h->n_density, h->n_sen);
        goto bad;
    }
    if ((clusters != 0 && clusters != 15 && clusters != 16) || (bits != 8 && bits != 4)) {
        ssw_set_error("%s: unsupported cluster_count %d / cluster_bits %d", path, clusters, bits);
        goto bad;
    }
    memset(codebook, 0, sizeof(codebook));
    if (clusters) {
        int n = clusters == 15 ? 16 : clusters; /* 15 is stored as 16, ptm_mgau.c:575-576 */
        if (r.at + (size_t)n > r.size)
            goto trunc;
        memcpy(codebook, r.base + r.at, (size_t)n);
        r.at += (size_t)n;
    }
    stride = bits == 4 ? ((size_t)cols + 1) / 2 : (size_t)cols;
    if (r.at + stride * (size_t)rows * (size_t)feats > r.size)
        goto trunc;
    h->ptm_mixw = (uint8_t *)malloc((size_t)feats * dens * sens);
    for (f = 0; f < feats; ++f)
        for (d = 0; d < dens; ++d) {
            const uint8_t *src = r.base + r.at + ((size_t)f * rows + d) * stride;
            uint8_t *dst = h->ptm_mixw + ((size_t)f * dens + d) * sens;
            if (!clusters) {
                memcpy(dst, src, (size_t)sens);
                continue;
            }
            /* Clustered dump, expanded once here with the reference's decode rule, which
             * keys the nibble choice on the packed byte's own low bit (ptm_mgau.c:375-378). */
            for (s = 0; s < sens; ++s) {
                int packed = src[s / 2];
                int code = (packed & 1) ? packed >> 4 : packed & 0x0f;
                /* the s2_semi scorer takes the nibble by the senone's parity instead
                 * (src/s2_semi_mgau.c:809-810) */
                if (ssw_host_scorer(h) == SSW_SCORER_S2_SEMI)
                    code = (s & 1) ? packed >> 4 : packed & 0x0f;
                dst[s] = codebook[code];
            }
        }
    rd_close(&r);
    return 0;
trunc:
    ssw_set_error("%s: truncated", path);
bad:
    rd_close(&r);
    return -1;
}

static int
load_mixw(ssw_host_model_t *h, const lbase_t *lb, const char *path, int fill_ptm)
{
    rd_t r;
    int32_t dims[4], s, f, c;
    float *w = NULL;
    const float wfloor = (float)h->cfg.mixwfloor;

    if (rd_open(&r, path) < 0)
        return -1;
    if (rd_s3_header(&r) < 0 || rd_words(&r, dims, 4) < 0)
        goto bad;
    if (dims[1] != h->n_feat || dims[2] != h->n_density || dims[3] != dims[0] * dims[1] * dims[2]
        || (h->n_sen && dims[0] != h->n_sen)) {
        ssw_set_error("%s: mixture weights are %d x %d x %d, model wants %d x %d x %d", path,
                      dims[0], dims[1], dims[2], h->n_sen, h->n_feat, h->n_density);
        goto bad;
    }
    h->n_sen = dims[0];
    w = (float *)malloc(sizeof(float) * (size_t)dims[2]);
    h->ms_pdf = (uint8_t *)malloc((size_t)dims[3]);
    if (fill_ptm)
        h->ptm_mixw = (uint8_t *)malloc((size_t)dims[3]);
    for (s = 0; s < dims[0]; ++s)
        for (f = 0; f < dims[1]; ++f) {
            if (rd_words(&r, w, (size_t)dims[2]) < 0)
                goto bad;
            renorm(w, dims[2]);
            for (c = 0; c < dims[2]; ++c)
                if (w[c] < (double)wfloor)
                    w[c] = wfloor;
            renorm(w, dims[2]);
            for (c = 0; c < dims[2]; ++c) {
                /* ms: shift-0 log, +511, >>10, saturate 255 (ms_senone.c:176-182) */
                int p = -ilog(lb, 0, w[c]) + ((1 << (SSW_SENSCR_SHIFT - 1)) - 1);
                h->ms_pdf[((size_t)s * dims[1] + f) * dims[2] + c]
                    = (uint8_t)(p < (255 << SSW_SENSCR_SHIFT) ? p >> SSW_SENSCR_SHIFT : 255);
                if (fill_ptm) { /* PTM: shift-10 log, saturate 159 (ptm_mgau.c:678-681) */
                    int q = -ilog(lb, SSW_SENSCR_SHIFT, w[c]);
                    if (q > SSW_MAX_NEG_MIXW || q < 0)
                        q = SSW_MAX_NEG_MIXW;
                    h->ptm_mixw[((size_t)f * dims[2] + c) * dims[0] + s] = (uint8_t)q;
                }
            }
        }
    if (rd_s3_finish(&r) < 0)
        goto bad;
    free(w);
    rd_close(&r);
    return 0;
bad:
    free(w);
    rd_close(&r);
    return -1;
}

/* ---------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------- */
/* device-layout Gaussian records and the quadratic-form scan records                   */
/* ---------------------------------------------------------------------------------- */
static int
cmp_float(const void *a, const void *b)
{
    float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}

/* The speculative scan evaluates  det - sum var (x - mean)^2  as a quadratic form in x,
 *   key = c + sum_j (a_j x_j + b_j x_j^2),  a = 2 var mean,  b = -var,
 *   c = (det - d0) - R + bias,  R = sum var mean^2,  d0 = the codebook's median det,
 * with 26 fused multiply-adds.  With u = 2^-24, S = sum var (x - mean)^2 and
 * M = |det - d0| + R + sum |a x| + sum |b| x^2 <= |det - d0| + 6 R + 3 S
 * (Cauchy-Schwarz), the form is within 27 u M of the real number and the reference's
 * fp32 value within 13 u |det| + 17 u S of it (13 subtractions whose partial sums lie
 * between det and the result; (1+u)^4 on every product); with
 * S <= |det - d0| + |value - d0| that is u (125 |det - d0| + 162 R + 13 |det|) -- folded
 * into c as `bias` with a few per cent of slack, so the key is an upper bound -- plus
 * 98 u |value - d0|, which the kernel adds (104 u |key| + 0.001: |value| and |key| differ
 * by at most the bias) to the one key it uses as a bound.  Densities whose bias would
 * exceed 4 score units (floored variances far from the origin) get an inert scan record
 * and go on the codebook's exact-form list: the kernel evaluates them the reference's
 * way after the scan.  tests/test_scan_bound.py replays the kernel's arithmetic on the
 * CPU against these tables. */
/* round-to-nearest-even float -> IEEE binary16, subnormals kept, overflow to infinity: what
 * v_cvt_pk_f16_f32 does with the kernels' default mode (tools/microbench/mfma_f16_scan.hip
 * compares the two on values down to 2^-40) */
static uint16_t
f16_rne(float x)
{
    uint32_t u, sign, mant;
    int e;
    memcpy(&u, &x, 4);
    sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u) /* inf / nan */
        return (uint16_t)(sign | 0x7c00u | (u > 0x7f800000u ? 0x200u : 0u));
    e = (int)(u >> 23) - 127;
    mant = (u & 0x7fffffu) | 0x800000u; /* 24 bits, value = mant 2^(e - 23) */
    if (e >= 16)
        return (uint16_t)(sign | 0x7c00u);
    if (e >= -14) { /* normal: keep 11 bits */
        uint32_t keep = mant >> 13, rest = mant & 0x1fffu;
        uint32_t h = ((uint32_t)(e + 15) << 10) + (keep & 0x3ffu);
        if (rest > 0x1000u || (rest == 0x1000u && (keep & 1u)))
            ++h; /* may carry into the exponent, up to infinity: correct */
        return (uint16_t)(sign | h);
    }
    if (e < -26) /* below half of the smallest subnormal (2^-25): zero */
        return (uint16_t)sign;
    {
        /* subnormal: value = q 2^-24, q = mant 2^(e + 1) rounded */
        const int shift = -1 - e; /* 14 .. 25 */
        uint32_t q = mant >> shift, rest = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rest > half || (rest == half && (q & 1u)))
            ++q;
        return (uint16_t)(sign | q);
    }
}

static float
f16_to_float(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const int e = (h >> 10) & 0x1f;
    const uint32_t m = h & 0x3ffu;
    float x;
    if (e == 0)
        x = ldexpf((float)m, -24);
    else if (e == 31)
        x = m ? NAN : INFINITY;
    else
        x = ldexpf((float)(m | 0x400u), e - 25);
    return sign ? -x : x;
}

/* x = p[0] + p[1] + r: two binary16 parts of a float, the first residual x - p[0] exact in float
 * arithmetic; |r| <= max(2^-22 |x|, 2^-25) while the parts stay finite */
static void
f16_split2(float x, uint16_t p[2])
{
    p[0] = f16_rne(x);
    p[1] = f16_rne(x - f16_to_float(p[0]));
}

/* Scan records for the matrix-core scan (csrc/ssw_k1a_mfma.inc).  The key of density i for
 * frame x is the same quadratic form c + sum_j (a_j x_j + b_j x_j^2) as in recq.
 *
 * Round 4: W = (a, c, b) and X = (x, 1, x^2) are cut into TWO binary16 parts each (2 x 11 = 22
 * significand bits) and the three part products (1,1) (1,2) (2,1) are accumulated by six
 * v_mfma_f32_32x32x16_f16 per 32 x 32 tile -- rounds 2-3 used three bf16 parts and six part
 * products, twelve MFMAs, for the same error constant.  binary16 has a narrow exponent range, so
 * the rows of a codebook x stream are scaled by one power of two, W' = W 2^-s (its keys come out
 * as key 2^-s: only keys of one codebook x stream are ever compared, and the kernel scales the
 * one key it uses as a bound back), and the constant travels as c' = c 2^-s 2^-ec against
 * X = 2^ec.  The kernel refuses the speculative result of a frame with |x_j| > 255 (x_j^2 would
 * not fit binary16): such a frame takes the exact pass.
 *
 * Error of the evaluated key against the real number, in units of u = 2^-24, with
 * M = sum_k |W_k X_k| (all of it scales with 2^-s, so the analysis is the unscaled one):
 *   (a) x^2 rounded to fp32 before the split:                          1 u M
 *   (b) what the three products leave out: W X - (W1 X1 + W1 X2 + W2 X1) = W2 X2 + (W1 + W2) Xr
 *       + Wr X with Xr, Wr the residuals of the two-part splits.  |W2| <= 2^-11 |W|, |X2| <=
 *       2^-11 |X|: 4 u M; |Xr| <= max(2^-22 |X|, 2^-25) (binary16 subnormals are honoured by the
 *       conversion and by the matrix pipe, tools/microbench/mfma_f16_scan.hip): 4 u M plus the
 *       CONSTANT 2^-25 sum_k |W'_k| 2^s; Wr is known here exactly, element by element: an
 *       element whose |Wr_k| Xmax_k (Xmax = 255, 255^2, 2^ec) stays below 0.02 score units is
 *       charged that constant, the others relatively, rho = max_k |Wr_k| / |W_k| (2^-22 = 4 u
 *       when both parts of the element are normal numbers):                (8.01 u + rho) M
 *   (c) the accumulation error of the six chained MFMAs.  Every product of two binary16 values
 *       is exact in fp32 (22 bits), so MFMA i returns the exact sum of its 16 products and its C
 *       input up to e_i <= eps (m_i + |C_i|), m_i = the sum of the |products| it adds.  The chain
 *       adds the small products first -- (1,2) and (2,1) of both K blocks, m_i <= 2^-11 M_kb
 *       (1 + 2^-11) -- then the (1,1) products of K block 0 and of K block 1 (M_0 + M_1 = M);
 *       |C_i| <= sum_{j<i} m_j (1 + eps)^i, so  sum e_i <= eps sum_j m_j (1 + number of MFMAs
 *       after j) <= eps (2 + 6 * 2 * 2^-11 * 1.001) M <= 2.01 eps M.
 *       eps itself is not documented for v_mfma_f32_32x32x16_f16.  Two models cover what a
 *       17-term fp32 adder can do: (A) the terms are added one after the other, in any order,
 *       each addition rounded OR truncated to fp32: error <= 16 * 2^-23 = 32 u of sum |terms|;
 *       (B) the terms are aligned to the largest exponent, truncated to a 24-bit grid, summed
 *       exactly and rounded once: 16 * 2 u + 2 u = 34 u.  eps <= 34 u is assumed -- 6.5 times
 *       the worst value tools/microbench/mfma_f16_scan.hip measures on cancelling data
 *       (5.2 u):                                                           68.4 u M
 *   (d) a = 2 var mean rounded to fp32 (b = -var is exact; c is rounded UP to a value its two
 *       parts represent exactly, below):                                    1 u M
 * Together K_i u M with K_i = 79 + rho_i / u per density (78.4 rounded up; 83 when every element
 * keeps both parts normal); a density whose K_i would pass SSW_MFMA_K = 96 goes on the
 * exact-form list.  An inert row is a = b = 0 with -65504 in the two spare K slots 13 and 14,
 * which X holds at 32768: key' = -4.3e9.
 * tests/test_gpu_mfma_bound.py checks the resulting bound on the device on stress inputs and on
 * inputs built to cancel (x = 2 mean: every a_j x_j + b_j x_j^2 pair cancels, M is 8 R while the
 * value is det - R), tests/test_scan_bound.py replays (a) and (b) exactly on the CPU (everything
 * but the adder), and tests/test_gpu_scan_agreement.py checks that the matrix-core scan and the
 * vector-unit scan (whose bound IS replayed on the CPU in full) give identical top-N blocks.
 * The reference's own fp32 value is within 13 u |det| + 17 u S of the real number, and
 * M <= |det - d0| + 6 R + 3 S, S <= |det - d0| + |value - d0| as for recq, which gives the
 * per-density constant (4 K_i + 17) |det - d0| + 6 K_i R + 13 |det| (in u) folded into c below
 * with the constants of (b), with slack, and the term (3 K + 17) u |value - d0| the kernel adds
 * (with K = SSW_MFMA_K) to the one key it uses as a bound.  Densities whose constant exceeds
 * SSW_MFMA_MAX_BIAS score units keep an inert record and are evaluated in the exact form
 * (exlistm); so is a density that alone forces a scale s at which others lose their second part
 * (a floored variance of 5e7 next to variances of 2). */
#define SSW_MFMA_K 96.0
#define SSW_MFMA_K0 79.0
#define SSW_MFMA_MAX_BIAS 64.0
#define SSW_MFMA_XMAX 255.0
#define SSW_MFMA_ABS_UNIT 0.02

/* the K index of MFMA operand slot k (record float slot): 0..12 a | 15 c | 16..28 b */
static double
mfma_slot_xmax(int k, double xconst)
{
    if (k < SSW_MAX_VECLEN)
        return SSW_MFMA_XMAX;
    if (k == SSW_REC_DET)
        return xconst;
    return SSW_MFMA_XMAX * SSW_MFMA_XMAX;
}

/* One density under scale 2^-s (and 2^-ec on the constant): its error constant K_i, the additive
 * constant of (b) in score units, and whether every scaled element stays finite in binary16.
 * q = the unscaled record (a, c WITHOUT bias, b). */
static int
mfma_density_terms(const double *q, int s, int ec, double *K_i, double *add)
{
    const double u24 = 1.0 / 16777216.0, scale = ldexp(1.0, s);
    double rho = 0.0, cst = 0.0, sumw = 0.0;
    int k;
    for (k = 0; k < SSW_REC_FLOATS; ++k) {
        uint16_t p[2];
        double w, wr;
        float wf;
        if (q[k] == 0.0)
            continue;
        wf = (float)ldexp(q[k], -(s + (k == SSW_REC_DET ? ec : 0)));
        if (!(fabsf(wf) <= 32768.0f))
            return -1;
        if (k == SSW_REC_DET) /* the constant is rounded up to what its parts represent: no error */
            continue;
        f16_split2(wf, p);
        w = (double)wf;
        wr = fabs(w - ((double)f16_to_float(p[0]) + (double)f16_to_float(p[1])));
        /* (the float rounding of the scaled element itself: q 2^-s is exact unless q 2^-s is a
         * float subnormal, which |q| >= 2^-100 rules out for every sane model) */
        if (wr * mfma_slot_xmax(k, 0.0) * scale <= SSW_MFMA_ABS_UNIT)
            cst += wr * mfma_slot_xmax(k, 0.0) * scale;
        else if (wr / fabs(w) > rho)
            rho = wr / fabs(w);
        sumw += fabs(w); /* X residual below the binary16 grid: 2^-25 per element */
    }
    cst += ldexp(sumw, -25) * scale;
    *K_i = SSW_MFMA_K0 + rho / u24;
    *add = cst;
    return 0;
}

/* A derived table of n elements, all zero: made on the first call, cleared in place on a later
 * one (a rebuild after ssw_host_model_apply_mllr: every size is what it was). */
static void *
table_zeroed(void *have, size_t n, size_t size)
{
    if (have == NULL)
        return calloc(n, size);
    memset(have, 0, n * size);
    return have;
}

static int
ssw_host_build_mfma_records(ssw_host_model_t *h)
{
    const int ncbf = h->n_cb * h->n_feat;
    const size_t nrec = (size_t)ncbf * h->n_density;
    const double u24 = 1.0 / 16777216.0;
    int cbf, d, j, rb, kb, p, l, e;
    double *qd;       /* [n_density][SSW_REC_FLOATS] unscaled a, c (no bias), b of one cbf */
    double *geo;      /* [n_density][4]: delta, R, det, max |a|,|b| */
    unsigned char *inert;

    h->n_exact_form_m = 0;
    if (h->n_density != 128)
        return 0; /* the MFMA scan is built for 128 densities; other shapes use the FMA scan */
    h->recqm = (float *)table_zeroed(h->recqm, nrec * SSW_REC_FLOATS, sizeof(float));
    h->exlistm = (uint32_t *)table_zeroed(h->exlistm, (size_t)ncbf * SSW_EXLIST_STRIDE,
                                          sizeof(uint32_t));
    h->wfrag = (uint16_t *)table_zeroed(h->wfrag, (size_t)ncbf * SSW_WFRAG_PER_CBF,
                                        sizeof(uint16_t));
    h->rec28 = (float *)table_zeroed(h->rec28, nrec * 28, sizeof(float));
    if (h->rec28 != NULL) {
        size_t i;
        for (i = 0; i < nrec; ++i) {
            const float *r = h->rec + i * SSW_REC_FLOATS;
            float *q28 = h->rec28 + i * 28;
            for (j = 0; j < 13; ++j) {
                q28[j] = r[j];
                q28[14 + j] = r[SSW_REC_VAR + j];
            }
            q28[13] = r[SSW_REC_DET];
        }
    }
    qd = (double *)calloc((size_t)h->n_density * SSW_REC_FLOATS, sizeof(double));
    geo = (double *)calloc((size_t)h->n_density * 4, sizeof(double));
    inert = (unsigned char *)calloc((size_t)h->n_density, 1);
    if (!h->recqm || !h->exlistm || !h->wfrag || !h->rec28 || !qd || !geo || !inert) {
        free(qd);
        free(geo);
        free(inert);
        ssw_set_error("out of memory building the MFMA scan records");
        return -1;
    }
    for (cbf = 0; cbf < ncbf; ++cbf) {
        uint32_t *xl = h->exlistm + (size_t)cbf * SSW_EXLIST_STRIDE;
        float *d0rec = h->recd0 + (size_t)cbf * SSW_REC_FLOATS;
        const float d0 = d0rec[0];
        int s = 0, ec = 0, round;
        memset(inert, 0, (size_t)h->n_density);
        memset(qd, 0, sizeof(double) * (size_t)h->n_density * SSW_REC_FLOATS);
        for (d = 0; d < h->n_density; ++d) {
            const float *r = h->rec + ((size_t)cbf * h->n_density + d) * SSW_REC_FLOATS;
            double *q = qd + (size_t)d * SSW_REC_FLOATS, *g = geo + (size_t)d * 4;
            const double det = r[SSW_REC_DET], delta = det - (double)d0;
            double R = 0.0, mw = 0.0, bias0;
            int finite = isfinite(det);
            for (j = 0; j < SSW_MAX_VECLEN; ++j) {
                double mean = r[j], var = r[SSW_REC_VAR + j];
                R += fabs(var) * mean * mean;
                finite = finite && isfinite(mean) && isfinite(var) && var >= 0.0;
                /* (as floats: these are the values whose parts the matrix cores multiply) */
                q[j] = (double)(float)(2.0 * var * mean);
                q[SSW_REC_VAR + j] = (double)(float)(-var);
                if (fabs(q[j]) > mw)
                    mw = fabs(q[j]);
                if (fabs(q[SSW_REC_VAR + j]) > mw)
                    mw = fabs(q[SSW_REC_VAR + j]);
            }
            g[0] = delta, g[1] = R, g[2] = det, g[3] = mw;
            /* intrinsically too ill-conditioned for the scan whatever the scale */
            bias0 = 1.05 * u24
                * ((4.0 * SSW_MFMA_K0 + 18.0) * fabs(delta) + (6.0 * SSW_MFMA_K0 + 2.0) * R
                   + 14.0 * fabs(det));
            if (!finite || !(bias0 <= SSW_MFMA_MAX_BIAS) || !(mw < 1.0e30))
                inert[d] = 1;
        }
        /* the scale: the largest |a|, |b| of the live densities just fits 2^15; a density that
         * fails at that scale only because of its lost second parts is what the scale-setter
         * costs, and the scale-setter goes on the exact-form list instead */
        for (round = 0; round <= h->n_density; ++round) {
            double mw = 0.0, mc = 0.0;
            int setter = -1, n_fail = 0;
            for (d = 0; d < h->n_density; ++d)
                if (!inert[d]) {
                    const double *g = geo + (size_t)d * 4;
                    if (g[3] > mw) {
                        mw = g[3];
                        setter = d;
                    }
                    /* |c| <= |delta| + R + bias */
                    if (fabs(g[0]) + g[1] + SSW_MFMA_MAX_BIAS > mc)
                        mc = fabs(g[0]) + g[1] + SSW_MFMA_MAX_BIAS;
                }
            s = 0;
            if (mw > 0.0) {
                (void)frexp(mw / 32768.0, &s); /* mw / 32768 = f 2^s, f in [0.5, 1): mw 2^-s <= 32768 */
                if (s < -8)
                    s = -8;
            }
            ec = 0;
            if (mc > 0.0) {
                (void)frexp(ldexp(mc, -s) / 32768.0, &ec);
                if (ec < 0)
                    ec = 0;
                if (ec > 15)
                    ec = 15;
            }
            for (d = 0; d < h->n_density; ++d)
                if (!inert[d]) {
                    const double *g = geo + (size_t)d * 4;
                    double *q = qd + (size_t)d * SSW_REC_FLOATS;
                    double K_i, add, bias;
                    q[SSW_REC_DET] = g[0] - g[1]; /* c without its bias */
                    if (mfma_density_terms(q, s, ec, &K_i, &add) < 0 || K_i > SSW_MFMA_K) {
                        ++n_fail;
                        continue;
                    }
                    bias = 1.05
                        * (u24
                               * ((4.0 * K_i + 18.0) * fabs(g[0]) + (6.0 * K_i + 2.0) * g[1]
                                  + 14.0 * fabs(g[2]))
                           + add);
                    if (!(bias <= SSW_MFMA_MAX_BIAS))
                        ++n_fail;
                }
            if (n_fail == 0 || setter < 0)
                break;
            /* would the others pass without the scale-setter?  Try: drop it and look again; when
             * the scale cannot shrink any more (s at its floor) the failures are their own */
            {
                double next = 0.0;
                int s2 = 0;
                for (d = 0; d < h->n_density; ++d)
                    if (!inert[d] && d != setter && geo[(size_t)d * 4 + 3] > next)
                        next = geo[(size_t)d * 4 + 3];
                if (next > 0.0)
                    (void)frexp(next / 32768.0, &s2);
                if (next > 0.0 && s2 < s && s > -8) {
                    inert[setter] = 1;
                    continue;
                }
            }
            /* the scale is not to blame: the failing densities go on the list themselves */
            for (d = 0; d < h->n_density; ++d)
                if (!inert[d]) {
                    const double *g = geo + (size_t)d * 4;
                    double *q = qd + (size_t)d * SSW_REC_FLOATS;
                    double K_i, add, bias;
                    q[SSW_REC_DET] = g[0] - g[1];
                    if (mfma_density_terms(q, s, ec, &K_i, &add) < 0 || K_i > SSW_MFMA_K) {
                        inert[d] = 1;
                        continue;
                    }
                    bias = 1.05
                        * (u24
                               * ((4.0 * K_i + 18.0) * fabs(g[0]) + (6.0 * K_i + 2.0) * g[1]
                                  + 14.0 * fabs(g[2]))
                           + add);
                    if (!(bias <= SSW_MFMA_MAX_BIAS))
                        inert[d] = 1;
                }
            /* (the scale may now be larger than the survivors need: one more look) */
        }
        d0rec[1] = (float)ldexp(1.0, s);   /* key = key' * this */
        d0rec[2] = (float)ldexp(1.0, -s);  /* key' = key * this (exact-form densities) */
        d0rec[3] = (float)ldexp(1.0, ec);  /* the constant's slot of X */
        for (d = 0; d < h->n_density; ++d) {
            float *q = h->recqm + ((size_t)cbf * h->n_density + d) * SSW_REC_FLOATS;
            const double *g = geo + (size_t)d * 4;
            double *qq = qd + (size_t)d * SSW_REC_FLOATS;
            double K_i = 0.0, add = 0.0, bias, cc;
            float cf;
            if (!inert[d]) {
                qq[SSW_REC_DET] = g[0] - g[1];
                if (mfma_density_terms(qq, s, ec, &K_i, &add) < 0 || K_i > SSW_MFMA_K)
                    inert[d] = 1; /* (cannot happen after the loop above; kept as a guard) */
            }
            if (inert[d]) {
                xl[1 + xl[0]++] = (uint32_t)d;
                q[SSW_REC_DET] = -3.0e38f; /* a = b = 0: the key stays out of the way */
                ++h->n_exact_form_m;
                continue;
            }
            bias = 1.05
                * (u24
                       * ((4.0 * K_i + 18.0) * fabs(g[0]) + (6.0 * K_i + 2.0) * g[1]
                          + 14.0 * fabs(g[2]))
                   + add);
            for (j = 0; j < SSW_MAX_VECLEN; ++j) {
                q[j] = (float)qq[j];
                q[SSW_REC_VAR + j] = (float)qq[SSW_REC_VAR + j];
            }
            cc = g[0] - g[1] + bias;
            /* the constant as the matrix cores will see it: scaled, cut in two parts, rounded
             * UP where the cut loses something */
            {
                uint16_t pp[2];
                float cs = (float)ldexp(cc, -(s + ec));
                double back;
                int tries;
                if ((double)cs < ldexp(cc, -(s + ec)))
                    cs = nextafterf(cs, INFINITY);
                for (tries = 0; tries < 64; ++tries) {
                    f16_split2(cs, pp);
                    back = (double)f16_to_float(pp[0]) + (double)f16_to_float(pp[1]);
                    if (back >= ldexp(cc, -(s + ec)))
                        break;
                    cs = nextafterf(cs, INFINITY);
                }
                if (back < ldexp(cc, -(s + ec))) {
                    /* 64 float steps do not always reach a value the two binary16
                     * parts hold from above -- below 2^-7 the second part is a binary16
                     * subnormal on a 2^-24 grid, hundreds of float ulps wide -- and a key that
                     * is not a proven upper bound is the one failure the exact pass cannot
                     * catch.  Such a density (constant nearly cancelled: none in en-us / fr-fr,
                     * whose smallest |c'| is 0.38) goes on the exact-form list instead. */
                    inert[d] = 1;
                    xl[1 + xl[0]++] = (uint32_t)d;
                    for (j = 0; j < SSW_MAX_VECLEN; ++j)
                        q[j] = q[SSW_REC_VAR + j] = 0.0f;
                    q[SSW_REC_DET] = -3.0e38f;
                    ++h->n_exact_form_m;
                    continue;
                }
                cf = (float)ldexp(back, s + ec);
                if ((double)cf < ldexp(back, s + ec))
                    cf = nextafterf(cf, INFINITY);
                q[SSW_REC_DET] = cf; /* what the two parts add up to, unscaled (for the tests) */
                qq[SSW_REC_DET] = back; /* scaled by 2^-(s + ec): what goes into the fragments */
            }
        }
        /* A fragments: K index k of the MFMA = float slot k of the record (a at 0..12, c at 15
         * against X = 2^ec, b at 16..28 against x^2; the other slots are zero on both sides) */
        for (rb = 0; rb < 4; ++rb)
            for (kb = 0; kb < 2; ++kb)
                for (l = 0; l < 64; ++l)
                    for (e = 0; e < 8; ++e) {
                        const int dens = 32 * rb + (l & 31), k = 16 * kb + 8 * (l >> 5) + e;
                        const double *qq = qd + (size_t)dens * SSW_REC_FLOATS;
                        uint16_t parts[2] = { 0, 0 };
                        if (inert[dens]) {
                            if (k == 13 || k == 14)
                                parts[0] = 0xfbffu; /* -65504, against X = 32768 */
                        } else {
                            const float wf = k == SSW_REC_DET ? (float)qq[k]
                                                               : (float)ldexp(qq[k], -s);
                            f16_split2(wf, parts);
                        }
                        for (p = 0; p < 2; ++p)
                            h->wfrag[(size_t)cbf * SSW_WFRAG_PER_CBF
                                     + ((((size_t)rb * 2 + kb) * 2 + p) * 64 + l) * 8 + e]
                                = parts[p];
                    }
    }
    free(qd);
    free(geo);
    free(inert);
    return 0;
}

int
ssw_host_build_records(ssw_host_model_t *h)
{
    const int ncbf = h->n_cb * h->n_feat;
    const size_t nrec = (size_t)ncbf * h->n_density;
    const double u24 = 1.0 / 16777216.0;
    const float *mp = h->mean, *vp = h->var;
    float *dets;
    int c, f, d, j, cbf;

    if (h->n_density > SSW_EXLIST_STRIDE - 1) {
        ssw_set_error("%d densities per codebook: at most %d are supported", h->n_density,
                      SSW_EXLIST_STRIDE - 1);
        return -1;
    }
    /* before any record is written: a record has SSW_MAX_VECLEN slots per table */
    for (f = 0; f < h->n_feat; ++f)
        if (h->veclen[f] > SSW_MAX_VECLEN) {
            ssw_set_error("stream %d has %d dimensions; the gfx950 kernels handle <= %d", f,
                          h->veclen[f], SSW_MAX_VECLEN);
            return -1;
        }
    h->rec = (float *)table_zeroed(h->rec, nrec * SSW_REC_FLOATS, sizeof(float));
    h->recq = (float *)table_zeroed(h->recq, nrec * SSW_REC_FLOATS, sizeof(float));
    h->recd0 = (float *)table_zeroed(h->recd0, (size_t)ncbf * SSW_REC_FLOATS, sizeof(float));
    h->exlist = (uint32_t *)table_zeroed(h->exlist, (size_t)ncbf * SSW_EXLIST_STRIDE,
                                         sizeof(uint32_t));
    dets = (float *)malloc(sizeof(float) * (size_t)h->n_density);
    if (!h->rec || !h->recq || !h->recd0 || !h->exlist || !dets) {
        free(dets);
        ssw_set_error("out of memory building the Gaussian records");
        return -1;
    }
    for (c = 0; c < h->n_cb; ++c)
        for (f = 0; f < h->n_feat; ++f)
            for (d = 0; d < h->n_density; ++d) {
                float *r = h->rec + (((size_t)c * h->n_feat + f) * h->n_density + d) * SSW_REC_FLOATS;
                for (j = 0; j < h->veclen[f]; ++j) {
                    r[j] = *mp++;
                    r[SSW_REC_VAR + j] = *vp++;
                }
                r[SSW_REC_DET] = h->det[((size_t)c * h->n_feat + f) * h->n_density + d];
            }
    h->n_exact_form = 0;
    for (cbf = 0; cbf < ncbf; ++cbf) {
        uint32_t *xl = h->exlist + (size_t)cbf * SSW_EXLIST_STRIDE;
        float d0;
        for (d = 0; d < h->n_density; ++d)
            dets[d] = h->rec[((size_t)cbf * h->n_density + d) * SSW_REC_FLOATS + SSW_REC_DET];
        qsort(dets, (size_t)h->n_density, sizeof(float), cmp_float);
        d0 = dets[h->n_density / 2];
        h->recd0[(size_t)cbf * SSW_REC_FLOATS] = d0;
        for (d = 0; d < h->n_density; ++d) {
            const float *r = h->rec + ((size_t)cbf * h->n_density + d) * SSW_REC_FLOATS;
            float *q = h->recq + ((size_t)cbf * h->n_density + d) * SSW_REC_FLOATS;
            const double det = r[SSW_REC_DET], delta = det - (double)d0;
            double R = 0.0, bias, cc;
            int finite = isfinite(det);
            float cf;
            for (j = 0; j < SSW_MAX_VECLEN; ++j) {
                double mean = r[j], var = r[SSW_REC_VAR + j];
                R += fabs(var) * mean * mean;
                finite = finite && isfinite(mean) && isfinite(var) && var >= 0.0;
            }
            bias = 1.05 * u24 * (126.0 * fabs(delta) + 164.0 * R + 14.0 * fabs(det));
            if (!finite || !(bias <= 4.0)) {
                xl[1 + xl[0]++] = (uint32_t)d;
                q[SSW_REC_DET] = -3.0e38f; /* a = b = 0: the key stays out of the way */
                ++h->n_exact_form;
                continue;
            }
            for (j = 0; j < SSW_MAX_VECLEN; ++j) {
                q[j] = (float)(2.0 * (double)r[SSW_REC_VAR + j] * (double)r[j]);
                q[SSW_REC_VAR + j] = -r[SSW_REC_VAR + j];
            }
            cc = delta - R + bias;
            cf = (float)cc;
            if ((double)cf < cc)
                cf = nextafterf(cf, INFINITY);
            q[SSW_REC_DET] = cf;
        }
    }
    free(dets);
    return ssw_host_build_mfma_records(h);
}


/* The scorer acmod_load_am would choose without senmgau (src/acmod.c:101-119: ptm, then
 * s2_semi, then ms): PTM when the codebooks number the CI phones and are at most 256
 * (src/ptm_mgau.c:760-768), else S2_SEMI for a single codebook (src/s2_semi_mgau.c:942), else
 * MS.  Before the mixture weights are read only the shape decides. */
int
ssw_host_scorer(const ssw_host_model_t *h)
{
    if (h->n_cb == h->n_ciphone && h->n_cb <= 256)
        return SSW_SCORER_PTM;
    if (h->n_cb == 1)
        return SSW_SCORER_S2_SEMI;
    return SSW_SCORER_MS;
}

/* The s2_semi kernels' Gaussian table (ssw_k10_semi.inc): per stream SSW_SC_ROWS rows of
 * SSW_SC_MAX_DENSITY floats, density-minor so that a wave's lanes read neighbouring densities:
 *   row j < 32  mean of dimension j     row 32 + j  scale 1 / (2 var) of dimension j     row 64  det
 * Unused dimensions and densities are 0.0f (the kernels walk veclen dimensions and n_density
 * densities only). */
static int
build_semi_records(ssw_host_model_t *h)
{
    const float *mp = h->mean, *vp = h->var;
    /* (the loader takes a topn outside 1 .. n_density for n_density) */
    const int topn = h->cfg.topn < 1 || h->cfg.topn > h->n_density ? h->n_density : h->cfg.topn;
    int f, d, j;

    if (topn > SSW_SC_MAX_TOPN) {
        ssw_set_error("s2_semi scorer: topn %d, at most %d is supported", topn, SSW_SC_MAX_TOPN);
        return -1;
    }
    if (h->n_density > SSW_SC_MAX_DENSITY) {
        ssw_set_error("s2_semi scorer: %d densities, at most %d are supported", h->n_density,
                      SSW_SC_MAX_DENSITY);
        return -1;
    }
    if (h->n_feat > SSW_MAX_FEAT) {
        ssw_set_error("s2_semi scorer: %d streams, at most %d are supported", h->n_feat,
                      SSW_MAX_FEAT);
        return -1;
    }
    for (f = 0; f < h->n_feat; ++f)
        if (h->veclen[f] > SSW_SC_MAX_VECLEN) {
            ssw_set_error("s2_semi scorer: stream %d has %d dimensions, at most %d are supported",
                          f, h->veclen[f], SSW_SC_MAX_VECLEN);
            return -1;
        }
    h->sc_rec = (float *)table_zeroed(h->sc_rec, (size_t)h->n_feat * SSW_SC_ROWS * SSW_SC_MAX_DENSITY,
                                      sizeof(float));
    if (h->sc_rec == NULL) {
        ssw_set_error("out of memory building the s2_semi records");
        return -1;
    }
    for (f = 0; f < h->n_feat; ++f) {
        float *r = h->sc_rec + (size_t)f * SSW_SC_ROWS * SSW_SC_MAX_DENSITY;
        for (d = 0; d < h->n_density; ++d) {
            for (j = 0; j < h->veclen[f]; ++j) {
                r[(size_t)j * SSW_SC_MAX_DENSITY + d] = *mp++;
                r[(size_t)(SSW_SC_MAX_VECLEN + j) * SSW_SC_MAX_DENSITY + d] = *vp++;
            }
            r[(size_t)(2 * SSW_SC_MAX_VECLEN) * SSW_SC_MAX_DENSITY + d]
                = h->det[(size_t)f * h->n_density + d];
        }
    }
    return 0;
}

/* n_sen of a mixture-weights file's header (a model without an mdef), 0 when it cannot be read:
 * load_mixw reports why */
static int32_t
peek_mixw_senones(const char *path)
{
    rd_t r;
    int32_t dims[4] = { 0, 0, 0, 0 };

    if (rd_open(&r, path) < 0)
        return 0;
    if (rd_s3_header(&r) < 0 || rd_words(&r, dims, 4) < 0)
        dims[0] = 0;
    rd_close(&r);
    return dims[0] > 0 ? dims[0] : 0;
}

/* The table of ssw_k11_cont.inc, senone-minor so that a wave's lanes (one per senone) read
 * neighbouring addresses.  Stream f starts cont_off[f] floats in; its density d takes
 * 2 veclen[f] + 1 rows of cont_sp floats:
 *   rows 2 j, 2 j + 1  (mean, scale 1 / (2 var)) of dimension j as pairs, [cont_sp][2]
 *   row 2 veclen[f]    det, [cont_sp]
 * Senones past n_sen are 0.0f (no lane reads them). */
static int
build_cont_records(ssw_host_model_t *h)
{
    /* (the loader takes a topn outside 1 .. n_density for n_density: every density, no selection) */
    const int topn = h->cfg.topn < 1 || h->cfg.topn > h->n_density ? h->n_density : h->cfg.topn;
    const size_t sp = ((size_t)h->n_cb + 63) & ~(size_t)63;
    const float *mp = h->mean, *vp = h->var, *dp = h->det;
    size_t total = 0;
    int c, f, d, j;

    if (h->n_cb > 32767) {
        ssw_set_error("continuous model: %d senones, at most 32767 are supported", h->n_cb);
        return -1;
    }
    if (h->n_feat > SSW_MAX_FEAT) {
        ssw_set_error("continuous model: %d streams, at most %d are supported", h->n_feat,
                      SSW_MAX_FEAT);
        return -1;
    }
    for (f = 0; f < h->n_feat; ++f)
        if (h->veclen[f] > SSW_CONT_MAX_VECLEN) {
            ssw_set_error("continuous model: stream %d has %d dimensions, at most %d are supported",
                          f, h->veclen[f], SSW_CONT_MAX_VECLEN);
            return -1;
        }
    if (h->n_density > SSW_CONT_MAX_DENSITY) {
        ssw_set_error("continuous model: %d densities, at most %d are supported", h->n_density,
                      SSW_CONT_MAX_DENSITY);
        return -1;
    }
    if (topn > SSW_CONT_MAX_TOPN && topn < h->n_density) {
        ssw_set_error("continuous model: topn %d, at most %d or all %d densities are supported",
                      topn, SSW_CONT_MAX_TOPN, h->n_density);
        return -1;
    }
    for (f = 0; f < h->n_feat; ++f) {
        h->cont_off[f] = total;
        total += sp * (size_t)h->n_density * (2 * (size_t)h->veclen[f] + 1);
    }
    h->cont_sp = (int32_t)sp;
    h->cont_floats = total;
    h->cont_rec = (float *)table_zeroed(h->cont_rec, total, sizeof(float));
    if (h->cont_rec == NULL) {
        ssw_set_error("out of memory building the continuous model's table (%zu bytes)",
                      total * sizeof(float));
        return -1;
    }
    for (c = 0; c < h->n_cb; ++c)
        for (f = 0; f < h->n_feat; ++f) {
            const size_t vl = (size_t)h->veclen[f];
            for (d = 0; d < h->n_density; ++d) {
                float *r = h->cont_rec + h->cont_off[f] + (size_t)d * (2 * vl + 1) * sp;
                for (j = 0; j < h->veclen[f]; ++j) {
                    r[2 * ((size_t)j * sp + (size_t)c)] = *mp++;
                    r[2 * ((size_t)j * sp + (size_t)c) + 1] = *vp++;
                }
                r[2 * vl * sp + (size_t)c] = *dp++;
            }
        }
    return 0;
}

/* The table of cont_listed_kernel (ssw_k11_cont.inc), senone-major so that the data of a listed
 * senone is whole contiguous records: the layout is stated at ssw_host_model_t::cont_rec_sm.  The
 * floats are those of build_cont_records (the same mean, var and det arrays, file order). */
int
ssw_host_build_cont_sm(ssw_host_model_t *h)
{
    const float *mp = h->mean, *vp = h->var, *dp = h->det;
    const size_t nd = (size_t)h->n_density;
    size_t per_sen = 0, total;
    float *tab;
    int c, f, d, j;

    if (!h->continuous || h->cont_rec == NULL) {
        ssw_set_error("the senone-major table is a continuous model's");
        return -1;
    }
    for (f = 0; f < h->n_feat; ++f) {
        h->cont_sm_off[f] = per_sen;
        per_sen += (nd * (2 * (size_t)h->veclen[f] + 1) + 1) & ~(size_t)1;
    }
    total = per_sen * (size_t)h->n_cb;
    tab = (float *)table_zeroed(h->cont_rec_sm, total, sizeof(float));
    if (tab == NULL) {
        ssw_set_error("out of memory building the continuous model's senone-major table (%zu bytes)",
                      total * sizeof(float));
        return -1;
    }
    h->cont_rec_sm = tab;
    h->cont_sm_sen = per_sen;
    h->cont_sm_floats = total;
    for (c = 0; c < h->n_cb; ++c)
        for (f = 0; f < h->n_feat; ++f) {
            const size_t vl = (size_t)h->veclen[f];
            float *r = tab + (size_t)c * per_sen + h->cont_sm_off[f];
            for (d = 0; d < h->n_density; ++d) {
                for (j = 0; j < h->veclen[f]; ++j) {
                    r[2 * ((size_t)j * nd + (size_t)d)] = *mp++;
                    r[2 * ((size_t)j * nd + (size_t)d) + 1] = *vp++;
                }
                r[2 * vl * nd + (size_t)d] = *dp++;
            }
        }
    return 0;
}

/* Everything derived from (mean, raw variance), for the loader and for ssw_host_model_apply_mllr:
 * det and the scaled variances, then the tables of the model's scorer.  A single-codebook model
 * is the s2_semi scorer's: its own table, none of the PTM scan's (records of 15 dimensions, at
 * most 131 densities); a continuous model likewise has its own.  Mixture weights, sen2cb, the
 * transition matrices and the log-add tables do not depend on the Gaussians. */
int
ssw_host_derive_tables(ssw_host_model_t *h)
{
    lbase_t lb;

    lb.base = h->cfg.logbase;
    lb.inv_ln_base = 1.0 / log(h->cfg.logbase);
    precompute_gaussians(h, &lb);
    if (h->continuous) {
        if (build_cont_records(h) < 0)
            return -1;
        /* (the second table only once it was asked for: ssw_model_enable_active) */
        return h->cont_rec_sm != NULL ? ssw_host_build_cont_sm(h) : 0;
    }
    if (ssw_host_scorer(h) == SSW_SCORER_S2_SEMI)
        return build_semi_records(h);
    return ssw_host_build_records(h);
}

/* ---------------------------------------------------------------------------------- */
/* MLLR transforms (mllr_t, src/ps_mllr.c; gauden_mllr_transform, src/ms_gauden.c)      */
/* ---------------------------------------------------------------------------------- */
/* a transform of n_feat streams that have no arrays yet (mllr_alloc_stream) */
static ssw_mllr_t *
mllr_alloc(int n_class, int n_feat)
{
    ssw_mllr_t *t = (ssw_mllr_t *)calloc(1, sizeof(*t));

    if (t != NULL) {
        t->refcnt = 1;
        t->n_class = n_class;
        t->veclen = (int *)calloc((size_t)n_feat, sizeof(int));
        t->A = (float ****)calloc((size_t)n_feat, sizeof(float ***));
        t->b = (float ***)calloc((size_t)n_feat, sizeof(float **));
        t->h = (float ***)calloc((size_t)n_feat, sizeof(float **));
        if (t->veclen && t->A && t->b && t->h) {
            t->n_feat = n_feat; /* (ssw_mllr_free walks n_feat streams) */
            return t;
        }
    }
    ssw_mllr_free(t);
    ssw_set_error("out of memory for an MLLR transform");
    return NULL;
}

/* stream f's arrays, laid out as ckd_calloc_3d / ckd_calloc_2d lay them out: the numbers in one
 * block (A[f][0][0], b[f][0], h[f][0]), A's row pointers in one block (A[f][0]) */
static int
mllr_alloc_stream(ssw_mllr_t *t, int f, int veclen)
{
    const size_t vl = (size_t)veclen, nc = (size_t)t->n_class;
    float *a = (float *)calloc(nc * vl * vl, sizeof(float));
    float *b = (float *)calloc(nc * vl, sizeof(float)), *h = (float *)calloc(nc * vl, sizeof(float));
    float **rows = (float **)calloc(nc * vl, sizeof(float *));
    size_t c, l;

    t->A[f] = (float ***)calloc(nc, sizeof(float **));
    t->b[f] = (float **)calloc(nc, sizeof(float *));
    t->h[f] = (float **)calloc(nc, sizeof(float *));
    if (!a || !b || !h || !rows || !t->A[f] || !t->b[f] || !t->h[f]) {
        free(a);
        free(b);
        free(h);
        free(rows);
        free(t->A[f]);
        free(t->b[f]);
        free(t->h[f]);
        t->A[f] = NULL;
        t->b[f] = t->h[f] = NULL;
        ssw_set_error("out of memory for an MLLR transform");
        return -1;
    }
    t->veclen[f] = veclen;
    for (c = 0; c < nc; ++c) {
        t->A[f][c] = rows + c * vl;
        for (l = 0; l < vl; ++l)
            t->A[f][c][l] = a + (c * vl + l) * vl;
        t->b[f][c] = b + c * vl;
        t->h[f][c] = h + c * vl;
    }
    return 0;
}

/* the limits a transform has whatever the model: -1 and ssw_set_error, naming `who` */
static int
mllr_check_counts(const char *who, int n_class, int n_feat)
{
    if (n_class < 1) {
        ssw_set_error("%s: %d MLLR classes, at least one is needed", who, n_class);
        return -1;
    }
    if (n_feat < 1 || n_feat > SSW_MAX_FEAT) {
        ssw_set_error("%s: %d feature streams, 1 to %d are supported", who, n_feat, SSW_MAX_FEAT);
        return -1;
    }
    return 0;
}

static int
mllr_check_veclen(const char *who, int f, int veclen)
{
    if (veclen >= 1 && veclen <= SSW_CONT_MAX_VECLEN)
        return 0;
    ssw_set_error("%s: stream %d has %d dimensions, 1 to %d are supported", who, f, veclen,
                  SSW_CONT_MAX_VECLEN);
    return -1;
}

ssw_mllr_t *
ssw_mllr_create(int32_t n_class, int32_t n_feat, const int32_t *veclen, const float *const *A,
                const float *const *b, const float *const *h)
{
    ssw_mllr_t *t;
    int f;

    if (veclen == NULL || A == NULL || b == NULL || h == NULL) {
        ssw_set_error("ssw_mllr_create: NULL argument");
        return NULL;
    }
    if (mllr_check_counts("ssw_mllr_create", n_class, n_feat) < 0)
        return NULL;
    for (f = 0; f < n_feat; ++f)
        if (mllr_check_veclen("ssw_mllr_create", f, veclen[f]) < 0)
            return NULL;
    if ((t = mllr_alloc(n_class, n_feat)) == NULL)
        return NULL;
    for (f = 0; f < n_feat; ++f) {
        const size_t v = (size_t)veclen[f], nc = (size_t)n_class;
        if (mllr_alloc_stream(t, f, veclen[f]) < 0) {
            ssw_mllr_free(t);
            return NULL;
        }
        memcpy(t->A[f][0][0], A[f], sizeof(float) * nc * v * v);
        memcpy(t->b[f][0], b[f], sizeof(float) * nc * v);
        memcpy(t->h[f][0], h[f], sizeof(float) * nc * v);
    }
    return t;
}

/* `count` numbers as mllr_read reads them ("%f "); -1 with the message set */
static int
mllr_read_floats(FILE *fp, const char *path, const char *what, int f, int c, float *dst,
                 size_t count)
{
    size_t i;
    for (i = 0; i < count; ++i)
        if (fscanf(fp, "%f ", &dst[i]) != 1) {
            ssw_set_error("%s: short file: cannot read the MLLR %s of stream %d, class %d "
                          "(number %zu of %zu)", path, what, f, c, i, count);
            return -1;
        }
    return 0;
}

/* mllr_read (src/ps_mllr.c:47-127): whitespace-separated numbers -- n_class, n_feat, then per
 * stream its veclen and per class A[veclen][veclen], b[veclen], h[veclen] as %f */
ssw_mllr_t *
ssw_mllr_read(const char *path)
{
    FILE *fp;
    ssw_mllr_t *t = NULL;
    int n_class = 0, n_feat = 0, f, c, n;

    if (path == NULL) {
        ssw_set_error("ssw_mllr_read: NULL path");
        return NULL;
    }
    if ((fp = fopen(path, "r")) == NULL) {
        ssw_set_error("%s: cannot open the MLLR file for reading", path);
        return NULL;
    }
    if (fscanf(fp, "%d", &n_class) != 1) {
        ssw_set_error("%s: cannot read the number of MLLR classes", path);
        goto bad;
    }
    if (n_class >= 1 && fscanf(fp, "%d", &n_feat) != 1) {
        ssw_set_error("%s: short file: cannot read the number of feature streams", path);
        goto bad;
    }
    if (mllr_check_counts(path, n_class, n_feat) < 0 || (t = mllr_alloc(n_class, n_feat)) == NULL)
        goto bad;
    for (f = 0; f < n_feat; ++f) {
        if (fscanf(fp, "%d", &n) != 1) {
            ssw_set_error("%s: short file: cannot read the length of stream %d", path, f);
            goto bad;
        }
        if (mllr_check_veclen(path, f, n) < 0 || mllr_alloc_stream(t, f, n) < 0)
            goto bad;
        for (c = 0; c < n_class; ++c)
            if (mllr_read_floats(fp, path, "rotation", f, c, t->A[f][c][0], (size_t)n * n) < 0
                || mllr_read_floats(fp, path, "bias", f, c, t->b[f][c], (size_t)n) < 0
                || mllr_read_floats(fp, path, "variance scale", f, c, t->h[f][c], (size_t)n) < 0)
                goto bad;
    }
    fclose(fp);
    return t;
bad:
    fclose(fp);
    ssw_mllr_free(t);
    return NULL;
}

ssw_mllr_t *
ssw_mllr_retain(ssw_mllr_t *t)
{
    if (t != NULL)
        ++t->refcnt;
    return t;
}

int
ssw_mllr_free(ssw_mllr_t *t)
{
    int f;

    if (t == NULL)
        return 0;
    if (--t->refcnt > 0)
        return t->refcnt;
    for (f = 0; f < t->n_feat; ++f) {
        if (t->A && t->A[f]) { /* (a stream mllr_alloc_stream made has all of its blocks) */
            free(t->A[f][0][0]);
            free(t->A[f][0]);
            free(t->A[f]);
            free(t->b[f][0]);
            free(t->b[f]);
            free(t->h[f][0]);
            free(t->h[f]);
        }
    }
    free(t->veclen);
    free(t->A);
    free(t->b);
    free(t->h);
    free(t->cb2mllr);
    free(t);
    return 0;
}

/* what gauden_mllr_transform does not ask (it reads out of bounds instead): does the transform
 * fit the model, and is every number of class 0 -- the one class it uses -- finite */
static int
mllr_check(const ssw_host_model_t *h, const ssw_mllr_t *t)
{
    int f, l, m;

    if (t->n_class < 1) {
        ssw_set_error("MLLR transform: %d classes, at least one is needed", t->n_class);
        return -1;
    }
    if (t->n_feat != h->n_feat) {
        ssw_set_error("MLLR transform: %d feature streams, the model has %d", t->n_feat, h->n_feat);
        return -1;
    }
    if (t->veclen == NULL || t->A == NULL || t->b == NULL || t->h == NULL) {
        ssw_set_error("MLLR transform: an array is missing");
        return -1;
    }
    for (f = 0; f < h->n_feat; ++f)
        if (t->veclen[f] != h->veclen[f]) {
            ssw_set_error("MLLR transform: stream %d has %d dimensions, the model's has %d", f,
                          t->veclen[f], h->veclen[f]);
            return -1;
        }
    for (f = 0; f < h->n_feat; ++f)
        for (l = 0; l < h->veclen[f]; ++l) {
            int finite = isfinite(t->b[f][0][l]) && isfinite(t->h[f][0][l]);
            for (m = 0; m < h->veclen[f]; ++m)
                finite = finite && isfinite(t->A[f][0][l][m]);
            if (!finite) {
                ssw_set_error("MLLR transform: a non-finite number in row %d of stream %d", l, f);
                return -1;
            }
        }
    return 0;
}

int
ssw_host_model_apply_mllr(ssw_host_model_t *h, const ssw_mllr_t *t)
{
    const size_t n = (size_t)h->n_cb * h->n_density * (size_t)h->veclen_total;
    double temp[SSW_CONT_MAX_VECLEN];
    float *mp, *vp;
    int c, f, d, l, m;

    if (t != NULL && mllr_check(h, t) < 0)
        return -1;
    /* the parameters as read: a transform is never applied on top of an earlier one */
    memcpy(h->mean, h->mean0, sizeof(float) * n);
    memcpy(h->var, h->var0, sizeof(float) * n);
    mp = h->mean;
    vp = h->var;
    for (c = 0; t != NULL && c < h->n_cb; ++c)
        for (f = 0; f < h->n_feat; ++f) {
            const int vl = h->veclen[f];
            float **A = t->A[f][0];
            const float *b = t->b[f][0], *hs = t->h[f][0];
            for (d = 0; d < h->n_density; ++d, mp += vl, vp += vl) {
                /* float32 products (no contraction), summed in float64 in index order from 0.0,
                 * then + b; every temp before any mean is overwritten */
                for (l = 0; l < vl; ++l) {
                    temp[l] = 0.0;
                    for (m = 0; m < vl; ++m) {
                        const float prod = A[l][m] * mp[m];
                        temp[l] += prod;
                    }
                    temp[l] += b[l];
                }
                for (l = 0; l < vl; ++l) {
                    mp[l] = (float)temp[l];
                    vp[l] *= hs[l];
                }
            }
        }
    if (ssw_host_derive_tables(h) < 0)
        return -1;
    ++h->mllr_generation;
    return 0;
}

ssw_host_model_t *
ssw_host_model_load(const char *mdef, const char *means, const char *variances,
                    const char *sendump, const char *mixw, const char *tmat,
                    const ssw_config_t *cfg)
{
    ssw_host_model_t *h = (ssw_host_model_t *)calloc(1, sizeof(*h));
    lbase_t lb;
    int i, n;
    int32_t n_sen_known;

    if (h == NULL)
        return NULL;
    if (cfg)
        h->cfg = *cfg;
    else
        ssw_config_defaults(&h->cfg);
    if (!(h->cfg.logbase > 1.0)) {
        ssw_set_error("logbase must be > 1");
        goto bad;
    }
    lb.base = h->cfg.logbase;
    lb.inv_ln_base = 1.0 / log(h->cfg.logbase);
    n = build_logadd8(&lb, SSW_SENSCR_SHIFT, h->logadd8);
    if (n < 0) { /* same refusal as src/ptm_mgau.c:739-743 */
        ssw_set_error("log base %f too small for an 8-bit add table", h->cfg.logbase);
        goto bad;
    }
    h->logadd8_size = n;
    h->zero8 = (int32_t)0x80000000 >> (SSW_SENSCR_SHIFT + 2);

    if (means == NULL || variances == NULL) {
        ssw_set_error("means and variances are required");
        goto bad;
    }
    if (mdef && load_mdef(h, mdef) < 0)
        goto bad;
    if (read_gaussians(h, means, variances) < 0)
        goto bad;
    /* the senones: the mdef's, or without one the mixture-weights file's */
    n_sen_known = h->n_sen;
    if (n_sen_known == 0 && mixw != NULL)
        n_sen_known = peek_mixw_senones(mixw);
    /* The codebooks number the senones, and are neither one nor the CI phones (those shapes are
     * s2_semi's and PTM's, as the order of attempts in acmod_load_am makes them, src/acmod.c:
     * 101-119): a continuous-density model, the ms scorer with the .cont. map (src/ms_senone.c:
     * 238-250).  It needs its mixture_weights file (src/ms_mgau.c:208-212). */
    if (ssw_host_scorer(h) == SSW_SCORER_MS && n_sen_known > 0) {
        if (h->n_cb == n_sen_known && mixw != NULL) {
            if (sendump != NULL) {
                ssw_set_error("continuous model (%d codebooks for %d senones): a sendump cannot be "
                              "used, the ms scorer reads mixture_weights", h->n_cb, n_sen_known);
                goto bad;
            }
            h->continuous = 1;
        } else if (h->n_cb > n_sen_known) {
            ssw_set_error("%d codebooks for %d senones: more codebooks than senones", h->n_cb,
                          n_sen_known);
            goto bad;
        } else if (h->n_cb < n_sen_known) {
            ssw_set_error("%d codebooks for %d senones: fewer codebooks than senones, and neither "
                          "one codebook nor one per CI phone (%d)", h->n_cb, n_sen_known,
                          h->n_ciphone);
            goto bad;
        }
    }
    if (ssw_host_derive_tables(h) < 0)
        goto bad;
    if (tmat && load_tmat(h, &lb, tmat) < 0)
        goto bad;
    if (sendump) {
        if (h->n_sen == 0) {
            ssw_set_error("a sendump needs the mdef for its senone count");
            goto bad;
        }
        if (load_sendump(h, sendump) < 0)
            goto bad;
    }
    if (mixw && load_mixw(h, &lb, mixw, sendump == NULL && !h->continuous) < 0)
        goto bad;
    if (h->continuous) { /* the .cont. map: senone s has codebook s (src/ms_senone.c:238-250) */
        int16_t *map = (int16_t *)realloc(h->sen2cb, sizeof(int16_t) * (size_t)h->n_sen);
        if (map == NULL) {
            ssw_set_error("out of memory");
            goto bad;
        }
        h->sen2cb = map;
        for (i = 0; i < h->n_sen; ++i)
            h->sen2cb[i] = (int16_t)i;
    }
    if (h->sen2cb == NULL && h->n_sen) {
        ssw_set_error("senone to codebook map needs the mdef");
        goto bad;
    }
    for (i = 0; i < h->n_sen && ssw_host_scorer(h) != SSW_SCORER_S2_SEMI; ++i)
        if (h->sen2cb[i] < 0 || h->sen2cb[i] >= h->n_cb) {
            /* PTM needs one codebook per CI phone (src/ptm_mgau.c:760-764) */
            ssw_set_error("senone %d maps to codebook %d of %d", i, h->sen2cb[i], h->n_cb);
            goto bad;
        }
    if (h->cfg.topn < 1 || h->cfg.topn > h->n_density)
        h->cfg.topn = h->n_density;
    /* the front end's settings: feat_params.json in the model directory (the means file's), as
     * acmod reads it; a file that cannot be used does not fail the load -- ssw_fe_batch
     * without a configuration of its own refuses with fe_err */
    ssw_fe_config_defaults(&h->fe);
    {
        const char *slash = strrchr(means, '/');
        size_t dir = slash ? (size_t)(slash - means) + 1 : 0;
        char *path = (char *)malloc(dir + sizeof("feat_params.json"));
        if (path == NULL) {
            ssw_set_error("out of memory");
            goto bad;
        }
        memcpy(path, means, dir);
        strcpy(path + dir, "feat_params.json");
        ssw_fe_strings_defaults(&h->fe_str);
        if (ssw_fe_config_read_strings(path, &h->fe, &h->fe_str, h->fe_err, sizeof(h->fe_err)) < 0) {
            ssw_fe_config_defaults(&h->fe);
            ssw_fe_strings_defaults(&h->fe_str);
            h->fe.from_file = 0;
        }
        /* the feature stage's keys of the same file; `lda` unset = the directory's
         * feature_transform, if there is one (expand_file_config, src/decoder.c:90-119) */
        ssw_feat_config_defaults(&h->feat);
        if (ssw_feat_config_read_err(path, &h->feat, h->feat_err, sizeof(h->feat_err)) < 0) {
            ssw_feat_config_defaults(&h->feat);
            h->feat.from_file = 0;
        }
        if (h->feat.lda[0] == '\0' && dir + sizeof("feature_transform") <= sizeof(h->feat.lda)) {
            FILE *lf;
            memcpy(h->feat.lda, means, dir);
            strcpy(h->feat.lda + dir, "feature_transform");
            if ((lf = fopen(h->feat.lda, "rb")) != NULL)
                fclose(lf);
            else
                h->feat.lda[0] = '\0';
        }
        free(path);
    }
    return h;
bad:
    ssw_host_model_free(h);
    return NULL;
}

void
ssw_host_model_free(ssw_host_model_t *h)
{
    if (h == NULL)
        return;
    free(h->mean);
    free(h->var);
    free(h->mean0);
    free(h->var0);
    free(h->det);
    free(h->pid_memo);
    free(h->rec);
    free(h->recq);
    free(h->recd0);
    free(h->exlist);
    free(h->recqm);
    free(h->exlistm);
    free(h->wfrag);
    free(h->rec28);
    free(h->sc_rec);
    free(h->cont_rec);
    free(h->cont_rec_sm);
    free(h->sseq);
    free(h->sen2cb);
    free(h->phone_ssid);
    free(h->phone_tmat);
    free(h->cd_tree);
    free(h->ci_filler);
    if (h->ciname) {
        int i;
        for (i = 0; i < h->n_ciphone; ++i)
            free(h->ciname[i]);
        free(h->ciname);
    }
    free(h->tp);
    free(h->ptm_mixw);
    free(h->ms_pdf);
    free(h);
}
