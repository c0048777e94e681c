/* fe_any_host_main.c -- the host side of ssw_fe_batch_any (csrc/ssw_model.c: feat_params.json
 * with its strings, ssw_fe_resolve, ssw_fe_framing, ssw_fe_any_tables_build,
 * ssw_fe_any_rate_build, ssw_fe_dc_sum_exact) as a stand-alone program, for
 * tests/test_fe_any_host.py to run under AddressSanitizer + UBSan.
 *
 *   fe_any_host_main (ok JSON_FILE RATE F32 | bad JSON_FILE RATE WORDS)...
 *
 * ok: the settings of JSON_FILE (a feat_params.json) resolve and every table builds at RATE;
 * prints "name out_dim plain nfft n_coeffs dc" per case (dc: 0 no remove_dc, 1 any order, 2 in
 * order, for F32 = 0 int16 / 1 float32 samples) and checks every table entry is finite and every
 * filter inside the spectrum.  bad: resolving, framing or the rate's tables are refused with an
 * error that contains WORDS.  Exits 0, or 1 saying what failed. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssw_internal.h"

static void
die(const char *what, const char *arg)
{
    fprintf(stderr, "FAILED: %s (%s): %s\n", what, arg, ssw_last_error());
    exit(1);
}

/* 0 and *rate_out built, or -1 with ssw_last_error */
static int
build(const char *json, double rate, struct ssw_fe_s *fe, ssw_fe_framing_t *fr,
      ssw_fe_rate_t **rate_out)
{
    ssw_fe_config_t c;
    ssw_fe_strings_t s;
    char err[256];
    ssw_fe_config_defaults(&c);
    ssw_fe_strings_defaults(&s);
    if (ssw_fe_config_read_strings(json, &c, &s, err, sizeof(err)) != 0) {
        fprintf(stderr, "FAILED: cannot read %s: %s\n", json, err);
        exit(1);
    }
    *rate_out = NULL;
    if (ssw_fe_resolve(&c, s.warp_type, s.warp_params, fe) < 0 || ssw_fe_framing(&fe->cfg, rate, fr) < 0
        || (*rate_out = ssw_fe_any_rate_build(fe, fr)) == NULL)
        return -1;
    return 0;
}

int
main(int argc, char **argv)
{
    int i = 1, n_ok = 0, n_bad = 0;
    while (i < argc) {
        struct ssw_fe_s fe;
        ssw_fe_framing_t fr;
        ssw_fe_rate_t *r;
        if (i + 3 < argc && !strcmp(argv[i], "ok")) {
            ssw_fe_any_tables_t *t = (ssw_fe_any_tables_t *)malloc(sizeof(*t));
            const int f32 = atoi(argv[i + 3]);
            const double *ham;
            const float *coef;
            int k, dc;
            if (t == NULL || build(argv[i + 1], atof(argv[i + 2]), &fe, &fr, &r) < 0)
                die("refused", argv[i + 1]);
            ssw_fe_any_tables_build(&fe, t);
            for (k = 0; k < t->ncep * t->nfilt; ++k)
                if (!isfinite(t->mel_cosine[k]))
                    die("mel_cosine", argv[i + 1]);
            for (k = 0; k < t->ncep; ++k)
                if (!isfinite(t->lifter[k]))
                    die("lifter", argv[i + 1]);
            ham = (const double *)((const char *)r + r->hamming_off);
            coef = (const float *)((const char *)r + r->coeff_off);
            for (k = 0; k < r->frame_size / 2; ++k)
                if (!(ham[k] > 0 && ham[k] <= 1))
                    die("hamming", argv[i + 1]);
            for (k = 0; k < r->nfilt; ++k)
                if (r->spec_start[k] < 0 || r->filt_width[k] < 1
                    || r->spec_start[k] + r->filt_width[k] > r->fft_size / 2 + 1
                    || r->filt_start[k] + r->filt_width[k] > r->n_coeffs)
                    die("a filter outside the spectrum", argv[i + 1]);
            for (k = 0; k < r->n_coeffs; ++k)
                if (!isfinite(coef[k]))
                    die("filter coefficient", argv[i + 1]);
            dc = !fe.cfg.remove_dc ? SSW_FE_DC_NONE
                : ssw_fe_dc_sum_exact((float)fe.cfg.alpha, fr.frame_size, f32) ? SSW_FE_DC_ANY_ORDER
                                                                                : SSW_FE_DC_IN_ORDER;
            printf("%s %d %d %d %d %d\n", argv[i + 1], fe.out_dim, fe.plain, fr.fft_size, r->n_coeffs,
                   dc);
            free(r);
            free(t);
            ++n_ok;
            i += 4;
        } else if (i + 3 < argc && !strcmp(argv[i], "bad")) {
            if (build(argv[i + 1], atof(argv[i + 2]), &fe, &fr, &r) == 0) {
                free(r);
                die("accepted", argv[i + 1]);
            }
            if (strstr(ssw_last_error(), argv[i + 3]) == NULL)
                die("refused in other words", argv[i + 3]);
            ++n_bad;
            i += 4;
        } else {
            fprintf(stderr, "usage: fe_any_host_main (ok JSON RATE F32 | bad JSON RATE WORDS)...\n");
            return 1;
        }
    }
    printf("ok %d built, %d refused\n", n_ok, n_bad);
    return 0;
}
