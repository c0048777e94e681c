/* Stand-alone sanitizer program for the loader of single-codebook models (csrc/ssw_model.c):
 * built by tests/test_sc_host_sanitizers.py with -fsanitize=address,undefined from ssw_model.c and
 * this file.
 *
 *   usage: sc_loader_main ( ok DIR TOPN | bad DIR TOPN WORDS )...
 *       ok   the model in DIR loads with topn = TOPN, is the s2_semi scorer's, and every slot of
 *            its Gaussian table can be read: the means, scales and dets of the files where they
 *            belong, zeros elsewhere
 *       bad  it is refused, and the message holds WORDS
 *   Prints "ok <n> loaded, <m> refused" and exits 0; exits 1 saying what went wrong. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssw_internal.h"

static ssw_host_model_t *
load(const char *dir, int topn)
{
    char p[5][600];
    ssw_config_t cfg;
    ssw_config_defaults(&cfg);
    cfg.topn = topn;
    cfg.device = SSW_DEVICE_NONE;
    snprintf(p[0], sizeof p[0], "%s/mdef", dir);
    snprintf(p[1], sizeof p[1], "%s/means", dir);
    snprintf(p[2], sizeof p[2], "%s/variances", dir);
    snprintf(p[3], sizeof p[3], "%s/sendump", dir);
    snprintf(p[4], sizeof p[4], "%s/transition_matrices", dir);
    return ssw_host_model_load(p[0], p[1], p[2], p[3], NULL, p[4], &cfg);
}

static int
check_table(const ssw_host_model_t *h)
{
    const float *mp = h->mean, *vp = h->var;
    int f, d, j;
    if (h->sc_rec == NULL || h->rec != NULL || h->recq != NULL || h->wfrag != NULL)
        return -1;
    for (f = 0; f < h->n_feat; ++f) {
        const float *r = h->sc_rec + (size_t)f * SSW_SC_ROWS * SSW_SC_MAX_DENSITY;
        for (d = 0; d < SSW_SC_MAX_DENSITY; ++d)
            for (j = 0; j < SSW_SC_MAX_VECLEN; ++j) {
                const int in = d < h->n_density && j < h->veclen[f];
                const float mean = r[(size_t)j * SSW_SC_MAX_DENSITY + d];
                const float scale = r[(size_t)(SSW_SC_MAX_VECLEN + j) * SSW_SC_MAX_DENSITY + d];
                if (in ? (mean != *mp++ || scale != *vp++) : (mean != 0.0f || scale != 0.0f))
                    return -1;
            }
        for (d = 0; d < SSW_SC_MAX_DENSITY; ++d)
            if (r[(size_t)(2 * SSW_SC_MAX_VECLEN) * SSW_SC_MAX_DENSITY + d]
                != (d < h->n_density ? h->det[(size_t)f * h->n_density + d] : 0.0f))
                return -1;
    }
    return 0;
}

int
main(int argc, char **argv)
{
    int a = 1, n_ok = 0, n_bad = 0;
    while (a < argc) {
        if (!strcmp(argv[a], "ok") && a + 2 < argc) {
            ssw_host_model_t *h = load(argv[a + 1], atoi(argv[a + 2]));
            if (h == NULL) {
                fprintf(stderr, "%s: %s\n", argv[a + 1], ssw_last_error());
                return 1;
            }
            if (ssw_host_scorer(h) != SSW_SCORER_S2_SEMI || h->ptm_mixw == NULL || check_table(h) < 0) {
                fprintf(stderr, "%s: not loaded as a single-codebook model\n", argv[a + 1]);
                return 1;
            }
            ssw_host_model_free(h);
            ++n_ok;
            a += 3;
        } else if (!strcmp(argv[a], "bad") && a + 3 < argc) {
            ssw_host_model_t *h = load(argv[a + 1], atoi(argv[a + 2]));
            if (h != NULL) {
                fprintf(stderr, "%s: was not refused\n", argv[a + 1]);
                return 1;
            }
            if (strstr(ssw_last_error(), argv[a + 3]) == NULL) {
                fprintf(stderr, "%s: refused with \"%s\", not with \"%s\"\n", argv[a + 1],
                        ssw_last_error(), argv[a + 3]);
                return 1;
            }
            ++n_bad;
            a += 4;
        } else {
            fprintf(stderr, "usage: sc_loader_main ( ok DIR TOPN | bad DIR TOPN WORDS )...\n");
            return 2;
        }
    }
    printf("ok %d loaded, %d refused\n", n_ok, n_bad);
    return 0;
}
