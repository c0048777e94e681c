/* Stand-alone sanitizer program for the loader of continuous-density models (csrc/ssw_model.c):
 * built by tests/test_cont_host_sanitizers.py with -fsanitize=address,undefined from ssw_model.c
 * and this file.
 *
 *   usage: cont_loader_main ( ok DIR TOPN | bad DIR TOPN WORDS )...
 *       ok   the model in DIR (means, variances, mixture_weights; the mdef and the transition
 *            matrices when DIR holds an mdef) loads with topn = TOPN, is continuous, maps senone s
 *            to codebook s, and every slot of its table can be read: the means, scales and dets
 *            of the files where they belong, zeros for the senones past the last
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
    FILE *f;
    int has_mdef;
    ssw_config_defaults(&cfg);
    cfg.topn = topn;
    cfg.device = SSW_DEVICE_NONE;
    snprintf(p[0], sizeof p[0], "%s/mdef", dir);
    snprintf(p[1], sizeof p[1], "%s/means", dir);
    snprintf(p[2], sizeof p[2], "%s/variances", dir);
    snprintf(p[3], sizeof p[3], "%s/mixture_weights", dir);
    snprintf(p[4], sizeof p[4], "%s/transition_matrices", dir);
    f = fopen(p[0], "rb");
    has_mdef = f != NULL;
    if (f != NULL)
        fclose(f);
    return ssw_host_model_load(has_mdef ? p[0] : NULL, p[1], p[2], NULL, p[3],
                               has_mdef ? p[4] : NULL, &cfg);
}

static int
check_table(const ssw_host_model_t *h)
{
    const float *mp = h->mean, *vp = h->var, *dp = h->det;
    const size_t sp = (size_t)h->cont_sp;
    size_t at = 0, seen = 0;
    int c, f, d, j;
    if (h->cont_rec == NULL || h->rec != NULL || h->recq != NULL || h->wfrag != NULL
        || h->sc_rec != NULL || h->ptm_mixw != NULL || h->ms_pdf == NULL)
        return -1;
    if (sp < (size_t)h->n_sen || sp % 64 != 0 || h->n_cb != h->n_sen)
        return -1;
    for (c = 0; c < h->n_sen; ++c)
        if (h->sen2cb[c] != c)
            return -1;
    for (c = 0; c < h->n_cb; ++c)
        for (f = 0; f < h->n_feat; ++f) {
            const size_t vl = (size_t)h->veclen[f];
            for (d = 0; d < h->n_density; ++d) {
                const float *r = h->cont_rec + h->cont_off[f] + (size_t)d * (2 * vl + 1) * sp;
                for (j = 0; j < h->veclen[f]; ++j)
                    if (r[2 * ((size_t)j * sp + (size_t)c)] != *mp++
                        || r[2 * ((size_t)j * sp + (size_t)c) + 1] != *vp++)
                        return -1;
                if (r[2 * vl * sp + (size_t)c] != *dp++)
                    return -1;
            }
        }
    /* the whole table can be read, and the senones past the last are zeros */
    for (f = 0; f < h->n_feat; ++f)
        at += sp * (size_t)h->n_density * (2 * (size_t)h->veclen[f] + 1);
    if (at != h->cont_floats)
        return -1;
    for (at = 0; at < h->cont_floats; ++at)
        seen += h->cont_rec[at] != 0.0f;
    if (seen > (size_t)h->n_sen * (size_t)h->n_density * (2 * (size_t)h->veclen_total + (size_t)h->n_feat))
        return -1;
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
            if (!h->continuous || ssw_host_scorer(h) != SSW_SCORER_MS || check_table(h) < 0) {
                fprintf(stderr, "%s: not loaded as a continuous model\n", argv[a + 1]);
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
            fprintf(stderr, "usage: cont_loader_main ( ok DIR TOPN | bad DIR TOPN WORDS )...\n");
            return 1;
        }
    }
    printf("ok %d loaded, %d refused\n", n_ok, n_bad);
    return 0;
}
