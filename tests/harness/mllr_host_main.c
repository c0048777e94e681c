/* Stand-alone sanitizer program for MLLR adaptation on the host (csrc/ssw_model.c): built by
 * tests/test_mllr_host_sanitizers.py with -fsanitize=address,undefined from ssw_model.c and this
 * file.
 *
 *   usage: mllr_host_main ( model DIR | ok FILE | bad FILE WORDS | unreadable FILE WORDS )...
 *       model       load the model in DIR (means, variances, mdef, transition_matrices; a sendump
 *                   or else mixture_weights) with SSW_DEVICE_NONE; it is the model of what follows
 *       ok          read FILE, apply it, apply it again (the tables must not move), retain and
 *                   release it, clear (the loaded means, variances and dets must be back)
 *       bad         FILE reads but the model refuses it with a message that holds WORDS, and its
 *                   tables do not move
 *       unreadable  FILE is refused by the parser with a message that holds WORDS
 *   Prints "ok <n> applied, <m> refused" and exits 0; exits 1 saying what went wrong. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssw_internal.h"

static ssw_host_model_t *
load(const char *dir)
{
    char p[6][600];
    ssw_config_t cfg;
    FILE *f;
    int has_dump;
    ssw_config_defaults(&cfg);
    cfg.device = SSW_DEVICE_NONE;
    snprintf(p[0], sizeof p[0], "%s/mdef", dir);
    snprintf(p[1], sizeof p[1], "%s/means", dir);
    snprintf(p[2], sizeof p[2], "%s/variances", dir);
    snprintf(p[3], sizeof p[3], "%s/sendump", dir);
    snprintf(p[4], sizeof p[4], "%s/mixture_weights", dir);
    snprintf(p[5], sizeof p[5], "%s/transition_matrices", dir);
    f = fopen(p[3], "rb");
    has_dump = f != NULL;
    if (f != NULL)
        fclose(f);
    return ssw_host_model_load(p[0], p[1], p[2], has_dump ? p[3] : NULL, has_dump ? NULL : p[4],
                               p[5], &cfg);
}

typedef struct { float *mean, *var, *det; size_t n, nd; } snap_t;

static snap_t
snapshot(const ssw_host_model_t *h)
{
    snap_t s;
    s.n = (size_t)h->n_cb * h->n_density * (size_t)h->veclen_total;
    s.nd = (size_t)h->n_cb * h->n_feat * h->n_density;
    s.mean = (float *)malloc(sizeof(float) * s.n);
    s.var = (float *)malloc(sizeof(float) * s.n);
    s.det = (float *)malloc(sizeof(float) * s.nd);
    if (!s.mean || !s.var || !s.det) {
        fprintf(stderr, "out of memory\n");
        exit(1);
    }
    memcpy(s.mean, h->mean, sizeof(float) * s.n);
    memcpy(s.var, h->var, sizeof(float) * s.n);
    memcpy(s.det, h->det, sizeof(float) * s.nd);
    return s;
}

static int
same(const ssw_host_model_t *h, const snap_t *s)
{
    return !memcmp(s->mean, h->mean, sizeof(float) * s->n)
        && !memcmp(s->var, h->var, sizeof(float) * s->n)
        && !memcmp(s->det, h->det, sizeof(float) * s->nd);
}

static void
drop(snap_t *s)
{
    free(s->mean);
    free(s->var);
    free(s->det);
}

int
main(int argc, char **argv)
{
    ssw_host_model_t *h = NULL;
    int a = 1, n_ok = 0, n_bad = 0;
    while (a < argc) {
        if (!strcmp(argv[a], "model") && a + 1 < argc) {
            ssw_host_model_free(h);
            if ((h = load(argv[a + 1])) == NULL) {
                fprintf(stderr, "%s: %s\n", argv[a + 1], ssw_last_error());
                return 1;
            }
            a += 2;
        } else if (!strcmp(argv[a], "ok") && a + 1 < argc && h != NULL) {
            ssw_mllr_t *t = ssw_mllr_read(argv[a + 1]);
            snap_t loaded = snapshot(h), once;
            const int gen = h->mllr_generation;
            if (t == NULL || ssw_host_model_apply_mllr(h, t) < 0) {
                fprintf(stderr, "%s: %s\n", argv[a + 1], ssw_last_error());
                return 1;
            }
            once = snapshot(h);
            if (ssw_mllr_retain(t) != t || ssw_mllr_free(t) != 1
                || ssw_host_model_apply_mllr(h, t) < 0 || !same(h, &once)) {
                fprintf(stderr, "%s: applying twice is not applying once\n", argv[a + 1]);
                return 1;
            }
            if (ssw_mllr_free(t) != 0 || ssw_host_model_apply_mllr(h, NULL) < 0 || !same(h, &loaded)
                || h->mllr_generation != gen + 3) {
                fprintf(stderr, "%s: clearing does not restore the loaded tables\n", argv[a + 1]);
                return 1;
            }
            drop(&loaded);
            drop(&once);
            ++n_ok;
            a += 2;
        } else if (!strcmp(argv[a], "bad") && a + 2 < argc && h != NULL) {
            ssw_mllr_t *t = ssw_mllr_read(argv[a + 1]);
            snap_t before = snapshot(h);
            if (t == NULL) {
                fprintf(stderr, "%s: %s\n", argv[a + 1], ssw_last_error());
                return 1;
            }
            if (ssw_host_model_apply_mllr(h, t) == 0 || strstr(ssw_last_error(), argv[a + 2]) == NULL
                || !same(h, &before)) {
                fprintf(stderr, "%s: not refused with \"%s\" (\"%s\"), or the model moved\n",
                        argv[a + 1], argv[a + 2], ssw_last_error());
                return 1;
            }
            ssw_mllr_free(t);
            drop(&before);
            ++n_bad;
            a += 3;
        } else if (!strcmp(argv[a], "unreadable") && a + 2 < argc) {
            ssw_mllr_t *t = ssw_mllr_read(argv[a + 1]);
            if (t != NULL || strstr(ssw_last_error(), argv[a + 2]) == NULL) {
                fprintf(stderr, "%s: not refused with \"%s\" (\"%s\")\n", argv[a + 1], argv[a + 2],
                        ssw_last_error());
                return 1;
            }
            ++n_bad;
            a += 3;
        } else {
            fprintf(stderr, "usage: mllr_host_main ( model DIR | ok FILE | bad FILE WORDS | "
                            "unreadable FILE WORDS )...\n");
            return 1;
        }
    }
    ssw_host_model_free(h);
    printf("ok %d applied, %d refused\n", n_ok, n_bad);
    return 0;
}
