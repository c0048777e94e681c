/* feat_types_driver.c -- the reference library's dynamic features (feat.h) over whole
 * utterances, for tests/golden/make_feat_types.py.  Our own program against the library's public
 * feat API, used the way its tests/test_feat.c uses it.
 *
 *   feat_types_driver MODE CEPIN OUT KEY=VALUE ... -- LEN LEN ...
 *       CEPIN   float32 cepstra, the utterances back to back, `ceplen` values a frame
 *       MODE    fresh: a new feat_init for every utterance (a fresh decoder each time)
 *               chain: one feat_init, the utterances in order (one decoder's utterances)
 *       KEY=VALUE  settings of config_defs.h FEAT_OPTIONS (feat, ceplen, cmn, cmninit, varnorm,
 *               lda, ldadim, svspec), through config_set_str
 *       LEN     frames of each utterance; 0 is allowed in chain mode
 *   Every utterance goes through feat_s2mfc2feat_live with beginutt = endutt = 1.  OUT receives,
 *   per utterance, LEN rows of WIDTH float32 (the first WIDTH floats of the frame's row: the
 *   subvectors' dimensions with a svspec, else feat_dimension), then -- when the configuration
 *   has a CMN -- cmn_mean[ceplen], sum[ceplen] as float32 and nframe as int32: the state the
 *   utterance leaves.  stdout: "DIMS <width> <raw> <window> <streams> <ceplen> <has_cmn>".
 *   feat_update_stats is NOT called between utterances: nothing in the library calls it, and
 *   the update at an utterance's end is feat_cmn's own (endutt).
 * Exits 0, or 1 saying what failed (also when feat_init refuses the configuration). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <soundswallower/ckd_alloc.h>
#include <soundswallower/cmn.h>
#include <soundswallower/configuration.h>
#include <soundswallower/feat.h>

static void
die(const char *what)
{
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
}

static feat_t *
make_feat(config_t *c)
{
    feat_t *f = feat_init(c);
    if (f == NULL)
        die("feat_init");
    return f;
}

int
main(int argc, char *argv[])
{
    config_t *c = config_init(NULL);
    feat_t *fcb = NULL;
    FILE *in, *out;
    int a, chain, first = 1;

    if (argc < 5)
        die("usage");
    chain = strcmp(argv[1], "chain") == 0;
    if (!chain && strcmp(argv[1], "fresh") != 0)
        die("MODE is fresh or chain");
    config_set_str(c, "loglevel", "ERROR");
    for (a = 4; a < argc && strcmp(argv[a], "--") != 0; ++a) {
        char *eq = strchr(argv[a], '=');
        if (eq == NULL)
            die("KEY=VALUE expected");
        *eq = '\0';
        if (config_set_str(c, argv[a], eq + 1) == NULL)
            die("config_set_str");
    }
    if (a >= argc)
        die("-- and the utterances' lengths expected");
    if ((in = fopen(argv[2], "rb")) == NULL || (out = fopen(argv[3], "wb")) == NULL)
        die("cannot open CEPIN or OUT");
    for (++a; a < argc; ++a) {
        const int n = atoi(argv[a]);
        int32 ncep = n, ceplen, raw = 0, width, i;
        mfcc_t **cep, ***feat;
        if (n < 0 || (n == 0 && !chain))
            die("bad LEN");
        if (fcb == NULL || !chain) {
            feat_free(fcb);
            fcb = make_feat(c);
        }
        ceplen = feat_cepsize(fcb);
        for (i = 0; i < fcb->n_stream; ++i)
            raw += fcb->stream_len[i];
        width = fcb->subvecs ? fcb->sv_dim : (int32)feat_dimension(fcb);
        if (first) {
            printf("DIMS %d %d %d %d %d %d\n", width, raw, feat_window_size(fcb), fcb->n_stream, ceplen,
                   fcb->cmn_struct != NULL);
            first = 0;
        }
        cep = (mfcc_t **)ckd_calloc_2d(n ? n : 1, ceplen, sizeof(mfcc_t));
        feat = feat_array_alloc(fcb, n ? n : 1);
        if (n && fread(cep[0], sizeof(mfcc_t) * (size_t)ceplen, (size_t)n, in) != (size_t)n)
            die("CEPIN is too short");
        if (feat_s2mfc2feat_live(fcb, cep, &ncep, 1, 1, feat) != n)
            die("feat_s2mfc2feat_live did not return every frame");
        for (i = 0; i < n; ++i)
            if (fwrite(feat[i][0], sizeof(mfcc_t), (size_t)width, out) != (size_t)width)
                die("write");
        if (fcb->cmn_struct != NULL) {
            const cmn_t *s = fcb->cmn_struct;
            int32 nframe = s->nframe;
            if (fwrite(s->cmn_mean, sizeof(mfcc_t), (size_t)ceplen, out) != (size_t)ceplen
                || fwrite(s->sum, sizeof(mfcc_t), (size_t)ceplen, out) != (size_t)ceplen
                || fwrite(&nframe, sizeof(nframe), 1, out) != 1)
                die("write");
        }
        ckd_free_2d(cep);
        feat_array_free(feat);
    }
    feat_free(fcb);
    config_free(c);
    fclose(in);
    if (fclose(out) != 0)
        die("write");
    return 0;
}
