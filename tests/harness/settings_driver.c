/* settings_driver.c -- the reference library scoring, aligning and recognising under a
 * non-default logbase, varfloor, mixwfloor or tmatfloor, for tests/golden/make_settings.py.
 * The decoder's public API, its acmod, and the scorer's tables through the library's own headers.
 * Every mode makes a fresh decoder on HMM with compallsen = yes and the four settings as given:
 *
 *   settings_driver score HMM LOGBASE VARFLOOR MIXWFLOOR TMATFLOOR PCM FEATOUT
 *       the whole of PCM (int16) through acmod_process_raw as one utterance, every frame through
 *       acmod_score.  The feature rows acmod scored are written to FEATOUT as float32.  Prints
 *         SCORER <name>                 the vtable's name
 *         TABLE det <crc32> var <crc32> CRC-32 of det[m][f][k] and of the scaled variances
 *                                       var[m][f][k][j], m, f, k, j ascending, as float32
 *         ROW <frame> <crc32>           CRC-32 of the frame's n_sen int16 scores
 *         FULL <frame> <n_sen values>   frames 0, 1, 2 and the last
 *       The log level is INFO in this mode: the loader's "<n> variance values floored" is on
 *       stderr with the rest of the log.
 *   settings_driver rec HMM LOGBASE VARFLOOR MIXWFLOOR TMATFLOOR FSG PCM
 *       HYP / SEG / JSON as fsg_driver prints them
 *   settings_driver align HMM LOGBASE VARFLOOR MIXWFLOOR TMATFLOOR PCM
 *       decoder_result_json at align_level 1 of the text "go forward ten meters"
 * What the library reports through its error log goes to stderr.  Exits 0, or 1 saying what
 * failed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <soundswallower/acmod.h>
#include <soundswallower/configuration.h>
#include <soundswallower/decoder.h>
#include <soundswallower/fsg_model.h>
#include <soundswallower/ms_mgau.h>
#include <soundswallower/ptm_mgau.h>

static void
die(const char *what)
{
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
}

static void *
read_file(const char *path, size_t *n)
{
    FILE *f = fopen(path, "rb");
    long len;
    void *p;
    if (f == NULL || fseek(f, 0, SEEK_END) != 0 || (len = ftell(f)) < 0 || fseek(f, 0, SEEK_SET) != 0)
        die("cannot read an input file");
    *n = (size_t)len;
    p = malloc(*n + 2);
    if (p == NULL || fread(p, 1, *n, f) != *n)
        die("cannot read an input file");
    fclose(f);
    return p;
}

static unsigned
crc32_of(unsigned crc, const void *data, size_t n)
{
    const unsigned char *p = (const unsigned char *)data;
    size_t i;
    int k;
    crc = ~crc;
    for (i = 0; i < n; ++i) {
        crc ^= p[i];
        for (k = 0; k < 8; ++k)
            crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

/* argv[2..6]: HMM LOGBASE VARFLOOR MIXWFLOOR TMATFLOOR */
static decoder_t *
make_decoder(char **argv, const char *loglevel)
{
    config_t *c = config_init(NULL);
    decoder_t *d;
    config_set_str(c, "hmm", argv[2]);
    config_set_str(c, "compallsen", "yes");
    config_set_float(c, "logbase", atof(argv[3]));
    config_set_float(c, "varfloor", atof(argv[4]));
    config_set_float(c, "mixwfloor", atof(argv[5]));
    config_set_float(c, "tmatfloor", atof(argv[6]));
    config_set_str(c, "loglevel", loglevel);
    if ((d = decoder_init(c)) == NULL)
        die("decoder_init");
    return d;
}

static void
print_tables(acmod_t *a)
{
    const char *name = a->mgau->vt->name;
    gauden_t *g = NULL;
    printf("SCORER %s\n", name);
    if (strcmp(name, "ms") == 0)
        g = ((ms_mgau_model_t *)a->mgau)->g;
    else if (strcmp(name, "ptm") == 0)
        g = ((ptm_mgau_t *)a->mgau)->g;
    if (g != NULL) {
        unsigned cd = 0, cv = 0;
        int m, f, k;
        for (m = 0; m < g->n_mgau; ++m)
            for (f = 0; f < g->n_feat; ++f)
                for (k = 0; k < g->n_density; ++k) {
                    cd = crc32_of(cd, &g->det[m][f][k], sizeof(mfcc_t));
                    cv = crc32_of(cv, g->var[m][f][k], sizeof(mfcc_t) * (size_t)g->featlen[f]);
                }
        printf("TABLE det %u var %u\n", cd, cv);
    }
}

static void
score_all(acmod_t *a)
{
    const int n_sen = bin_mdef_n_sen(a->mdef), total = a->n_feat_frame;
    while (a->n_feat_frame > 0) {
        int fi = -1, i;
        const int16 *s = acmod_score(a, &fi);
        if (s == NULL)
            die("acmod_score");
        printf("ROW %d %u\n", fi, crc32_of(0, s, sizeof(int16) * (size_t)n_sen));
        if (fi < 3 || fi == total - 1) {
            printf("FULL %d", fi);
            for (i = 0; i < n_sen; ++i)
                printf(" %d", s[i]);
            printf("\n");
        }
        acmod_advance(a);
    }
}

int
main(int argc, char **argv)
{
    if (argc == 9 && !strcmp(argv[1], "score")) {
        size_t n;
        int16 *pcm = (int16 *)read_file(argv[7], &n), *p = pcm;
        decoder_t *d = make_decoder(argv, "INFO");
        acmod_t *a = d->acmod;
        FILE *out;
        int f, i, dim = 0;
        n /= sizeof(int16);
        print_tables(a);
        acmod_set_grow(a, TRUE);
        acmod_start_utt(a);
        if (acmod_process_raw(a, &p, &n, TRUE) < 0)
            die("acmod_process_raw");
        acmod_end_utt(a);
        for (i = 0; i < feat_dimension1(a->fcb); ++i)
            dim += (int)feat_dimension2(a->fcb, i);
        if ((out = fopen(argv[8], "wb")) == NULL)
            die("cannot write the feature rows");
        for (f = 0; f < a->n_feat_frame; ++f) {
            int fi = f;
            mfcc_t **row = acmod_get_frame(a, &fi);
            if (row == NULL || fwrite(row[0], sizeof(mfcc_t), (size_t)dim, out) != (size_t)dim)
                die("cannot write the feature rows");
        }
        fclose(out);
        score_all(a);
        decoder_free(d);
        free(pcm);
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "rec")) {
        size_t n;
        int16 *pcm = (int16 *)read_file(argv[8], &n);
        decoder_t *d = make_decoder(argv, "ERROR");
        fsg_model_t *fsg = fsg_model_readfile(argv[7], decoder_logmath(d),
                                              (float32)config_float(decoder_config(d), "lw"));
        const char *hyp, *js;
        seg_iter_t *it;
        int32 score;
        n /= sizeof(int16);
        printf("SCORER %s\n", d->acmod->mgau->vt->name);
        if (fsg == NULL || decoder_set_fsg(d, fsg) < 0)
            die("decoder_set_fsg");
        if (decoder_start_utt(d) < 0 || decoder_process_int16(d, pcm, n, FALSE, TRUE) < 0
            || decoder_end_utt(d) < 0)
            die("recognition");
        printf("FRAMES %d\n", decoder_n_frames(d));
        hyp = decoder_hyp(d, &score);
        if (hyp == NULL)
            printf("NOHYP\n");
        else
            printf("HYP %d %s\n", score, hyp);
        for (it = decoder_seg_iter(d); it; it = seg_iter_next(it)) {
            int sf, ef;
            int32 ascr, lscr, prob;
            seg_iter_frames(it, &sf, &ef);
            prob = seg_iter_prob(it, &ascr, &lscr);
            printf("SEG %d %d %d %d %d %s\n", sf, ef, ascr, lscr, prob, seg_iter_word(it));
        }
        if ((js = decoder_result_json(d, 0.0, 0)) == NULL)
            die("decoder_result_json");
        printf("JSON %s", js); /* (the line ends in its own newline) */
        decoder_free(d);
        free(pcm);
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "align")) {
        size_t n;
        int16 *pcm = (int16 *)read_file(argv[7], &n);
        decoder_t *d = make_decoder(argv, "ERROR");
        const char *js;
        n /= sizeof(int16);
        printf("SCORER %s\n", d->acmod->mgau->vt->name);
        if (decoder_set_align_text(d, "go forward ten meters") < 0 || decoder_start_utt(d) < 0
            || decoder_process_int16(d, pcm, n, FALSE, TRUE) < 0 || decoder_end_utt(d) < 0)
            die("alignment");
        if ((js = decoder_result_json(d, 0.0, 1)) == NULL)
            die("decoder_result_json");
        printf("JSON %s", js);
        decoder_free(d);
        free(pcm);
        return 0;
    }
    fprintf(stderr, "usage: settings_driver score HMM LOGBASE VARFLOOR MIXWFLOOR TMATFLOOR PCM FEATOUT"
                    " | rec HMM LOGBASE VARFLOOR MIXWFLOOR TMATFLOOR FSG PCM"
                    " | align HMM LOGBASE VARFLOOR MIXWFLOOR TMATFLOOR PCM\n");
    return 1;
}
