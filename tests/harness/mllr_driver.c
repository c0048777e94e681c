/* mllr_driver.c -- the reference library scoring, recognising and aligning with an MLLR-adapted
 * acoustic model, for tests/golden/make_mllr.py.  The decoder's public API, its acmod, and the
 * scorers' Gaussians through the library's own headers.
 *
 * Every mode takes HOW and MLLR, the two ways the reference reaches gauden_mllr_transform:
 *     config   mllr = MLLR in the configuration decoder_init gets (src/acmod.c:122-127)
 *     apply    a decoder without it, then mllr_read(MLLR) + decoder_apply_mllr (src/decoder.c:590)
 *     none     no transform (MLLR is ignored)
 *
 *   mllr_driver score HMM HOW MLLR MIXW DS PCM FEATOUT
 *       compallsen = yes, ds = DS; MIXW other than "-": mixw = MIXW and senmgau = .semi., which
 *       makes the ms scorer of a model acmod would give to ptm.  The whole of PCM (int16) through
 *       acmod_process_raw as one utterance, every frame through acmod_score.  The feature rows
 *       acmod scored go to FEATOUT as float32.  Prints
 *         SCORER <name>                 the vtable's name
 *         TABLE det <crc32> var <crc32> CRC-32 of det[m][f][k] and of the scaled variances
 *                                       var[m][f][k][j], m, f, k, j ascending, as float32
 *         ROW <frame> <crc32>           CRC-32 of the frame's n_sen int16 scores
 *         FULL <frame> <n_sen values>   frames 0, 1, 2 and the last
 *   mllr_driver rec HMM HOW MLLR COMPALLSEN FSG PCM
 *       COMPALLSEN yes | default (the key left unset); HYP / SEG / JSON as fsg_driver prints them
 *   mllr_driver align HMM HOW MLLR COMPALLSEN PCM
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
#include <soundswallower/mllr.h>
#include <soundswallower/ms_mgau.h>
#include <soundswallower/ptm_mgau.h>
#include <soundswallower/s2_semi_mgau.h>

static void
die(const char *what)
{
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
}

static int16 *
read_pcm(const char *path, size_t *n)
{
    FILE *f = fopen(path, "rb");
    long len;
    int16 *p;
    if (f == NULL || fseek(f, 0, SEEK_END) != 0 || (len = ftell(f)) < 0 || fseek(f, 0, SEEK_SET) != 0)
        die("cannot read the PCM file");
    *n = (size_t)len / sizeof(int16);
    p = (int16 *)malloc(*n * sizeof(int16) + 2);
    if (p == NULL || fread(p, sizeof(int16), *n, f) != *n)
        die("cannot read the PCM file");
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

static decoder_t *
make_decoder(const char *hmm, const char *how, const char *mllr, const char *compallsen,
             const char *mixw, const char *ds)
{
    config_t *c = config_init(NULL);
    decoder_t *d;
    config_set_str(c, "hmm", hmm);
    if (!strcmp(compallsen, "yes"))
        config_set_str(c, "compallsen", "yes");
    else if (strcmp(compallsen, "default"))
        die("COMPALLSEN is yes or default");
    if (mixw != NULL && strcmp(mixw, "-")) {
        config_set_str(c, "mixw", mixw);
        config_set_str(c, "senmgau", ".semi.");
    }
    if (ds != NULL)
        config_set_int(c, "ds", atol(ds));
    if (!strcmp(how, "config"))
        config_set_str(c, "mllr", mllr);
    config_set_str(c, "loglevel", "ERROR");
    if ((d = decoder_init(c)) == NULL)
        die("decoder_init");
    if (!strcmp(how, "apply")) {
        mllr_t *t = mllr_read(mllr);
        if (t == NULL)
            die("mllr_read");
        if (decoder_apply_mllr(d, t) == NULL)
            die("decoder_apply_mllr");
        mllr_free(t); /* (acmod holds its own reference) */
    } else if (strcmp(how, "config") && strcmp(how, "none"))
        die("HOW is config, apply or none");
    return d;
}

static void
print_tables(acmod_t *a)
{
    const char *name = a->mgau->vt->name;
    gauden_t *g = NULL;
    unsigned cd = 0, cv = 0;
    int m, f, k;
    printf("SCORER %s\n", name);
    if (strcmp(name, "ms") == 0)
        g = ((ms_mgau_model_t *)a->mgau)->g;
    else if (strcmp(name, "ptm") == 0)
        g = ((ptm_mgau_t *)a->mgau)->g;
    else if (strcmp(name, "s2_semi") == 0)
        g = ((s2_semi_mgau_t *)a->mgau)->g;
    else
        die("unknown scorer");
    for (m = 0; m < g->n_mgau; ++m)
        for (f = 0; f < g->n_feat; ++f)
            for (k = 0; k < g->n_density; ++k) {
                cd = crc32_of(cd, &g->det[m][f][k], sizeof(mfcc_t));
                cv = crc32_of(cv, g->var[m][f][k], sizeof(mfcc_t) * (size_t)g->featlen[f]);
            }
    printf("TABLE det %u var %u\n", cd, cv);
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
        int16 *pcm = read_pcm(argv[7], &n), *p = pcm;
        decoder_t *d = make_decoder(argv[2], argv[3], argv[4], "yes", argv[5], argv[6]);
        acmod_t *a = d->acmod;
        FILE *out;
        int f, i, dim = 0;
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
    if (argc == 8 && !strcmp(argv[1], "rec")) {
        size_t n;
        int16 *pcm = read_pcm(argv[7], &n);
        decoder_t *d = make_decoder(argv[2], argv[3], argv[4], argv[5], NULL, NULL);
        fsg_model_t *fsg = fsg_model_readfile(argv[6], decoder_logmath(d),
                                              (float32)config_float(decoder_config(d), "lw"));
        const char *hyp, *js;
        seg_iter_t *it;
        int32 score;
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
    if (argc == 7 && !strcmp(argv[1], "align")) {
        size_t n;
        int16 *pcm = read_pcm(argv[6], &n);
        decoder_t *d = make_decoder(argv[2], argv[3], argv[4], argv[5], NULL, NULL);
        const char *js;
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
    fprintf(stderr, "usage: mllr_driver score HMM HOW MLLR MIXW DS PCM FEATOUT | rec HMM HOW MLLR "
                    "COMPALLSEN FSG PCM | align HMM HOW MLLR COMPALLSEN PCM\n");
    return 1;
}
