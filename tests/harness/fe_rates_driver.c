/* fe_rates_driver.c -- the reference library's front end and decoder at any sample rate, for
 * tests/golden/make_mfcc_rates.py.  Only the public fe_* / config_* / decoder_* API.
 *
 *   fe_rates_driver fe JSON PCM OUT     fe_init with the settings in JSON (config_parse_json over
 *                                       the defaults), fe_start + fe_process_int16 over all of
 *                                       PCM (int16) + fe_end; the cepstra to OUT as float32
 *                                       [frames][ncep]; prints the frame count
 *   fe_rates_driver count JSON PCM NMAX frames of PCM[0 .. n) for n = 1 .. NMAX, one per line
 *   fe_rates_driver align HMM RATE COMPALLSEN PCM
 *                                       decoder_init on HMM, samprate RATE as decode_file sets it
 *                                       (py/_soundswallower.pyx:757-762: config, then
 *                                       reinit_feat), "go forward ten meters" aligned to PCM;
 *                                       prints decoder_result_json at align_level 1
 * Exits 0, or 1 saying what failed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <soundswallower/configuration.h>
#include <soundswallower/decoder.h>
#include <soundswallower/fe.h>

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

static fe_t *
make_fe(const char *json)
{
    config_t *c = config_init(NULL);
    fe_t *fe;
    config_set_str(c, "loglevel", "ERROR");
    if (c == NULL || config_parse_json(c, json) == NULL)
        die("config_parse_json");
    fe = fe_init(c);
    if (fe == NULL)
        die("fe_init refused the settings");
    config_free(c);
    return fe;
}

/* the frames of pcm[0 .. n) into rows (NULL: count only) */
static int
run_fe(fe_t *fe, const int16 *pcm, size_t n, mfcc_t **rows, int max_rows)
{
    int16 *p = (int16 *)pcm;
    size_t left = n;
    int nfr = 0, k;
    if (fe_start(fe) < 0)
        die("fe_start");
    while (left > 0) {
        k = fe_process_int16(fe, &p, &left, rows ? rows + nfr : NULL, max_rows - nfr);
        if (k < 0)
            die("fe_process_int16");
        nfr += k;
        if (k == 0 && left > 0)
            die("fe_process_int16 made no progress");
    }
    k = fe_end(fe, rows ? rows + nfr : NULL, max_rows - nfr);
    if (k < 0)
        die("fe_end");
    return nfr + k;
}

static mfcc_t **
alloc_rows(int n, int ncep)
{
    mfcc_t **rows = (mfcc_t **)malloc(sizeof(*rows) * (size_t)(n > 0 ? n : 1));
    mfcc_t *buf = (mfcc_t *)calloc((size_t)(n > 0 ? n : 1) * (size_t)ncep, sizeof(mfcc_t));
    int i;
    if (rows == NULL || buf == NULL)
        die("out of memory");
    for (i = 0; i < n; ++i)
        rows[i] = buf + (size_t)i * ncep;
    return rows;
}

int
main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "fe")) {
        size_t n;
        int16 *pcm = read_pcm(argv[3], &n);
        fe_t *fe = make_fe(argv[2]);
        int ncep = fe_get_output_size(fe);
        int cap = (int)(n / 2 + 16); /* frame shift > 1 */
        mfcc_t **rows = alloc_rows(cap, ncep);
        int nfr = run_fe(fe, pcm, n, rows, cap);
        FILE *out = fopen(argv[4], "wb");
        if (out == NULL || (nfr > 0 && fwrite(rows[0], sizeof(mfcc_t) * (size_t)ncep, (size_t)nfr, out) != (size_t)nfr))
            die("cannot write the cepstra");
        fclose(out);
        printf("%d\n", nfr);
        fe_free(fe);
        free(rows[0]);
        free(rows);
        free(pcm);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "count")) {
        size_t n, k, nmax = (size_t)atol(argv[4]);
        int16 *pcm = read_pcm(argv[3], &n);
        fe_t *fe = make_fe(argv[2]);
        int cap = (int)(nmax / 2 + 16);
        mfcc_t **rows = alloc_rows(cap, fe_get_output_size(fe));
        if (nmax > n)
            die("NMAX is longer than the PCM");
        for (k = 1; k <= nmax; ++k)
            printf("%d\n", run_fe(fe, pcm, k, rows, cap));
        fe_free(fe);
        free(rows[0]);
        free(rows);
        free(pcm);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "align")) {
        size_t n;
        int16 *pcm = read_pcm(argv[5], &n);
        config_t *c = config_init(NULL);
        decoder_t *d;
        const char *js;
        config_set_str(c, "hmm", argv[2]);
        config_set_str(c, "compallsen", argv[4]);
        config_set_str(c, "loglevel", "ERROR");
        if ((d = decoder_init(c)) == NULL)
            die("decoder_init");
        config_set_int(decoder_config(d), "samprate", atol(argv[3]));
        if (decoder_reinit_feat(d, NULL) < 0)
            die("decoder_reinit_feat");
        if (decoder_set_align_text(d, "go forward ten meters") < 0 || decoder_start_utt(d) < 0
            || decoder_process_int16(d, pcm, n, FALSE, TRUE) < 0 || decoder_end_utt(d) < 0)
            die("alignment");
        if ((js = decoder_result_json(d, 0.0, 1)) == NULL)
            die("decoder_result_json");
        fputs(js, stdout); /* (the line ends in its own newline) */
        decoder_free(d);
        free(pcm);
        return 0;
    }
    fprintf(stderr, "usage: fe_rates_driver fe JSON PCM OUT | count JSON PCM NMAX | "
                    "align HMM RATE COMPALLSEN PCM\n");
    return 1;
}
