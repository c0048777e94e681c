/* fe_any_driver.c -- the reference library's front end under any settings fe_init accepts, and
 * its aligner on a model directory with such settings, for tests/golden/make_fe_any.py.  Only the
 * public fe_* / config_* / decoder_* API.  One process per fixture: the reference keeps warp
 * parameters in process-wide statics.
 *
 *   fe_any_driver fe JSON KIND PCM OUT   fe_init with the settings in JSON (config_parse_json over
 *                                        the defaults), fe_start + fe_process_int16 (KIND i16, PCM
 *                                        int16) or fe_process_float32 (KIND f32, PCM float32) over
 *                                        all samples + fe_end; the rows to OUT as float32
 *                                        [frames][fe_get_output_size]; prints "frames width"
 *   fe_any_driver align HMM COMPALLSEN PCM
 *                                        decoder_init on the model directory HMM, "go forward ten
 *                                        meters" aligned to PCM (int16, 16 kHz); prints
 *                                        decoder_result_json at align_level 1
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

static void *
read_file(const char *path, size_t item, size_t *n)
{
    FILE *f = fopen(path, "rb");
    long len;
    void *p;
    if (f == NULL || fseek(f, 0, SEEK_END) != 0 || (len = ftell(f)) < 0 || fseek(f, 0, SEEK_SET) != 0)
        die("cannot read the PCM file");
    *n = (size_t)len / item;
    p = malloc(*n * item + item);
    if (p == NULL || fread(p, item, *n, f) != *n)
        die("cannot read the PCM file");
    fclose(f);
    return p;
}

int
main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "fe")) {
        const int f32 = !strcmp(argv[3], "f32");
        size_t n, left;
        void *pcm = read_file(argv[4], f32 ? sizeof(float32) : sizeof(int16), &n);
        config_t *c = config_init(NULL);
        fe_t *fe;
        mfcc_t **rows, *buf;
        int width, cap, nfr = 0, k, i;
        FILE *out;
        if (c == NULL)
            die("config_init");
        config_set_str(c, "loglevel", "ERROR");
        if (config_parse_json(c, argv[2]) == NULL)
            die("config_parse_json");
        if ((fe = fe_init(c)) == NULL)
            die("fe_init refused the settings");
        config_free(c);
        width = fe_get_output_size(fe);
        cap = (int)(n / 2 + 16); /* frame shift > 1 */
        rows = (mfcc_t **)malloc(sizeof(*rows) * (size_t)cap);
        buf = (mfcc_t *)calloc((size_t)cap * (size_t)width, sizeof(mfcc_t));
        if (rows == NULL || buf == NULL)
            die("out of memory");
        for (i = 0; i < cap; ++i)
            rows[i] = buf + (size_t)i * width;
        if (fe_start(fe) < 0)
            die("fe_start");
        left = n;
        if (f32) {
            float32 *p = (float32 *)pcm;
            while (left > 0) {
                if ((k = fe_process_float32(fe, &p, &left, rows + nfr, cap - nfr)) < 0)
                    die("fe_process_float32");
                nfr += k;
                if (k == 0 && left > 0)
                    die("fe_process_float32 made no progress");
            }
        } else {
            int16 *p = (int16 *)pcm;
            while (left > 0) {
                if ((k = fe_process_int16(fe, &p, &left, rows + nfr, cap - nfr)) < 0)
                    die("fe_process_int16");
                nfr += k;
                if (k == 0 && left > 0)
                    die("fe_process_int16 made no progress");
            }
        }
        if ((k = fe_end(fe, rows + nfr, cap - nfr)) < 0)
            die("fe_end");
        nfr += k;
        out = fopen(argv[5], "wb");
        if (out == NULL
            || (nfr > 0 && fwrite(buf, sizeof(mfcc_t) * (size_t)width, (size_t)nfr, out) != (size_t)nfr))
            die("cannot write the rows");
        fclose(out);
        printf("%d %d\n", nfr, width);
        fe_free(fe);
        free(buf);
        free(rows);
        free(pcm);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "align")) {
        size_t n;
        int16 *pcm = (int16 *)read_file(argv[4], sizeof(int16), &n);
        config_t *c = config_init(NULL);
        decoder_t *d;
        const char *js;
        if (c == NULL)
            die("config_init");
        config_set_str(c, "hmm", argv[2]);
        config_set_str(c, "compallsen", argv[3]);
        config_set_str(c, "loglevel", "ERROR");
        if ((d = decoder_init(c)) == NULL)
            die("decoder_init");
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
    fprintf(stderr, "usage: fe_any_driver fe JSON KIND PCM OUT | align HMM COMPALLSEN PCM\n");
    return 1;
}
