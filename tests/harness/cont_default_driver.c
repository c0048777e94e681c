/* cont_default_driver.c -- the reference library aligning a text in its DEFAULT configuration
 * (compallsen = no), for tests/golden/make_cont_default.py.  Only the public config_* / decoder_*
 * API, in the manner of fsg_default_driver.c.
 *
 *   cont_default_driver align HMM PCM TEXT
 *       decoder_init on HMM with loglevel=ERROR and nothing else, decoder_set_align_text(TEXT),
 *       the whole of PCM (int16) as one full utterance.  Prints, one item per line:
 *         FRAMES <n>                           decoder_n_frames
 *         JSON0 <line>                         decoder_result_json(d, 0, 0)
 *         JSON1 <line> | JSON1 NOALIGN         decoder_result_json(d, 0, 1), NOALIGN for NULL
 *         JSON2 <line> | JSON2 NOALIGN         decoder_result_json(d, 0, 2)
 *       What the library reports through its error log goes to stderr as it comes.
 * Exits 0, or 1 saying what failed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <soundswallower/configuration.h>
#include <soundswallower/decoder.h>

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

int
main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "align")) {
        size_t n;
        int16 *pcm = read_pcm(argv[3], &n);
        config_t *c = config_init(NULL);
        decoder_t *d;
        int level;
        config_set_str(c, "hmm", argv[2]);
        config_set_str(c, "loglevel", "ERROR");
        if ((d = decoder_init(c)) == NULL)
            die("decoder_init");
        if (decoder_set_align_text(d, argv[4]) < 0 || decoder_start_utt(d) < 0
            || decoder_process_int16(d, pcm, n, FALSE, TRUE) < 0 || decoder_end_utt(d) < 0)
            die("alignment");
        printf("FRAMES %d\n", decoder_n_frames(d));
        for (level = 0; level <= 2; ++level) {
            const char *js = decoder_result_json(d, 0.0, level);
            if (js == NULL)
                printf("JSON%d NOALIGN\n", level);
            else
                printf("JSON%d %s", level, js); /* (the line ends in its own newline) */
        }
        decoder_free(d);
        free(pcm);
        return 0;
    }
    fprintf(stderr, "usage: cont_default_driver align HMM PCM TEXT\n");
    return 1;
}
