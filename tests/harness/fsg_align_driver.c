/* fsg_align_driver.c -- the reference library recognising against a grammar and then aligning
 * what it recognised (decoder_result_json at align_level 1 and 2, decoder_alignment), for
 * tests/golden/make_fsg_align.py.  Only the public config_* / fsg_model_* / decoder_* /
 * alignment_* API, in the manner of fsg_default_driver.c.
 *
 *   fsg_align_driver HMM GRAMMAR PCM NSAMP COMPALLSEN
 *       decoder_init on HMM with loglevel=ERROR and compallsen=COMPALLSEN (yes | no; no is the
 *       library's default and is then not set at all).  GRAMMAR ending in ".fsg": fsg_model_readfile
 *       with the decoder's log base and lw, then decoder_set_fsg; anything else is a JSGF file for
 *       decoder_set_jsgf_file.  The first NSAMP samples of PCM (int16; 0: all of it) as one full
 *       utterance.  Prints, one item per line:
 *         FRAMES <n>                           decoder_n_frames
 *         HYP <score> <text> | NOHYP           decoder_hyp
 *         JSON0 <line>                         decoder_result_json(d, 0, 0)
 *         JSON1 <line> | JSON1 NOALIGN         decoder_result_json(d, 0, 1), NOALIGN for NULL
 *         JSON2 <line> | JSON2 NOALIGN         decoder_result_json(d, 0, 2)
 *         WORD | PHONE | STATE <start> <duration> <score> <name>
 *                                              every entry of decoder_alignment, through
 *                                              alignment_words / _phones / _states and the
 *                                              alignment_iter_* calls; or ALIGNMENT NONE
 *       What the library reports through its error log goes to stderr as it comes.
 * Exits 0, or 1 saying what failed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <soundswallower/alignment.h>
#include <soundswallower/configuration.h>
#include <soundswallower/decoder.h>
#include <soundswallower/fsg_model.h>

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

static void
print_level(const char *tag, alignment_iter_t *it)
{
    for (; it; it = alignment_iter_next(it)) {
        int start, duration;
        int score = alignment_iter_seg(it, &start, &duration);
        printf("%s %d %d %d %s\n", tag, start, duration, score, alignment_iter_name(it));
    }
}

static int
ends_with(const char *s, const char *tail)
{
    size_t n = strlen(s), k = strlen(tail);
    return n >= k && strcmp(s + n - k, tail) == 0;
}

int
main(int argc, char **argv)
{
    size_t n, want;
    int16 *pcm;
    config_t *c;
    decoder_t *d;
    const char *hyp, *js;
    alignment_t *al;
    int32 score;
    int level;

    if (argc != 6 || (strcmp(argv[5], "yes") != 0 && strcmp(argv[5], "no") != 0)) {
        fprintf(stderr, "usage: fsg_align_driver HMM GRAMMAR PCM NSAMP yes|no\n");
        return 1;
    }
    pcm = read_pcm(argv[3], &n);
    want = (size_t)atol(argv[4]);
    if (want > n)
        die("NSAMP is longer than the PCM");
    if (want > 0)
        n = want;
    c = config_init(NULL);
    config_set_str(c, "hmm", argv[1]);
    config_set_str(c, "loglevel", "ERROR");
    if (strcmp(argv[5], "yes") == 0)
        config_set_bool(c, "compallsen", TRUE);
    if ((d = decoder_init(c)) == NULL)
        die("decoder_init");
    if (ends_with(argv[2], ".fsg")) {
        fsg_model_t *fsg = fsg_model_readfile(argv[2], decoder_logmath(d),
                                              (float32)config_float(decoder_config(d), "lw"));
        if (fsg == NULL)
            die("fsg_model_readfile");
        if (decoder_set_fsg(d, fsg) < 0) /* (the search owns the grammar from here) */
            die("decoder_set_fsg");
    } else if (decoder_set_jsgf_file(d, argv[2]) < 0)
        die("decoder_set_jsgf_file");
    if (decoder_start_utt(d) < 0 || decoder_process_int16(d, pcm, n, FALSE, TRUE) < 0
        || decoder_end_utt(d) < 0)
        die("recognition");
    printf("FRAMES %d\n", decoder_n_frames(d));
    hyp = decoder_hyp(d, &score);
    if (hyp == NULL)
        printf("NOHYP\n");
    else
        printf("HYP %d %s\n", score, hyp);
    if ((js = decoder_result_json(d, 0.0, 0)) == NULL)
        die("decoder_result_json");
    printf("JSON0 %s", js); /* (the line ends in its own newline) */
    for (level = 1; level <= 2; ++level) {
        js = decoder_result_json(d, 0.0, level);
        if (js == NULL)
            printf("JSON%d NOALIGN\n", level);
        else
            printf("JSON%d %s", level, js);
    }
    al = decoder_alignment(d);
    if (al == NULL)
        printf("ALIGNMENT NONE\n");
    else {
        print_level("WORD", alignment_words(al));
        print_level("PHONE", alignment_phones(al));
        print_level("STATE", alignment_states(al));
    }
    decoder_free(d);
    free(pcm);
    return 0;
}
