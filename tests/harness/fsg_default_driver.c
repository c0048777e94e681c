/* fsg_default_driver.c -- the reference library recognising against a word FSG in its DEFAULT
 * configuration, for tests/golden/make_fsg_default.py.  Only the public config_* / fsg_model_* /
 * decoder_* API.  fsg_driver.c with neither compallsen nor bestpath set: acmod scores the senones
 * of the HMMs the search holds active, and the scorer normalises over those.
 *
 *   fsg_default_driver HMM FSG PCM NSAMP
 *       decoder_init on HMM with loglevel=ERROR and nothing else, fsg_model_readfile of FSG
 *       with the decoder's log base and lw, the first NSAMP samples of PCM (int16; 0: all of it)
 *       as one full utterance.  Prints, one item per line:
 *         FSG <line>                           fsg_model_write of the grammar as read (null
 *                                              closure done, no silences or alternates yet)
 *         FSGX <line>                          the same after decoder_set_fsg: with the silences
 *                                              and alternates fsg_search_init added
 *         FRAMES <n>                           decoder_n_frames
 *         HYP <score> <text> | NOHYP           decoder_hyp
 *         SEG <sf> <ef> <ascr> <lscr> <prob> <word>   decoder_seg_iter + seg_iter_prob
 *         JSON <line>                          decoder_result_json(d, 0, 0)
 *       What the library reports through its error log goes to stderr as it comes.
 * Exits 0, or 1 saying what failed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
print_fsg(const char *tag, fsg_model_t *fsg)
{
    char *dump = NULL, *line, *save;
    size_t dump_len = 0;
    FILE *mem = open_memstream(&dump, &dump_len);
    if (mem == NULL)
        die("open_memstream");
    fsg_model_write(fsg, mem);
    fclose(mem);
    for (line = strtok_r(dump, "\n", &save); line; line = strtok_r(NULL, "\n", &save))
        printf("%s %s\n", tag, line);
    free(dump);
}

int
main(int argc, char **argv)
{
    size_t n, want;
    int16 *pcm;
    config_t *c;
    decoder_t *d;
    fsg_model_t *fsg;
    const char *hyp, *js;
    seg_iter_t *it;
    int32 score;

    if (argc != 5) {
        fprintf(stderr, "usage: fsg_default_driver HMM FSG PCM NSAMP\n");
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
    if ((d = decoder_init(c)) == NULL)
        die("decoder_init");
    fsg = fsg_model_readfile(argv[2], decoder_logmath(d),
                             (float32)config_float(decoder_config(d), "lw"));
    if (fsg == NULL)
        die("fsg_model_readfile");
    print_fsg("FSG", fsg);
    if (decoder_set_fsg(d, fsg) < 0) /* (the search owns the grammar from here and changes it) */
        die("decoder_set_fsg");
    print_fsg("FSGX", fsg);
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
