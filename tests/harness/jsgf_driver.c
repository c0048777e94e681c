/* jsgf_driver.c -- the reference library parsing a JSGF grammar, building the FSG of one rule and
 * recognising against it, for tests/golden/make_jsgf.py.  Only the public config_* / jsgf_* /
 * fsg_model_* / decoder_* API; the steps are those of decoder_set_jsgf_file, taken one by one so
 * that the grammar can be written out between them.
 *
 *   jsgf_driver HMM GRAM PCM NSAMP COMPALLSEN TOPRULE
 *       decoder_init on HMM with loglevel=ERROR and, when COMPALLSEN is "yes", compallsen=yes;
 *       jsgf_parse_file of GRAM; the rule TOPRULE ("grammar.rule", through jsgf_get_rule) or,
 *       when TOPRULE is "-", jsgf_get_public_rule; jsgf_build_fsg with the decoder's log base and
 *       lw; decoder_set_fsg; the first NSAMP samples of PCM (int16; 0: all of it) as one full
 *       utterance.  Prints, one item per line:
 *         GRAMMAR <name>                       jsgf_grammar_name
 *         RULE <0|1> <name>                    jsgf_rule_iter order: public flag, jsgf_rule_name
 *         CHOSEN <name>                        the rule built
 *         REFUSED <what>                       the step that failed; nothing follows
 *         FSG <line>                           fsg_model_write after jsgf_build_fsg
 *         FSG2 <line>                          the same of a second jsgf_build_fsg of the same rule
 *                                              from the same parsed grammar
 *         FSGX <line>                          fsg_model_write of the first after decoder_set_fsg
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
#include <soundswallower/jsgf.h>

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
    jsgf_t *jsgf;
    jsgf_rule_t *rule;
    jsgf_rule_iter_t *it_r;
    fsg_model_t *fsg, *fsg2;
    const char *hyp, *js;
    seg_iter_t *it;
    int32 score;
    float32 lw;

    if (argc != 7) {
        fprintf(stderr, "usage: jsgf_driver HMM GRAM PCM NSAMP COMPALLSEN TOPRULE\n");
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
    if (strcmp(argv[5], "yes") == 0)
        config_set_str(c, "compallsen", "yes");
    config_set_str(c, "loglevel", "ERROR");
    if ((d = decoder_init(c)) == NULL)
        die("decoder_init");
    if ((jsgf = jsgf_parse_file(argv[2], NULL)) == NULL) {
        printf("REFUSED jsgf_parse_file\n");
        return 0;
    }
    printf("GRAMMAR %s\n", jsgf_grammar_name(jsgf));
    for (it_r = jsgf_rule_iter(jsgf); it_r; it_r = jsgf_rule_iter_next(it_r))
        printf("RULE %d %s\n", jsgf_rule_public(jsgf_rule_iter_rule(it_r)) ? 1 : 0,
               jsgf_rule_name(jsgf_rule_iter_rule(it_r)));
    if (strcmp(argv[6], "-") != 0) {
        if ((rule = jsgf_get_rule(jsgf, argv[6])) == NULL) {
            printf("REFUSED Start rule %s not found\n", argv[6]); /* src/decoder.c:627 */
            return 0;
        }
    } else if ((rule = jsgf_get_public_rule(jsgf)) == NULL) {
        printf("REFUSED No public rules found in %s\n", argv[2]);
        return 0;
    }
    printf("CHOSEN %s\n", jsgf_rule_name(rule));
    lw = (float32)config_float(decoder_config(d), "lw");
    if ((fsg = jsgf_build_fsg(jsgf, rule, decoder_logmath(d), lw)) == NULL)
        die("jsgf_build_fsg");
    print_fsg("FSG", fsg);
    if ((fsg2 = jsgf_build_fsg(jsgf, rule, decoder_logmath(d), lw)) == NULL)
        die("jsgf_build_fsg, second time");
    print_fsg("FSG2", fsg2);
    fsg_model_free(fsg2);
    if (decoder_set_fsg(d, fsg) < 0) { /* (the search owns the grammar from here and changes it) */
        printf("REFUSED decoder_set_fsg\n");
        return 0;
    }
    jsgf_grammar_free(jsgf);
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
