/* inputs_driver.c -- the reference library fed float32 audio, and words added to its loaded
 * dictionary, for tests/golden/make_inputs.py.  Only the public fe_* / config_* / fsg_model_* /
 * decoder_* API, in the manner of fe_rates_driver.c and fsg_driver.c.
 *
 *   inputs_driver fe32 JSON F32FILE OUT
 *       fe_init with the settings in JSON (config_parse_json over the defaults), fe_start +
 *       fe_process_float32 over all of F32FILE (float32, 1.0 = 32768) + fe_end; the cepstra to
 *       OUT as float32 [frames][ncep]; prints the frame count
 *   inputs_driver align32 HMM RATE COMPALLSEN F32FILE TEXT
 *       decoder_init on HMM, samprate RATE (config, then decoder_reinit_feat), TEXT aligned to
 *       F32FILE through decoder_process_float32 as one full utterance; prints
 *       decoder_result_json at align_level 1
 *   inputs_driver words HMM ADDS COMPALLSEN PCM TEXT|FSG
 *       decoder_init on HMM; every line "word<TAB>phones" of ADDS through decoder_add_word, then
 *       decoder_lookup_word of each; an argument ending in ".fsg" is read with fsg_model_readfile
 *       and set with decoder_set_fsg, anything else is a text for decoder_set_align_text; PCM
 *       (int16) as one full utterance.  Prints, one item per line:
 *         ADD <return value> <word>
 *         LOOKUP <word><TAB><phones> | LOOKUP <word><TAB>(NULL)
 *         FSGX <line>            fsg_model_write of the searched grammar, after decoder_set_fsg.
 *                                For a text the grammar is built here as decoder_set_align_text
 *                                builds it (src/decoder.c:708-729: fsg_model_init named by the
 *                                text, one fsg_model_word_add and fsg_model_trans_add per word)
 *                                and set on the decoder for the dump; decoder_set_align_text
 *                                then replaces it for the search
 *         FRAMES <n>             decoder_n_frames
 *         HYP <score> <text> | NOHYP
 *         SEG <sf> <ef> <ascr> <lscr> <prob> <word>
 *         JSON1 <line> | JSON1 NOALIGN      decoder_result_json(d, 0, 1)
 * What the library reports through its error log goes to stderr as it comes.
 * Exits 0, or 1 saying what failed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <soundswallower/configuration.h>
#include <soundswallower/decoder.h>
#include <soundswallower/fe.h>
#include <soundswallower/fsg_model.h>

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
        die("cannot read the input file");
    *n = (size_t)len / item;
    p = malloc(*n * item + item);
    if (p == NULL || fread(p, item, *n, f) != *n)
        die("cannot read the input file");
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

static int
ends_with(const char *s, const char *tail)
{
    size_t n = strlen(s), k = strlen(tail);
    return n >= k && strcmp(s + n - k, tail) == 0;
}

static int
mode_fe32(char **argv)
{
    size_t n, left;
    float32 *pcm = (float32 *)read_file(argv[3], sizeof(float32), &n), *p = pcm;
    config_t *c = config_init(NULL);
    fe_t *fe;
    mfcc_t **rows, *buf;
    int ncep, cap, nfr = 0, k, i;
    FILE *out;
    config_set_str(c, "loglevel", "ERROR");
    if (config_parse_json(c, argv[2]) == NULL)
        die("config_parse_json");
    if ((fe = fe_init(c)) == NULL)
        die("fe_init refused the settings");
    config_free(c);
    ncep = fe_get_output_size(fe);
    cap = (int)(n / 2 + 16); /* frame shift > 1 */
    rows = (mfcc_t **)malloc(sizeof(*rows) * (size_t)cap);
    buf = (mfcc_t *)calloc((size_t)cap * (size_t)ncep, sizeof(mfcc_t));
    if (rows == NULL || buf == NULL)
        die("out of memory");
    for (i = 0; i < cap; ++i)
        rows[i] = buf + (size_t)i * ncep;
    if (fe_start(fe) < 0)
        die("fe_start");
    for (left = n; left > 0; nfr += k) {
        k = fe_process_float32(fe, &p, &left, rows + nfr, cap - nfr);
        if (k < 0)
            die("fe_process_float32");
        if (k == 0 && left > 0)
            die("fe_process_float32 made no progress");
    }
    if ((k = fe_end(fe, rows + nfr, cap - nfr)) < 0)
        die("fe_end");
    nfr += k;
    out = fopen(argv[4], "wb");
    if (out == NULL || (nfr > 0 && fwrite(buf, sizeof(mfcc_t) * (size_t)ncep, (size_t)nfr, out) != (size_t)nfr))
        die("cannot write the cepstra");
    fclose(out);
    printf("%d\n", nfr);
    fe_free(fe);
    free(buf);
    free(rows);
    free(pcm);
    return 0;
}

static decoder_t *
make_decoder(const char *hmm, const char *compallsen)
{
    config_t *c = config_init(NULL);
    decoder_t *d;
    config_set_str(c, "hmm", hmm);
    config_set_str(c, "compallsen", compallsen);
    config_set_str(c, "loglevel", "ERROR");
    if ((d = decoder_init(c)) == NULL)
        die("decoder_init");
    return d;
}

static int
mode_align32(char **argv)
{
    size_t n;
    float32 *pcm = (float32 *)read_file(argv[5], sizeof(float32), &n);
    decoder_t *d = make_decoder(argv[2], argv[4]);
    const char *js;
    config_set_int(decoder_config(d), "samprate", atol(argv[3]));
    if (decoder_reinit_feat(d, NULL) < 0)
        die("decoder_reinit_feat");
    if (decoder_set_align_text(d, argv[6]) < 0 || decoder_start_utt(d) < 0
        || decoder_process_float32(d, pcm, n, FALSE, TRUE) < 0 || decoder_end_utt(d) < 0)
        die("alignment");
    if ((js = decoder_result_json(d, 0.0, 1)) == NULL)
        die("decoder_result_json");
    fputs(js, stdout); /* (the line ends in its own newline) */
    decoder_free(d);
    free(pcm);
    return 0;
}

/* the grammar decoder_set_align_text makes of a text (src/decoder.c:708-729) */
static fsg_model_t *
text_fsg(decoder_t *d, const char *text)
{
    char *buf = strdup(text), *save, *w;
    int n = 0;
    fsg_model_t *fsg;
    for (w = strtok_r(buf, " \t\n\r", &save); w; w = strtok_r(NULL, " \t\n\r", &save))
        ++n;
    free(buf);
    fsg = fsg_model_init(text, decoder_logmath(d),
                         (float32)config_float(decoder_config(d), "lw"), n + 1);
    buf = strdup(text);
    n = 0;
    for (w = strtok_r(buf, " \t\n\r", &save); w; w = strtok_r(NULL, " \t\n\r", &save), ++n)
        fsg_model_trans_add(fsg, n, n + 1, 0, fsg_model_word_add(fsg, w));
    free(buf);
    fsg->start_state = 0;
    fsg->final_state = n;
    return fsg;
}

static int
mode_words(char **argv)
{
    size_t n;
    int16 *pcm = (int16 *)read_file(argv[5], sizeof(int16), &n);
    decoder_t *d = make_decoder(argv[2], argv[4]);
    FILE *adds = fopen(argv[3], "r");
    char line[4096], *words[64];
    int n_adds = 0, i;
    fsg_model_t *fsg;
    const char *hyp, *js;
    seg_iter_t *it;
    int32 score;

    if (adds == NULL)
        die("cannot read ADDS");
    while (fgets(line, sizeof(line), adds)) {
        char *tab = strchr(line, '\t');
        if (tab == NULL || n_adds == 64)
            die("ADDS: word<TAB>phones, 64 lines at most");
        *tab = '\0';
        tab[1 + strcspn(tab + 1, "\r\n")] = '\0';
        words[n_adds++] = strdup(line);
        printf("ADD %d %s\n", decoder_add_word(d, line, tab + 1, TRUE), line);
    }
    fclose(adds);
    for (i = 0; i < n_adds; ++i) {
        char *ph = decoder_lookup_word(d, words[i]);
        printf("LOOKUP %s\t%s\n", words[i], ph ? ph : "(NULL)");
        free(ph);
        free(words[i]);
    }
    if (ends_with(argv[6], ".fsg")) {
        fsg = fsg_model_readfile(argv[6], decoder_logmath(d),
                                 (float32)config_float(decoder_config(d), "lw"));
        if (fsg == NULL)
            die("fsg_model_readfile");
        if (decoder_set_fsg(d, fsg) < 0) /* (the search owns the grammar from here and changes it) */
            die("decoder_set_fsg");
        print_fsg("FSGX", fsg);
    } else {
        fsg = text_fsg(d, argv[6]);
        if (decoder_set_fsg(d, fsg) < 0)
            die("decoder_set_fsg of the text's grammar");
        print_fsg("FSGX", fsg);
        if (decoder_set_align_text(d, argv[6]) < 0) /* (frees the search above and its grammar) */
            die("decoder_set_align_text");
    }
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
    js = hyp ? decoder_result_json(d, 0.0, 1) : NULL;
    if (js == NULL)
        printf("JSON1 NOALIGN\n");
    else
        printf("JSON1 %s", js); /* (the line ends in its own newline) */
    decoder_free(d);
    free(pcm);
    return 0;
}

int
main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "fe32"))
        return mode_fe32(argv);
    if (argc == 7 && !strcmp(argv[1], "align32"))
        return mode_align32(argv);
    if (argc == 7 && !strcmp(argv[1], "words"))
        return mode_words(argv);
    fprintf(stderr, "usage: inputs_driver fe32 JSON F32FILE OUT | align32 HMM RATE COMPALLSEN "
                    "F32FILE TEXT | words HMM ADDS COMPALLSEN PCM TEXT|FSG\n");
    return 1;
}
