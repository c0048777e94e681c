/* Stand-alone sanitizer program for words added to a loaded dictionary (csrc/ssw_lexicon.c:
 * ssw_dict_add_word, ssw_dict_lookup_word): built by tests/test_dict_add_sanitizers.py with
 * -fsanitize=address,undefined from csrc/ssw_model.c + ssw_lexicon.c + ssw_fsg.c + ssw_jsgf.c and
 * this file, which supplies the one thing the HIP translation unit normally provides to them (the
 * model handle).
 *
 *   usage: dict_add_host <model dir> <small dictionary>
 *       the model's own dictionary: adds (alternates among them), every refusal, lookups into
 *       buffers of every length, the searched grammar written before and after.  Then the small
 *       dictionary, which starts at the first capacity: adds past the doubling and its rehash,
 *       alternates of words from before and after it, every word found again, the pointers
 *       ssw_dict_word handed out before the growth compared and read.  Prints "ok ..." and exits
 *       0; exits 1 where an add that must succeed does not, or one that must not does. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssw_internal.h"

struct ssw_model_s {
    ssw_host_model_t *h;
};

const ssw_host_model_t *
ssw_model_host(const ssw_model_t *m)
{
    return m->h;
}

static int n_added, n_refused;

static void
fail(const char *what, const char *word)
{
    fprintf(stderr, "FAILED: %s: %s (%s)\n", what, word, ssw_last_error());
    exit(1);
}

static int32_t
must_add(ssw_dict_t *d, const ssw_model_t *m, const char *word, const char *phones)
{
    const int32_t n = ssw_dict_size(d), w = ssw_dict_add_word(d, m, word, phones);
    if (w != n || ssw_dict_size(d) != n + 1 || ssw_dict_word_id(d, word) != w
        || strcmp(ssw_dict_word(d, w), word) != 0 || ssw_dict_is_filler(d, w))
        fail("add", word);
    ++n_added;
    return w;
}

static void
must_refuse(ssw_dict_t *d, const ssw_model_t *m, const char *word, const char *phones)
{
    const int32_t n = ssw_dict_size(d);
    if (ssw_dict_add_word(d, m, word, phones) != -1 || ssw_dict_size(d) != n)
        fail("refusal", word ? word : "(null)");
    ++n_refused;
}

/* the lookup into buffers of 0 .. need + 2 bytes, each allocated to its size */
static void
lookups(const ssw_dict_t *d, const ssw_model_t *m, const char *word, const char *want)
{
    const int32_t need = ssw_dict_lookup_word(d, m, word, NULL, 0);
    int32_t k;
    if (need != (int32_t)strlen(want))
        fail("lookup length", word);
    for (k = 1; k <= need + 2; ++k) {
        char *buf = (char *)malloc((size_t)k);
        const size_t len = (size_t)(k - 1 < need ? k - 1 : need);
        if (buf == NULL || ssw_dict_lookup_word(d, m, word, buf, k) != need
            || strlen(buf) != len || strncmp(buf, want, len) != 0)
            fail("lookup", word);
        free(buf);
    }
}

static long
searched_len(const ssw_model_t *m, const ssw_dict_t *d, const char *w1, const char *w2)
{
    const int32_t from[2] = { 0, 1 }, to[2] = { 1, 2 };
    const float prob[2] = { 1.0f, 1.0f };
    const char *const words[2] = { w1, w2 };
    ssw_fsg_t *f = ssw_fsg_create(m, d, "chain", 3, 0, 2, 2, from, to, prob, words);
    int32_t need;
    char *buf;
    long len;
    if (f == NULL)
        fail("ssw_fsg_create", w1);
    need = ssw_fsg_write(f, d, NULL, 1, NULL, 0);
    buf = (char *)malloc((size_t)need + 1);
    if (need < 0 || buf == NULL || ssw_fsg_write(f, d, NULL, 1, buf, need + 1) != need)
        fail("ssw_fsg_write", w1);
    len = (long)strlen(buf);
    free(buf);
    ssw_fsg_free(f);
    return len;
}

int
main(int argc, char **argv)
{
    char p[5][1024], word[64], long_pron[4 * 257 + 1];
    struct ssw_model_s m;
    ssw_dict_t *d;
    const char *early[8];
    long before, after;
    int32_t n0, i, w;

    if (argc != 3)
        return 2;
    snprintf(p[0], sizeof p[0], "%s/mdef", argv[1]);
    snprintf(p[1], sizeof p[1], "%s/means", argv[1]);
    snprintf(p[2], sizeof p[2], "%s/variances", argv[1]);
    snprintf(p[3], sizeof p[3], "%s/sendump", argv[1]);
    snprintf(p[4], sizeof p[4], "%s/transition_matrices", argv[1]);
    m.h = ssw_host_model_load(p[0], p[1], p[2], p[3], NULL, p[4], NULL);
    if (m.h == NULL) {
        fprintf(stderr, "load: %s\n", ssw_last_error());
        return 1;
    }
    /* the model's own dictionary */
    snprintf(p[0], sizeof p[0], "%s/dict.txt", argv[1]);
    snprintf(p[1], sizeof p[1], "%s/noisedict.txt", argv[1]);
    if ((d = ssw_dict_load(&m, p[0], p[1])) == NULL) {
        fprintf(stderr, "dict: %s\n", ssw_last_error());
        return 1;
    }
    before = searched_len(&m, d, "go", "forward");
    must_add(d, &m, "fourward", "F AO R W ER D");
    must_add(d, &m, "forward(2)", "  F AO\tW ER D \n");
    must_add(d, &m, "forward(3)", "F AO R D");
    must_add(d, &m, "fourward(2)", "F AO R W ER D Z");
    must_add(d, &m, "geee", "G");
    lookups(d, &m, "forward(2)", "F AO W ER D");
    lookups(d, &m, "geee", "G");
    lookups(d, &m, "forward", "F AO R W ER D");
    after = searched_len(&m, d, "go", "forward");
    if (after <= before || searched_len(&m, d, "geee", "fourward") <= 0)
        fail("the searched grammar does not offer the new alternates", "forward");
    must_refuse(d, &m, "forward", "F AO R W ER D");
    must_refuse(d, &m, "fourward", "F");
    must_refuse(d, &m, "qqnophone", "F XX");
    must_refuse(d, &m, "qqnophone", "F AO_a_phone_name_longer_than_any_buffer_that_holds_one_"
                                    "AO_a_phone_name_longer_than_any_buffer_that_holds_one");
    must_refuse(d, &m, "qqnobase(2)", "T EH N");
    must_refuse(d, &m, "qqempty", "");
    must_refuse(d, &m, "qqempty", " \t\n");
    must_refuse(d, &m, "qq word", "T EH N");
    must_refuse(d, &m, "", "T EH N");
    must_refuse(d, &m, NULL, "T EH N");
    must_refuse(d, &m, "qqnull", NULL);
    long_pron[0] = '\0';
    for (i = 0; i < 257; ++i)
        strcat(long_pron, i ? " AH" : "AH");
    must_refuse(d, &m, "qqlong", long_pron);
    long_pron[strlen(long_pron) - 3] = '\0'; /* 256 phones: what a dictionary line holds */
    must_add(d, &m, "qqlong", long_pron);
    lookups(d, &m, "qqlong", long_pron);
    if (ssw_dict_lookup_word(d, &m, "nosuchword", word, sizeof word) != -1
        || ssw_dict_lookup_word(d, &m, NULL, word, sizeof word) != -1)
        fail("lookup of an unknown word", "nosuchword");
    ssw_dict_free(d);

    /* growth: the small dictionary starts at 4096 entries */
    if ((d = ssw_dict_load(&m, argv[2], p[1])) == NULL) {
        fprintf(stderr, "dict: %s\n", ssw_last_error());
        return 1;
    }
    n0 = ssw_dict_size(d);
    if (n0 < 8 || n0 >= 4096)
        fail("the small dictionary", argv[2]);
    for (i = 0; i < 8; ++i)
        early[i] = ssw_dict_word(d, i);
    for (i = 0; i < 9000; ++i) { /* past 4096 and past 8192 */
        snprintf(word, sizeof word, "w%d", (int)i);
        must_add(d, &m, word, i % 3 ? "G OW" : "T EH N  M IY T ER Z");
        if (i % 1000 == 999) { /* alternates of words from before and after the growth */
            snprintf(word, sizeof word, "w%d(2)", (int)i);
            must_add(d, &m, word, "F AO R");
            snprintf(word, sizeof word, "w%d(2)", (int)(i / 1000));
            must_add(d, &m, word, "F AO R");
            must_refuse(d, &m, word, "F AO");
        }
    }
    for (i = 0; i < 9000; ++i) {
        snprintf(word, sizeof word, "w%d", (int)i);
        if ((w = ssw_dict_word_id(d, word)) < n0 || strcmp(ssw_dict_word(d, w), word) != 0
            || ssw_dict_base_id(d, w) != w)
            fail("a word is lost after the growth", word);
    }
    lookups(d, &m, "w8999", "G OW");
    lookups(d, &m, "w8999(2)", "F AO R");
    lookups(d, &m, "w9", "T EH N M IY T ER Z");
    for (i = 0; i < 8; ++i)
        if (ssw_dict_word(d, i) != early[i] || ssw_dict_word_id(d, early[i]) != i)
            fail("a word pointer moved", early[i]);
    if (!ssw_dict_is_filler(d, ssw_dict_word_id(d, "<sil>"))
        || ssw_dict_is_filler(d, ssw_dict_size(d) - 1) || searched_len(&m, d, "w0", "w8999") <= 0)
        fail("fillers after the growth", "<sil>");
    printf("ok %d added, %d refused, %d words\n", n_added, n_refused, (int)ssw_dict_size(d));
    ssw_dict_free(d);
    ssw_host_model_free(m.h);
    return 0;
}
