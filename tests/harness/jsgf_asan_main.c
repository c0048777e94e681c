/* Stand-alone sanitizer program for the JSGF front door (csrc/ssw_jsgf.c): built by
 * tests/test_jsgf_sanitizers.py with -fsanitize=address,undefined from csrc/ssw_model.c +
 * ssw_lexicon.c + ssw_fsg.c + ssw_jsgf.c and this file, which supplies the one thing the HIP
 * translation unit normally provides to them (the model handle).
 *
 *   usage: jsgf_asan_main <model dir> grammar.gram ...
 *       every grammar: parsed from the file and from its text; every rule of it expanded twice,
 *       without a dictionary and with the model's, and written out as read and as searched; the
 *       one-call entry points.  Then a fixed list of malformed and outsized inputs, each of which
 *       has to be refused (or accepted) without a fault.  Prints "ok ..." and exits 0; exits 1
 *       where an input that must parse does not, or one that must not does. */
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

static long n_built, n_refused, n_bytes;

static void
write_out(const ssw_fsg_t *f, const ssw_dict_t *d, int searched)
{
    int32_t need = ssw_fsg_write(f, d, NULL, searched, NULL, 0);
    char *buf;
    if (need < 0)
        return;
    buf = (char *)malloc((size_t)need + 1);
    if (buf != NULL && ssw_fsg_write(f, d, NULL, searched, buf, need + 1) == need)
        n_bytes += (long)strlen(buf);
    free(buf);
}

/* the first `limit` rules and the public one, twice each (the second build starts from the weights
 * the first left) */
static void
expand_all(const ssw_model_t *m, const ssw_dict_t *d, ssw_jsgf_t *j, int limit, int write_states)
{
    const int pub = ssw_jsgf_public_rule(j);
    int i, k;
    for (i = 0; i < ssw_jsgf_n_rules(j); ++i)
        for (k = 0; k < 2 && (i < limit || i == pub); ++k) {
            const ssw_dict_t *dk = k ? d : NULL;
            ssw_fsg_t *f = ssw_jsgf_build_fsg(m, dk, j, i);
            if (f == NULL) {
                ++n_refused;
                continue;
            }
            ++n_built;
            if (ssw_fsg_n_states(f) <= write_states) { /* (the null closure of a deep nest is slow) */
                write_out(f, dk, 0);
                if (dk != NULL)
                    write_out(f, dk, 1);
            }
            ssw_fsg_free(f);
        }
}

/* 1 parsed, 0 refused */
static int
try_text(const ssw_model_t *m, const ssw_dict_t *d, const char *text)
{
    ssw_jsgf_t *j = ssw_jsgf_parse_string(text);
    ssw_fsg_t *f;
    int has_a = 0;
    if (j != NULL) {
        (void)ssw_jsgf_name(j);
        (void)ssw_jsgf_public_rule(j);
        has_a = ssw_jsgf_find_rule(j, "t.a") >= 0;
        (void)ssw_jsgf_rule_name(j, -1);
        (void)ssw_jsgf_rule_public(j, ssw_jsgf_n_rules(j));
        expand_all(m, d, j, 2, 150);
        ssw_jsgf_free(j);
    } else
        ++n_refused;
    if ((f = ssw_fsg_from_jsgf_string(m, d, text, has_a ? NULL : "t.a")) != NULL)
        ssw_fsg_free(f);
    return j != NULL;
}

static char *
read_all(const char *path)
{
    FILE *fp = fopen(path, "rb");
    long size;
    char *buf;
    if (fp == NULL || fseek(fp, 0, SEEK_END) != 0 || (size = ftell(fp)) < 0
        || fseek(fp, 0, SEEK_SET) != 0 || (buf = (char *)malloc((size_t)size + 1)) == NULL)
        return NULL;
    if (fread(buf, 1, (size_t)size, fp) != (size_t)size) {
        free(buf);
        buf = NULL;
    } else
        buf[size] = '\0';
    fclose(fp);
    return buf;
}

#define HEAD "#JSGF V1.0;\ngrammar t;\n"

/* HEAD public <a> = open x depth  go  close x depth ; */
static char *
nested(int depth, const char *open, const char *close)
{
    const size_t lo = strlen(open), lc = strlen(close);
    char *s = (char *)malloc(strlen(HEAD) + 64 + (lo + lc) * (size_t)depth), *p = s;
    int i;
    if (s == NULL)
        return NULL;
    p += sprintf(p, "%spublic <a> = ", HEAD);
    for (i = 0; i < depth; ++i, p += lo)
        memcpy(p, open, lo);
    p += sprintf(p, " go ");
    for (i = 0; i < depth; ++i, p += lc)
        memcpy(p, close, lc);
    sprintf(p, ";\n");
    return s;
}

int
main(int argc, char **argv)
{
    /* (text, 1 when it has to parse) */
    static const struct { const char *text; int parses; } fixed[] = {
        { "", 0 },
        { "#JSGF", 0 },
        { HEAD, 1 },
        { HEAD "public <a> = go {never closed ;\n", 0 },              /* unterminated tag */
        { HEAD "public <a> = go {closed \\} twice} \\} ;\n", 0 },
        { HEAD "public <a> = \"go ten;\n", 1 },                       /* unterminated quote: a token */
        { HEAD "public <a> = \"go \\\" ten;\n", 1 },
        { HEAD "public <a> = go /* never closed ;\n", 0 },            /* unterminated comment */
        { HEAD "public <a> = go; /* never closed", 1 },
        { HEAD "public <a> = go /0.5 ten;\n", 0 },                    /* unterminated weight */
        { HEAD "public <a> = go /", 0 },
        { HEAD "public <a> = go //", 0 },
        { HEAD "public <a> = // go;", 1 },                            /* no line end: a weight of 0 */
        { HEAD "public <a> = ;\n", 0 },                               /* an empty rule */
        { HEAD "public <a> = go | ;\n", 0 },
        { HEAD "public <a> = go );\n", 0 },                           /* a stray ) */
        { HEAD "public <a> = ( go ];\n", 0 },
        { HEAD "public <a> = <>;\n", 0 },
        { HEAD "public <a> = <", 0 },
        { HEAD "public <a", 0 },
        { HEAD "public", 0 },
        { HEAD "import <x.y>;\npublic <a> = go;\n", 0 },
        { HEAD "public <a> = go <a>;\n", 1 },                         /* recursion with no way out */
        { HEAD "public <a> = <a>;\n", 1 },
        { HEAD "public <a> = <a> go;\n", 1 },                         /* left recursion: refused */
        { HEAD "public <a> = <b>; <b> = <c> x; <c> = <a>;\n", 1 },
        { HEAD "public <a> = <nowhere>;\n", 1 },
        { HEAD "public <a> = <VOID>;\n", 1 },
        { HEAD "public <a> = <NULL>;\n", 1 },
        { HEAD "public <a> = <NULL>*;\n", 1 },
        { HEAD "public <a> = /0/ go | /0/ ten;\n", 1 },
        { HEAD "public <a> = /1e-99/ go | ten /99999999999999999999999999999999999999999/ x;\n", 1 },
        { HEAD "public <a> = go; <a> = (ten)*; public <a> = [stop]+;\n", 1 },
        { HEAD "public <.> = go; public <a.> = <.> <.a>;\n", 1 },
        { "\xEF\xBB\xBF#JSGF a b c;grammar \xC3\xA9;public <\xC3\xA9> = \xC3\xA9 \x80\xFF;", 1 },
    };
    char p[6][600];
    struct ssw_model_s m;
    ssw_dict_t *d;
    size_t i;
    int a, n_files = 0;
    char *s, *q;

    if (argc < 2)
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
    snprintf(p[0], sizeof p[0], "%s/dict.txt", argv[1]);
    snprintf(p[1], sizeof p[1], "%s/noisedict.txt", argv[1]);
    if ((d = ssw_dict_load(&m, p[0], p[1])) == NULL) {
        fprintf(stderr, "dict: %s\n", ssw_last_error());
        return 1;
    }
    /* the committed grammars */
    for (a = 2; a < argc; ++a, ++n_files) {
        ssw_jsgf_t *j = ssw_jsgf_parse_file(argv[a]);
        ssw_fsg_t *f;
        if (j == NULL) {
            fprintf(stderr, "%s: %s\n", argv[a], ssw_last_error());
            return 1;
        }
        expand_all(&m, d, j, 1 << 20, 2000);
        ssw_jsgf_free(j);
        if ((f = ssw_fsg_from_jsgf_file(&m, d, argv[a], NULL)) != NULL)
            ssw_fsg_free(f);
        if ((s = read_all(argv[a])) == NULL || !try_text(&m, d, s)) {
            fprintf(stderr, "%s: its text does not parse: %s\n", argv[a], ssw_last_error());
            return 1;
        }
        /* and every prefix of it that ends at a line end: cut grammars (the small ones) */
        for (q = s + strlen(s); q > s && strlen(s) < 2000; --q)
            if (q[-1] == '\n' && *q != '\0') {
                *q = '\0';
                (void)try_text(&m, d, s);
            }
        free(s);
    }
    if (ssw_jsgf_parse_file("/nonexistent/nowhere.gram") != NULL)
        return 1;
    /* the fixed list */
    for (i = 0; i < sizeof(fixed) / sizeof(fixed[0]); ++i)
        if (try_text(&m, d, fixed[i].text) != fixed[i].parses) {
            fprintf(stderr, "input %d %s: %s\n", (int)i,
                    fixed[i].parses ? "does not parse" : "parses", ssw_last_error());
            return 1;
        }
    /* nesting 200 deep, of every kind, parses and expands; 5000 deep is refused, not a fault.
     * (x)+ names x twice, so nesting it doubles the grammar with every level: 12 deep */
    {
        static const char *const kind[][2] = { { "(", ")" }, { "[", "]" }, { "(", ")*" },
                                               { "[(", ")+]" } };
        for (i = 0; i < 4; ++i) {
            if ((s = nested(i == 3 ? 12 : 200, kind[i][0], kind[i][1])) == NULL
                || !try_text(&m, d, s)) {
                fprintf(stderr, "nesting 200 deep (%s): %s\n", kind[i][0], ssw_last_error());
                return 1;
            }
            free(s);
            if ((s = nested(5000, kind[i][0], kind[i][1])) == NULL || try_text(&m, d, s)) {
                fprintf(stderr, "nesting 5000 deep (%s) was not refused\n", kind[i][0]);
                return 1;
            }
            free(s);
        }
    }
    /* a chain of 5000 rules, each naming the next: refused when expanded */
    {
        size_t cap = 64 * 5000 + 256, len;
        if ((s = (char *)malloc(cap)) == NULL)
            return 1;
        len = (size_t)sprintf(s, "%spublic <a> = <r0>;\n", HEAD);
        for (a = 0; a < 5000; ++a)
            len += (size_t)sprintf(s + len, "<r%d> = go <r%d>;\n", a, a + 1);
        sprintf(s + len, "<r5000> = stop;\n");
        if (!try_text(&m, d, s))
            return 1;
        free(s);
    }
    /* a rule referenced twice is expanded twice: 2^24 copies are refused */
    {
        size_t len;
        if ((s = (char *)malloc(4096)) == NULL)
            return 1;
        len = (size_t)sprintf(s, "%spublic <a> = <r0>;\n", HEAD);
        for (a = 0; a < 24; ++a)
            len += (size_t)sprintf(s + len, "<r%d> = <r%d> <r%d>;\n", a, a + 1, a + 1);
        sprintf(s + len, "<r24> = go;\n");
        if (!try_text(&m, d, s))
            return 1;
        free(s);
    }
    /* a 1 MB token, tag, rule name and quoted string */
    {
        static const char *const form[] = { "%spublic <a> = go %s ten;\n", "%spublic <a> = go {%s} ten;\n",
                                            "%spublic <a> = go <%s>;\n", "%spublic <a> = go \"%s\" ten;\n",
                                            "%spublic <%s> = go;\n", "%spublic <a> = go /%s/ ten;\n" };
        const size_t big = 1u << 20;
        char *tok = (char *)malloc(big + 1);
        if (tok == NULL || (s = (char *)malloc(big + 256)) == NULL)
            return 1;
        for (i = 0; i < sizeof(form) / sizeof(form[0]); ++i) {
            memset(tok, i == 5 ? '7' : 'x', big);
            tok[big] = '\0';
            sprintf(s, form[i], HEAD, tok);
            if (!try_text(&m, d, s)) {
                fprintf(stderr, "1 MB input %d: %s\n", (int)i, ssw_last_error());
                return 1;
            }
        }
        free(tok);
        free(s);
    }
    printf("ok %d grammars, %ld built, %ld refused, %ld bytes written\n", n_files, n_built,
           n_refused, n_bytes);
    ssw_dict_free(d);
    ssw_host_model_free(m.h);
    return 0;
}
