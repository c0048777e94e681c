/*
 * ssw_jsgf.c -- host C: JSGF grammars, the front door of decoder_set_jsgf_string / _file
 * (src/decoder.c:609-683).  A hand-written scanner and recursive-descent parser for what
 * src/jsgf_scanner.l and src/jsgf_parser.y accept, the rule table of src/jsgf.c, and the expansion
 * of one rule into the transition list jsgf_build_fsg_internal hands to fsg_model_* (src/jsgf.c:
 * 298-421, 483-532).  The result is an ssw_fsg_t; the grammar search takes it from there.
 *
 * What decides the reference's state numbers, link order and probabilities, restated here:
 *   - the scanner's longest-match rules (src/jsgf_scanner.l:54-90): outside a declaration
 *     everything but the keywords, a rule name and comments is skipped; inside one a token is a
 *     run of bytes other than blanks and = ; | * + < > ( ) [ ] { } /, a quoted string keeps its
 *     quotes, "//" without a line end after it is a weight of 0, a tag ends at the LAST '}' that
 *     every earlier '}' before it is escaped for;
 *   - groups, optionals and closures define rules <grammar.gNNNNN>, NNNNN the number of rules
 *     in the table at that moment (jsgf_define_rule :611-642); [x] is (<NULL> | x) with <NULL>
 *     walked first, x* is <g> = <NULL> | x <g>, x+ is <g> = x | x <g> (:173-205);
 *   - alternatives hang off a rule last-to-first (src/jsgf_parser.y:117-121);
 *   - the rule table is hash_table_new(64, 0): 101 buckets, key2hash over the full name with
 *     its angle brackets (src/hash_table.c:171-206), a bucket's chain its first key, then the
 *     later ones newest first (:355-395); jsgf_rule_iter walks the buckets in order, and
 *     jsgf_get_public_rule takes the first public rule met (:444-469);
 *   - expand_rule allocates entry and exit per instance, divides the leading weight of every
 *     alternative by their float32 sum IN PLACE, each time it expands the rule (:379-421).
 *
 * Deliberately different from the reference: where expand_rhs fails (an undefined rule, recursion
 * that is not right-recursion, <VOID>; :327-352) the reference logs the error, ignores it and
 * searches the half-built grammar (jsgf_build_fsg_internal does not look at expand_rule's
 * result, :502).  Here the build is refused with the reference's error text.  import is refused
 * as unsupported.
 */
#include "ssw_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAX_NEST 2000     /* groups within groups; rules within rules while expanding */
#define MAX_LINKS (1 << 20)
#define N_BUCKETS 101u    /* prime_size(64 + 32), src/hash_table.c:139-159 */

typedef struct {
    char *name;   /* a token, or <rule> */
    float weight;
} atom_t;

typedef struct {
    atom_t *atoms;
    int n, cap;
} alt_t;

typedef struct {
    char *name;   /* <grammar.rule> */
    int is_public;
    alt_t *alts;  /* in the order expand_rule walks rule->rhs, rhs->alt, ... */
    int n_alts;
    int entry, exit, on_stack;
} rule_t;

struct ssw_jsgf_s {
    char *name;
    rule_t **all;  /* every rule made, also those whose name was taken: owned here */
    int n_all, cap_all;
    rule_t **tab;  /* the table in jsgf_rule_iter order */
    unsigned *hash;
    int n_tab, cap_tab;
};

/* ---- scanner ---------------------------------------------------------------------------- */
enum { T_EOF, T_HEADER, T_GRAMMAR, T_IMPORT, T_PUBLIC, T_TOKEN, T_RULENAME, T_TAG, T_WEIGHT, T_CHAR };

typedef struct {
    const char *p, *end;
    int decl;  /* inside a declaration (the scanner's DECL state) */
    int line;  /* yylineno */
    int tok;
    const char *ts; /* the token's text */
    size_t tlen;
    float weight;
    int depth;
    int oom;
    ssw_jsgf_t *j;
} lex_t;

static char *
dup_n(const char *s, size_t n)
{
    char *r = (char *)malloc(n + 1);
    if (r != NULL) {
        memcpy(r, s, n);
        r[n] = '\0';
    }
    return r;
}

static int
is_ws(int c)
{
    return c == ' ' || c == '\t' || c == '\r' || c == '\n';
}

static int
is_token_char(int c)
{
    return c != '\0' && !is_ws(c) && strchr("=;|*+<>()[]{}/", c) == NULL;
}

static void
eat(lex_t *x, size_t n)
{
    size_t i;
    for (i = 0; i < n; ++i)
        if (x->p[i] == '\n')
            ++x->line;
    x->p += n;
}

/* \<[^<>]+\> at p: its length, or 0 */
static size_t
match_rulename(const char *p, const char *end)
{
    const char *q = p + 1;
    while (q < end && *q != '<' && *q != '>')
        ++q;
    return (q < end && *q == '>' && q > p + 1) ? (size_t)(q + 1 - p) : 0;
}

/* open (\\.|[^close]+)* close, the longest match: a closing character that a backslash precedes
 * can always be taken into the body, one that none precedes cannot */
static size_t
match_delimited(const char *p, const char *end, char close)
{
    const char *q;
    size_t best = 0;
    for (q = p + 1; q < end; ++q)
        if (*q == close) {
            best = (size_t)(q + 1 - p);
            if (!(q > p + 1 && q[-1] == '\\'))
                break;
        }
    return best;
}

/* \/[0-9]*(\.[0-9]+)?(e-)?[0-9]*\/ */
static size_t
match_weight(const char *p, const char *end)
{
    const char *q = p + 1;
    while (q < end && *q >= '0' && *q <= '9')
        ++q;
    if (q + 1 < end && *q == '.' && q[1] >= '0' && q[1] <= '9') {
        ++q;
        while (q < end && *q >= '0' && *q <= '9')
            ++q;
    }
    if (q + 1 < end && *q == 'e' && q[1] == '-')
        q += 2;
    while (q < end && *q >= '0' && *q <= '9')
        ++q;
    return (q < end && *q == '/') ? (size_t)(q + 1 - p) : 0;
}

static int
starts(const lex_t *x, const char *kw)
{
    const size_t n = strlen(kw);
    return (size_t)(x->end - x->p) >= n && memcmp(x->p, kw, n) == 0;
}

static void
set_tok(lex_t *x, int tok, size_t len)
{
    x->tok = tok;
    x->ts = x->p;
    x->tlen = len;
    eat(x, len);
}

static void
next_token(lex_t *x)
{
    for (;;) {
        size_t n;
        int c;
        if (x->p >= x->end) {
            x->tok = T_EOF;
            x->ts = x->p;
            x->tlen = 0;
            return;
        }
        c = (unsigned char)*x->p;
        if (is_ws(c)) {
            eat(x, 1);
            continue;
        }
        if (c == '/' && x->p + 1 < x->end && x->p[1] == '/') {
            /* \/\/.*\n : a comment only when the line ends */
            const char *nl = (const char *)memchr(x->p, '\n', (size_t)(x->end - x->p));
            if (nl != NULL) {
                eat(x, (size_t)(nl + 1 - x->p));
                continue;
            }
            if (x->decl) { /* the weight's pattern matches "//": atof("/") */
                x->weight = 0.0f;
                set_tok(x, T_WEIGHT, 2);
                return;
            }
            eat(x, 1);
            continue;
        }
        if (c == '/' && x->p + 1 < x->end && x->p[1] == '*') {
            const char *q = x->p + 2;
            while (q + 1 < x->end && !(q[0] == '*' && q[1] == '/'))
                ++q;
            eat(x, q + 1 < x->end ? (size_t)(q + 2 - x->p) : (size_t)(x->end - x->p));
            continue;
        }
        if (!x->decl) {
            if (starts(x, "\xEF\xBB\xBF#JSGF")) {
                x->decl = 1;
                set_tok(x, T_HEADER, 8);
                return;
            }
            if (starts(x, "#JSGF")) {
                x->decl = 1;
                set_tok(x, T_HEADER, 5);
                return;
            }
            if (starts(x, "grammar")) {
                x->decl = 1;
                set_tok(x, T_GRAMMAR, 7);
                return;
            }
            if (starts(x, "import")) {
                x->decl = 1;
                set_tok(x, T_IMPORT, 6);
                return;
            }
            if (starts(x, "public")) {
                x->decl = 1;
                set_tok(x, T_PUBLIC, 6);
                return;
            }
            if (c == '<' && (n = match_rulename(x->p, x->end)) > 0) {
                x->decl = 1;
                set_tok(x, T_RULENAME, n);
                return;
            }
            eat(x, 1); /* .|\n : unmatched stuff */
            continue;
        }
        if (c == '<' && (n = match_rulename(x->p, x->end)) > 0) {
            set_tok(x, T_RULENAME, n);
            return;
        }
        if (c == '{' && (n = match_delimited(x->p, x->end, '}')) > 0) {
            set_tok(x, T_TAG, n);
            return;
        }
        if (c == '/' && (n = match_weight(x->p, x->end)) > 0) {
            char *num = dup_n(x->p + 1, n - 1); /* atof(yytext + 1): the closing slash ends it */
            if (num == NULL)
                x->oom = 1;
            x->weight = num ? (float)atof(num) : 0.0f;
            free(num);
            set_tok(x, T_WEIGHT, n);
            return;
        }
        if (is_token_char(c)) {
            const char *q = x->p;
            size_t q_len = (c == '"') ? match_delimited(x->p, x->end, '"') : 0;
            while (q < x->end && is_token_char((unsigned char)*q))
                ++q;
            n = (size_t)(q - x->p);
            set_tok(x, T_TOKEN, q_len > n ? q_len : n);
            return;
        }
        if (c == ';')
            x->decl = 0;
        set_tok(x, T_CHAR, 1);
        return;
    }
}

/* ---- rule table ------------------------------------------------------------------------- */
/* key2hash, case-sensitive: chars are signed where the reference is built */
static unsigned
name_hash(const char *key)
{
    uint32_t hash = 0;
    int s = 0;
    for (; *key; ++key) {
        hash += (uint32_t)(int32_t)(signed char)*key << s;
        s += 5;
        if (s >= 25)
            s -= 24;
    }
    return hash % N_BUCKETS;
}

static int
table_find(const ssw_jsgf_t *j, const char *name)
{
    const unsigned h = name_hash(name);
    int lo = 0, hi = j->n_tab, i;
    while (lo < hi) { /* the table is kept in bucket order: the first entry of bucket h */
        const int mid = lo + (hi - lo) / 2;
        if (j->hash[mid] < h)
            lo = mid + 1;
        else
            hi = mid;
    }
    for (i = lo; i < j->n_tab && j->hash[i] == h; ++i)
        if (!strcmp(j->tab[i]->name, name))
            return i;
    return -1;
}

static void
alt_clear(alt_t *a)
{
    int i;
    for (i = 0; i < a->n; ++i)
        free(a->atoms[i].name);
    free(a->atoms);
    memset(a, 0, sizeof(*a));
}

static void
alts_free(alt_t *alts, int n)
{
    int i;
    for (i = 0; i < n; ++i)
        alt_clear(&alts[i]);
    free(alts);
}

static int
alt_push(alt_t *a, char *name, float weight)
{
    if (name == NULL)
        return -1;
    if (a->n == a->cap) {
        const int nc = a->cap ? 2 * a->cap : 4;
        atom_t *q = (atom_t *)realloc(a->atoms, sizeof(atom_t) * (size_t)nc);
        if (q == NULL) {
            free(name);
            return -1;
        }
        a->atoms = q;
        a->cap = nc;
    }
    a->atoms[a->n].name = name;
    a->atoms[a->n].weight = weight;
    ++a->n;
    return 0;
}

/* jsgf_fullname / jsgf_fullname_from_rule: <name> -> <grammar.name> unless it has a dot */
static char *
full_name(const char *grammar, size_t glen, const char *name)
{
    char *r;
    if (strchr(name + 1, '.'))
        return dup_n(name, strlen(name));
    if ((r = (char *)malloc(glen + strlen(name) + 4)) != NULL)
        sprintf(r, "<%.*s.%s", (int)glen, grammar, name + 1);
    return r;
}

/* jsgf_define_rule: takes over alts (also on failure); name NULL: an internal rule.  A name
 * already in the table keeps its first definition ("Multiply defined symbol") */
static rule_t *
define_rule(ssw_jsgf_t *j, const char *name, alt_t *alts, int n_alts, int is_public)
{
    rule_t *r = (rule_t *)calloc(1, sizeof(*r));
    if (r != NULL) {
        if (name == NULL) {
            if ((r->name = (char *)malloc(strlen(j->name) + 32)) != NULL)
                sprintf(r->name, "<%s.g%05d>", j->name, j->n_tab);
        } else
            r->name = full_name(j->name, strlen(j->name), name);
    }
    if (r == NULL || r->name == NULL)
        goto oom;
    if (j->n_all == j->cap_all) {
        const int nc = j->cap_all ? 2 * j->cap_all : 16;
        rule_t **q = (rule_t **)realloc(j->all, sizeof(rule_t *) * (size_t)nc);
        if (q == NULL)
            goto oom;
        j->all = q;
        j->cap_all = nc;
    }
    r->alts = alts;
    r->n_alts = n_alts;
    r->is_public = is_public;
    j->all[j->n_all++] = r;
    if (table_find(j, r->name) < 0) {
        const unsigned h = name_hash(r->name);
        int a = 0, pos;
        if (j->n_tab == j->cap_tab) {
            const int nc = j->cap_tab ? 2 * j->cap_tab : 16;
            rule_t **q = (rule_t **)realloc(j->tab, sizeof(rule_t *) * (size_t)nc);
            unsigned *g = q ? (unsigned *)realloc(j->hash, sizeof(unsigned) * (size_t)nc) : NULL;
            if (q) j->tab = q;
            if (g) j->hash = g;
            if (!g)
                return NULL; /* (the rule is owned by j->all already) */
            j->cap_tab = nc;
        }
        while (a < j->n_tab && j->hash[a] < h)
            ++a;
        pos = (a < j->n_tab && j->hash[a] == h) ? a + 1 : a;
        memmove(&j->tab[pos + 1], &j->tab[pos], sizeof(rule_t *) * (size_t)(j->n_tab - pos));
        memmove(&j->hash[pos + 1], &j->hash[pos], sizeof(unsigned) * (size_t)(j->n_tab - pos));
        j->tab[pos] = r;
        j->hash[pos] = h;
        ++j->n_tab;
    }
    return r;
oom:
    if (r != NULL)
        free(r->name);
    free(r);
    alts_free(alts, n_alts);
    return NULL;
}

/* ---- parser ----------------------------------------------------------------------------- */
/* every parse_* returns 0, or -1 with the error set (x->oom: out of memory) */
static int
syntax_error(lex_t *x, const char *expected)
{
    if (x->tok == T_EOF)
        ssw_set_error("syntax error, unexpected end of input, expecting %s at line %d", expected,
                      x->line);
    else
        ssw_set_error("syntax error, expecting %s at line %d current token '%.*s'", expected,
                      x->line, (int)(x->tlen > 64 ? 64 : x->tlen), x->ts);
    return -1;
}

static int
is_char(const lex_t *x, int c)
{
    return x->tok == T_CHAR && *x->ts == c;
}

static int parse_alternatives(lex_t *x, alt_t **alts_out, int *n_out, int optional);

/* rule_atom: TOKEN | RULENAME | ( alternate_list ) | [ alternate_list ], then any * and + */
static int
parse_atom(lex_t *x, char **name_out)
{
    char *name = NULL;
    if (x->tok == T_TOKEN || x->tok == T_RULENAME) {
        if ((name = dup_n(x->ts, x->tlen)) == NULL)
            goto oom;
        next_token(x);
    } else if (is_char(x, '(') || is_char(x, '[')) {
        const int optional = is_char(x, '[');
        alt_t *alts;
        int n_alts;
        rule_t *r;
        if (++x->depth > MAX_NEST) {
            ssw_set_error("groups nested more than %d deep at line %d", MAX_NEST, x->line);
            return -1;
        }
        next_token(x);
        if (parse_alternatives(x, &alts, &n_alts, optional) < 0)
            return -1;
        --x->depth;
        if (!is_char(x, optional ? ']' : ')')) {
            alts_free(alts, n_alts);
            return syntax_error(x, optional ? "']'" : "')'");
        }
        if ((r = define_rule(x->j, NULL, alts, n_alts, 0)) == NULL
            || (name = dup_n(r->name, strlen(r->name))) == NULL)
            goto oom;
        next_token(x);
    } else
        return syntax_error(x, "a token, a rule name, '(' or '['");
    while (is_char(x, '*') || is_char(x, '+')) {
        /* jsgf_kleene_new: <g> = <NULL> | atom <g>, or atom | atom <g> */
        const int plus = is_char(x, '+');
        alt_t *alts = (alt_t *)calloc(2, sizeof(alt_t));
        rule_t *r;
        char *gname;
        if (alts == NULL
            || alt_push(&alts[0], plus ? dup_n(name, strlen(name)) : dup_n("<NULL>", 6), 1.0f) < 0) {
            alts_free(alts, alts ? 2 : 0);
            goto oom;
        }
        if (alt_push(&alts[1], name, 1.0f) < 0) {
            name = NULL;
            alts_free(alts, 2);
            goto oom;
        }
        name = NULL;
        /* (the rule takes its number before its second alternative names it) */
        if ((r = define_rule(x->j, NULL, alts, 2, 0)) == NULL)
            goto oom;
        if (alt_push(&r->alts[1], dup_n(r->name, strlen(r->name)), 1.0f) < 0
            || (gname = dup_n(r->name, strlen(r->name))) == NULL)
            goto oom;
        name = gname;
        next_token(x);
    }
    *name_out = name;
    return 0;
oom:
    free(name);
    x->oom = 1;
    ssw_set_error("out of memory parsing the JSGF grammar");
    return -1;
}

/* alternate_list: sequences of [/weight/] atom {tag}* separated by '|'.  On success *alts_out
 * holds them in the order expand_rule walks them: last to first, after <NULL> for an optional */
static int
parse_alternatives(lex_t *x, alt_t **alts_out, int *n_out, int optional)
{
    alt_t *alts = NULL;
    int n = 0, cap = 0, i, k;
    if (optional) { /* jsgf_optional_new */
        if ((alts = (alt_t *)calloc(4, sizeof(alt_t))) == NULL
            || alt_push(&alts[0], dup_n("<NULL>", 6), 1.0f) < 0)
            goto oom;
        n = 1;
        cap = 4;
    }
    for (;;) {
        alt_t *a;
        if (n == cap) {
            const int nc = cap ? 2 * cap : 4;
            alt_t *q = (alt_t *)realloc(alts, sizeof(alt_t) * (size_t)nc);
            if (q == NULL)
                goto oom;
            memset(q + cap, 0, sizeof(alt_t) * (size_t)(nc - cap));
            alts = q;
            cap = nc;
        }
        a = &alts[n++];
        memset(a, 0, sizeof(*a));
        do {
            float weight = 1.0f;
            int weighted = 0;
            char *name;
            if (x->tok == T_WEIGHT) {
                weight = x->weight;
                weighted = 1;
                next_token(x);
            }
            if (parse_atom(x, &name) < 0)
                goto bad;
            if (alt_push(a, name, weighted ? weight : 1.0f) < 0)
                goto oom;
            while (x->tok == T_TAG) /* kept by the reference's parser, dropped by its FSG builder */
                next_token(x);
        } while (x->tok == T_WEIGHT || x->tok == T_TOKEN || x->tok == T_RULENAME
                 || is_char(x, '(') || is_char(x, '['));
        if (!is_char(x, '|'))
            break;
        next_token(x);
    }
    if (x->oom)
        goto oom;
    /* the parser links each alternative in front of the ones before it */
    for (i = optional ? 1 : 0, k = n - 1; i < k; ++i, --k) {
        alt_t t = alts[i];
        alts[i] = alts[k];
        alts[k] = t;
    }
    *alts_out = alts;
    *n_out = n;
    return 0;
oom:
    x->oom = 1;
    ssw_set_error("out of memory parsing the JSGF grammar");
bad:
    alts_free(alts, n);
    return -1;
}

void
ssw_jsgf_free(ssw_jsgf_t *j)
{
    int i;
    if (j == NULL)
        return;
    for (i = 0; i < j->n_all; ++i) {
        alts_free(j->all[i]->alts, j->all[i]->n_alts);
        free(j->all[i]->name);
        free(j->all[i]);
    }
    free(j->all);
    free(j->tab);
    free(j->hash);
    free(j->name);
    free(j);
}

static ssw_jsgf_t *
parse(const char *text, size_t len)
{
    lex_t x;
    ssw_jsgf_t *j = (ssw_jsgf_t *)calloc(1, sizeof(*j));
    int n_hdr = 0;

    if (j == NULL) {
        ssw_set_error("out of memory parsing the JSGF grammar");
        return NULL;
    }
    memset(&x, 0, sizeof(x));
    x.p = text;
    x.end = text + len;
    x.line = 1;
    x.j = j;
    next_token(&x);
    /* jsgf_header: HEADER with up to three tokens (version, charset, locale) */
    if (x.tok != T_HEADER) {
        syntax_error(&x, "#JSGF");
        goto bad;
    }
    next_token(&x);
    while (x.tok == T_TOKEN && n_hdr < 3) {
        ++n_hdr;
        next_token(&x);
    }
    if (!is_char(&x, ';')) {
        syntax_error(&x, "';'");
        goto bad;
    }
    next_token(&x);
    /* grammar_header: GRAMMAR TOKEN ';' */
    if (x.tok != T_GRAMMAR) {
        syntax_error(&x, "grammar");
        goto bad;
    }
    next_token(&x);
    if (x.tok != T_TOKEN) {
        syntax_error(&x, "the grammar's name");
        goto bad;
    }
    if ((j->name = dup_n(x.ts, x.tlen)) == NULL) {
        ssw_set_error("out of memory parsing the JSGF grammar");
        goto bad;
    }
    next_token(&x);
    if (!is_char(&x, ';')) {
        syntax_error(&x, "';'");
        goto bad;
    }
    next_token(&x);
    while (x.tok != T_EOF) {
        int is_public = 0, n_alts;
        char *name;
        alt_t *alts;
        rule_t *r;
        if (x.tok == T_IMPORT) {
            ssw_set_error("import at line %d: imported grammars are not supported", x.line);
            goto bad;
        }
        if (x.tok == T_PUBLIC) {
            is_public = 1;
            next_token(&x);
        }
        if (x.tok != T_RULENAME) {
            syntax_error(&x, is_public ? "a rule name" : "public or a rule name");
            goto bad;
        }
        if ((name = dup_n(x.ts, x.tlen)) == NULL) {
            ssw_set_error("out of memory parsing the JSGF grammar");
            goto bad;
        }
        next_token(&x);
        if (!is_char(&x, '=')) {
            syntax_error(&x, "'='");
            free(name);
            goto bad;
        }
        next_token(&x);
        if (parse_alternatives(&x, &alts, &n_alts, 0) < 0) {
            free(name);
            goto bad;
        }
        if (!is_char(&x, ';')) {
            syntax_error(&x, "';'");
            alts_free(alts, n_alts);
            free(name);
            goto bad;
        }
        r = define_rule(j, name, alts, n_alts, is_public);
        free(name);
        if (r == NULL) {
            ssw_set_error("out of memory parsing the JSGF grammar");
            goto bad;
        }
        next_token(&x);
    }
    if (x.oom) {
        ssw_set_error("out of memory parsing the JSGF grammar");
        goto bad;
    }
    return j;
bad:
    ssw_jsgf_free(j);
    return NULL;
}

ssw_jsgf_t *
ssw_jsgf_parse_string(const char *text)
{
    if (text == NULL) {
        ssw_set_error("bad arguments to ssw_jsgf_parse_string");
        return NULL;
    }
    return parse(text, strlen(text));
}

ssw_jsgf_t *
ssw_jsgf_parse_file(const char *path)
{
    FILE *fp;
    char *buf = NULL;
    long size;
    ssw_jsgf_t *j;
    if (path == NULL) {
        ssw_set_error("bad arguments to ssw_jsgf_parse_file");
        return NULL;
    }
    if ((fp = fopen(path, "rb")) == NULL) {
        ssw_set_error("Failed to open %s for parsing", path); /* src/jsgf.c:832-835 */
        return NULL;
    }
    if (fseek(fp, 0, SEEK_END) != 0 || (size = ftell(fp)) < 0 || fseek(fp, 0, SEEK_SET) != 0
        || (buf = (char *)malloc((size_t)size + 1)) == NULL
        || fread(buf, 1, (size_t)size, fp) != (size_t)size) {
        fclose(fp);
        free(buf);
        ssw_set_error("Failed to open %s for parsing", path);
        return NULL;
    }
    fclose(fp);
    j = parse(buf, (size_t)size);
    free(buf);
    return j;
}

const char *
ssw_jsgf_name(const ssw_jsgf_t *j)
{
    return j ? j->name : NULL;
}

int32_t
ssw_jsgf_n_rules(const ssw_jsgf_t *j)
{
    return j ? j->n_tab : -1;
}

const char *
ssw_jsgf_rule_name(const ssw_jsgf_t *j, int32_t i)
{
    return (j && i >= 0 && i < j->n_tab) ? j->tab[i]->name : NULL;
}

int32_t
ssw_jsgf_rule_public(const ssw_jsgf_t *j, int32_t i)
{
    return (j && i >= 0 && i < j->n_tab) ? j->tab[i]->is_public : -1;
}

/* jsgf_get_public_rule, src/jsgf.c:444-469: the first public rule whose name starts with the
 * grammar's (up to the rule name's last dot) */
int32_t
ssw_jsgf_public_rule(const ssw_jsgf_t *j)
{
    int i;
    for (i = 0; j != NULL && i < j->n_tab; ++i)
        if (j->tab[i]->is_public) {
            const char *name = j->tab[i]->name, *dot = strrchr(name + 1, '.');
            if (dot == NULL || strncmp(name + 1, j->name, (size_t)(dot - name - 1)) == 0)
                return i;
        }
    return -1;
}

/* jsgf_get_rule, src/jsgf.c:429-442: "<" name ">" looked up verbatim */
int32_t
ssw_jsgf_find_rule(const ssw_jsgf_t *j, const char *name)
{
    char *full;
    int i;
    if (j == NULL || name == NULL || (full = (char *)malloc(strlen(name) + 3)) == NULL)
        return -1;
    sprintf(full, "<%s>", name);
    i = table_find(j, full);
    free(full);
    return i;
}

/* ---- expansion -------------------------------------------------------------------------- */
typedef struct {
    int from, to;
    const atom_t *atom; /* NULL: a rule's exit */
    const rule_t *rule; /* the rule whose expansion made the link */
} jlink_t;

typedef struct {
    ssw_jsgf_t *j;
    jlink_t *links;
    int n_links, cap_links, n_state, depth;
} expand_t;

#define EXPAND_RECURSION -2

static int
add_link(expand_t *e, const atom_t *atom, const rule_t *rule, int from, int to)
{
    if (e->n_links >= MAX_LINKS) {
        ssw_set_error("Rule %s expands to more than %d transitions", rule->name, MAX_LINKS);
        return -1;
    }
    if (e->n_links == e->cap_links) {
        const int nc = e->cap_links ? 2 * e->cap_links : 64;
        jlink_t *q = (jlink_t *)realloc(e->links, sizeof(jlink_t) * (size_t)nc);
        if (q == NULL) {
            ssw_set_error("out of memory expanding the JSGF grammar");
            return -1;
        }
        e->links = q;
        e->cap_links = nc;
    }
    e->links[e->n_links].from = from;
    e->links[e->n_links].to = to;
    e->links[e->n_links].atom = atom;
    e->links[e->n_links].rule = rule;
    ++e->n_links;
    return 0;
}

static int expand_rule(expand_t *e, rule_t *rule);

/* expand_rhs, src/jsgf.c:300-377: the last state of the sequence, EXPAND_RECURSION, or -1 */
static int
expand_alt(expand_t *e, rule_t *rule, const alt_t *alt)
{
    int last = rule->entry, i;
    for (i = 0; i < alt->n; ++i) {
        const atom_t *atom = &alt->atoms[i];
        if (atom->name[0] != '<') { /* a word and a new state */
            if (add_link(e, atom, rule, last, e->n_state) < 0)
                return -1;
            last = e->n_state++;
        } else if (!strcmp(atom->name, "<NULL>")) {
            if (add_link(e, atom, rule, last, e->n_state) < 0)
                return -1;
            last = e->n_state++;
        } else if (!strcmp(atom->name, "<VOID>")) {
            ssw_set_error("<VOID> in %s makes the alternative unspeakable: not supported",
                          rule->name);
            return -1;
        } else {
            /* jsgf_fullname_from_rule: qualified by the grammar part of the RULE's name */
            const char *dot = strrchr(rule->name + 1, '.');
            char *full = dot ? full_name(rule->name + 1, (size_t)(dot - rule->name - 1), atom->name)
                             : dup_n(atom->name, strlen(atom->name));
            rule_t *sub;
            int k;
            if (full == NULL) {
                ssw_set_error("out of memory expanding the JSGF grammar");
                return -1;
            }
            if ((k = table_find(e->j, full)) < 0) {
                ssw_set_error("Undefined rule in RHS: %s", full);
                free(full);
                return -1;
            }
            free(full);
            sub = e->j->tab[k];
            if (sub->on_stack) {
                if (i + 1 < alt->n) {
                    ssw_set_error("Only right-recursion is permitted (in %s.%s)", e->j->name,
                                  rule->name);
                    return -1;
                }
                /* a link back to the beginning of the instance on the stack */
                if (add_link(e, atom, rule, last, sub->entry) < 0)
                    return -1;
                return EXPAND_RECURSION;
            }
            if (expand_rule(e, sub) < 0 || add_link(e, atom, rule, last, sub->entry) < 0)
                return -1;
            last = sub->exit;
        }
    }
    return last;
}

/* expand_rule, src/jsgf.c:379-421 */
static int
expand_rule(expand_t *e, rule_t *rule)
{
    float norm = 0;
    int i;
    if (++e->depth > MAX_NEST) {
        ssw_set_error("rules nested more than %d deep at %s", MAX_NEST, rule->name);
        return -1;
    }
    rule->on_stack = 1;
    /* the leading weights of the alternatives, summed and divided in float32, in place */
    for (i = 0; i < rule->n_alts; ++i)
        norm += rule->alts[i].atoms[0].weight;
    rule->entry = e->n_state++;
    rule->exit = e->n_state++;
    if (norm == 0)
        norm = 1;
    for (i = 0; i < rule->n_alts; ++i) {
        int last;
        rule->alts[i].atoms[0].weight /= norm;
        if ((last = expand_alt(e, rule, &rule->alts[i])) == -1)
            return -1;
        if (last != EXPAND_RECURSION && add_link(e, NULL, rule, last, rule->exit) < 0)
            return -1;
    }
    rule->on_stack = 0;
    --e->depth;
    return rule->exit;
}

/* jsgf_build_fsg, src/jsgf.c:483-539.  It changes the grammar: the weights stay divided */
ssw_fsg_t *
ssw_jsgf_build_fsg(const ssw_model_t *m, const ssw_dict_t *d, ssw_jsgf_t *j, int32_t rule)
{
    expand_t e;
    rule_t *top;
    ssw_fsg_t *f = NULL;
    int32_t *from = NULL, *to = NULL;
    float *prob = NULL;
    const char **word = NULL;
    int i, rv;

    if (m == NULL || j == NULL || rule < 0 || rule >= j->n_tab) {
        ssw_set_error("bad arguments to ssw_jsgf_build_fsg");
        return NULL;
    }
    memset(&e, 0, sizeof(e));
    e.j = j;
    top = j->tab[rule];
    for (i = 0; i < j->n_all; ++i)
        j->all[i]->on_stack = 0;
    rv = expand_rule(&e, top);
    for (i = 0; i < j->n_all; ++i)
        j->all[i]->on_stack = 0;
    if (rv < 0)
        goto done;
    from = (int32_t *)malloc(sizeof(int32_t) * (size_t)e.n_links);
    to = (int32_t *)malloc(sizeof(int32_t) * (size_t)e.n_links);
    prob = (float *)malloc(sizeof(float) * (size_t)e.n_links);
    word = (const char **)malloc(sizeof(char *) * (size_t)e.n_links);
    if (!from || !to || !prob || !word) {
        ssw_set_error("out of memory expanding the JSGF grammar");
        goto done;
    }
    /* (glist_reverse of a list built by prepending: the order the links were made in) */
    for (i = 0; i < e.n_links; ++i) {
        const jlink_t *l = &e.links[i];
        from[i] = l->from;
        to[i] = l->to;
        prob[i] = l->atom ? l->atom->weight : 1.0f;
        word[i] = (l->atom && l->atom->name[0] != '<') ? l->atom->name : NULL;
        if (!(prob[i] > 0.0f) || prob[i] > 1.0f) {
            ssw_set_error("Rule %s: the weight of %.64s is %g after normalisation, not in (0, 1]",
                          l->rule->name, l->atom->name, (double)prob[i]);
            goto done;
        }
    }
    f = ssw_fsg_create_jsgf(m, d, top->name, e.n_state, top->entry, top->exit, e.n_links, from, to,
                            prob, word);
done:
    free(e.links);
    free(from);
    free(to);
    free(prob);
    free((void *)word);
    return f;
}

/* decoder_set_jsgf_string / _file up to decoder_set_fsg, src/decoder.c:609-683 */
static ssw_fsg_t *
from_jsgf(const ssw_model_t *m, const ssw_dict_t *d, ssw_jsgf_t *j, const char *toprule,
          const char *path)
{
    ssw_fsg_t *f = NULL;
    int rule;
    if (j == NULL)
        return NULL;
    if (toprule != NULL) {
        if ((rule = ssw_jsgf_find_rule(j, toprule)) < 0)
            ssw_set_error("Start rule %s not found", toprule);
    } else if ((rule = ssw_jsgf_public_rule(j)) < 0) {
        if (path != NULL)
            ssw_set_error("No public rules found in %s", path);
        else
            ssw_set_error("No public rules found in input string");
    }
    if (rule >= 0)
        f = ssw_jsgf_build_fsg(m, d, j, rule);
    ssw_jsgf_free(j);
    return f;
}

ssw_fsg_t *
ssw_fsg_from_jsgf_string(const ssw_model_t *m, const ssw_dict_t *d, const char *text,
                         const char *toprule)
{
    if (m == NULL || text == NULL) {
        ssw_set_error("bad arguments to ssw_fsg_from_jsgf_string");
        return NULL;
    }
    return from_jsgf(m, d, ssw_jsgf_parse_string(text), toprule, NULL);
}

ssw_fsg_t *
ssw_fsg_from_jsgf_file(const ssw_model_t *m, const ssw_dict_t *d, const char *path,
                       const char *toprule)
{
    if (m == NULL || path == NULL) {
        ssw_set_error("bad arguments to ssw_fsg_from_jsgf_file");
        return NULL;
    }
    return from_jsgf(m, d, ssw_jsgf_parse_file(path), toprule, path);
}
