/*
 * ssw_fsg_model.inc -- host C, part of ssw_fsg.c (included there): word finite-state grammars (fsg_model_t, src/fsg_model.c) and what
 * fsg_search_init makes of one before it is searched (src/fsg_search.c:84-170, 224-233).
 *
 * An ssw_fsg_t keeps the transitions as they were given (ssw_fsg_create, or the .fsg text
 * format of fsg_model_read_s3file, src/fsg_model.c:505-693).  ssw_fsg_compile turns it into the
 * reference's link lists for one configuration:
 *   - log probabilities (int32)(logmath_log(p) * lw), src/fsg_model.c:630;
 *   - fsg_model_trans_add: a link met again keeps the larger probability, a new one goes to the
 *     FRONT of the list of its (from, to) pair (:62-95);
 *   - fsg_model_null_trans_add and fsg_model_null_trans_closure: no null self loops, one null
 *     per pair with the best probability, closed transitively (:97-219);
 *   - with `searched`: fsg_search_add_silences (<sil> with silprob, then every other filler of
 *     the dictionary but <s> and </s> with fillprob, as self loops on every state) and
 *     fsg_search_add_altpron (every alternate of every word, in front of the list that holds
 *     the word, fsg_model_add_alt :388-451).  fsg_model_has_sil / _has_alt are true only after
 *     fsg_model_add_silence / _add_alt were called, which neither the reader nor create_fsg
 *     does: a grammar read from a file gets both, also one that names <sil> or an alternate
 *     itself (its own <sil> link then keeps the larger of the two probabilities);
 *   - the order fsg_model_arcs walks a state's links (:248-302): the (from, to) lists in the
 *     order of the hash table keyed by the destination state, then the nulls in the order of
 *     theirs.  Both tables have 101 buckets (hash_table_new(5): prime_size(7)) and a key is the
 *     four bytes of the state number spelt as two letters each (makekey, src/hash_table.c:
 *     208-223, key2hash :171-206); a bucket's chain is its first key, then the later ones newest
 *     first (enter, :355-395).  That order is the sibling order of a state's phone-tree roots
 *     and so decides exact score ties.
 */
#include <stdio.h>

struct ssw_fsg_s {
    char *name;
    int32_t n_state, start, final;
    int32_t n_word;
    char **vocab;   /* in order of first appearance */
    int32_t n_trans;
    int32_t *from, *to, *wid; /* wid: vocabulary index, -1 for a null transition */
    float *prob;
    double logbase;
    int32_t jsgf; /* built by jsgf_build_fsg (ssw_jsgf.c): see ssw_fsg_create_jsgf */
};

/* ---- the reference's tables, restated ------------------------------------------------ */
typedef struct {
    int to, hash;
    int n, cap;
    int *lnk; /* link pool indices, list head first */
} dest_t;
typedef struct {
    dest_t *d; /* in iteration order */
    int n, cap;
} dtab_t;
typedef struct {
    int *from, *to, *logp, *wid;
    int n, cap;
} pool_t;

static int
state_hash(int32_t to)
{
    /* makekey: byte b -> 'A' + (b & 15), 'J' + (b >> 4); key2hash: sum of c << s, s = 0, 5, ..,
     * back by 24 once it reaches 25; mod the table size */
    uint32_t hash = 0;
    int s = 0, i;
    for (i = 0; i < 4; ++i) {
        const unsigned b = ((uint32_t)to >> (8 * i)) & 0xff;
        const char c[2] = { (char)('A' + (b & 15)), (char)('J' + ((b >> 4) & 15)) };
        int k;
        for (k = 0; k < 2; ++k) {
            hash += (uint32_t)(c[k] << s);
            s += 5;
            if (s >= 25)
                s -= 24;
        }
    }
    return (int)(hash % 101u);
}

static dest_t *
dtab_find(dtab_t *t, int to)
{
    int i;
    for (i = 0; i < t->n; ++i)
        if (t->d[i].to == to)
            return &t->d[i];
    return NULL;
}

static dest_t *
dtab_insert(dtab_t *t, int to)
{
    const int h = state_hash(to);
    int a = 0, pos;
    if (t->n == t->cap) {
        const int nc = t->cap ? 2 * t->cap : 4;
        dest_t *q = (dest_t *)realloc(t->d, sizeof(dest_t) * (size_t)nc);
        if (q == NULL)
            return NULL;
        t->d = q;
        t->cap = nc;
    }
    while (a < t->n && t->d[a].hash < h)
        ++a;
    /* a bucket's chain: its first key, then the later ones newest first */
    pos = (a < t->n && t->d[a].hash == h) ? a + 1 : a;
    memmove(&t->d[pos + 1], &t->d[pos], sizeof(dest_t) * (size_t)(t->n - pos));
    memset(&t->d[pos], 0, sizeof(dest_t));
    t->d[pos].to = to;
    t->d[pos].hash = h;
    ++t->n;
    return &t->d[pos];
}

static int
dest_prepend(dest_t *d, int link)
{
    if (d->n == d->cap) {
        const int nc = d->cap ? 2 * d->cap : 4;
        int *q = (int *)realloc(d->lnk, sizeof(int) * (size_t)nc);
        if (q == NULL)
            return -1;
        d->lnk = q;
        d->cap = nc;
    }
    memmove(d->lnk + 1, d->lnk, sizeof(int) * (size_t)d->n);
    d->lnk[0] = link;
    ++d->n;
    return 0;
}

static int
pool_add(pool_t *p, int from, int to, int logp, int wid)
{
    if (p->n == p->cap) {
        const int nc = p->cap ? 2 * p->cap : 64;
        int *a = (int *)realloc(p->from, sizeof(int) * (size_t)nc);
        int *b = a ? (int *)realloc(p->to, sizeof(int) * (size_t)nc) : NULL;
        int *c = b ? (int *)realloc(p->logp, sizeof(int) * (size_t)nc) : NULL;
        int *e = c ? (int *)realloc(p->wid, sizeof(int) * (size_t)nc) : NULL;
        if (a) p->from = a;
        if (b) p->to = b;
        if (c) p->logp = c;
        if (e) p->wid = e;
        if (!e)
            return -1;
        p->cap = nc;
    }
    p->from[p->n] = from;
    p->to[p->n] = to;
    p->logp[p->n] = logp;
    p->wid[p->n] = wid;
    return p->n++;
}

typedef struct {
    pool_t pool;
    dtab_t *trans, *nulls; /* [n_state] */
    int n_state;
} model_t;

/* fsg_model_trans_add; 0, or -1 out of memory */
static int
trans_add(model_t *md, int from, int to, int logp, int wid)
{
    dest_t *d = dtab_find(&md->trans[from], to);
    int i, l;
    if (d != NULL)
        for (i = 0; i < d->n; ++i)
            if (md->pool.wid[d->lnk[i]] == wid) {
                if (md->pool.logp[d->lnk[i]] < logp)
                    md->pool.logp[d->lnk[i]] = logp;
                return 0;
            }
    if (d == NULL && (d = dtab_insert(&md->trans[from], to)) == NULL)
        return -1;
    if ((l = pool_add(&md->pool, from, to, logp, wid)) < 0)
        return -1;
    return dest_prepend(d, l);
}

/* fsg_model_null_trans_add: 1 a new link, 0 an old one made better, -1 nothing changed,
 * -2 out of memory */
static int
null_add(model_t *md, int from, int to, int logp)
{
    dest_t *d;
    int l;
    if (from == to)
        return -1;
    d = dtab_find(&md->nulls[from], to);
    if (d != NULL) {
        if (md->pool.logp[d->lnk[0]] < logp) {
            md->pool.logp[d->lnk[0]] = logp;
            return 0;
        }
        return -1;
    }
    if ((d = dtab_insert(&md->nulls[from], to)) == NULL
        || (l = pool_add(&md->pool, from, to, logp, -1)) < 0 || dest_prepend(d, l) < 0)
        return -2;
    return 1;
}

static void
model_free(model_t *md)
{
    int s, i;
    for (s = 0; s < md->n_state; ++s) {
        if (md->trans) {
            for (i = 0; i < md->trans[s].n; ++i)
                free(md->trans[s].d[i].lnk);
            free(md->trans[s].d);
        }
        if (md->nulls) {
            for (i = 0; i < md->nulls[s].n; ++i)
                free(md->nulls[s].d[i].lnk);
            free(md->nulls[s].d);
        }
    }
    free(md->trans);
    free(md->nulls);
    free(md->pool.from);
    free(md->pool.to);
    free(md->pool.logp);
    free(md->pool.wid);
}

void
ssw_fsg_compiled_free(ssw_fsg_compiled_t *c)
{
    int i;
    if (c == NULL)
        return;
    for (i = 0; i < c->n_word; ++i)
        free(c->vocab[i]);
    free(c->vocab);
    free(c->dict_wid);
    free(c->is_sil);
    free(c->links);
    free(c->state_off);
    free(c);
}

static int
vocab_add(ssw_fsg_compiled_t *c, int *cap, const char *w)
{
    int i;
    for (i = 0; i < c->n_word; ++i)
        if (!strcmp(c->vocab[i], w))
            return i;
    if (c->n_word == *cap) {
        const int nc = *cap ? 2 * *cap : 16;
        char **v = (char **)realloc(c->vocab, sizeof(char *) * (size_t)nc);
        uint8_t *s = v ? (uint8_t *)realloc(c->is_sil, (size_t)nc) : NULL;
        if (v) c->vocab = v;
        if (s) c->is_sil = s;
        if (!s)
            return -1;
        *cap = nc;
    }
    if ((c->vocab[c->n_word] = strdup(w)) == NULL)
        return -1;
    c->is_sil[c->n_word] = 0;
    return c->n_word++;
}

ssw_fsg_compiled_t *
ssw_fsg_compile(const ssw_fsg_t *f, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg_in,
                int searched)
{
    ssw_first_pass_config_t cfg;
    ssw_fsg_compiled_t *c = (ssw_fsg_compiled_t *)calloc(1, sizeof(*c));
    model_t md;
    int cap_vocab = 0, i, s, k;
    int *nl_link = NULL, *nl_next = NULL, nl_n = 0, nl_cap = 0, nl_head = -1;

    if (cfg_in)
        cfg = *cfg_in;
    else
        ssw_first_pass_config_defaults(&cfg);
    memset(&md, 0, sizeof(md));
    if (c == NULL)
        goto oom;
    md.n_state = f->n_state;
    md.trans = (dtab_t *)calloc((size_t)(f->n_state ? f->n_state : 1), sizeof(dtab_t));
    md.nulls = (dtab_t *)calloc((size_t)(f->n_state ? f->n_state : 1), sizeof(dtab_t));
    if (!md.trans || !md.nulls)
        goto oom;
    c->n_state = f->n_state;
    c->start = f->start;
    c->final = f->final;
    for (i = 0; i < f->n_word; ++i)
        if (vocab_add(c, &cap_vocab, f->vocab[i]) < 0)
            goto oom;
    /* the transitions in the order given; the nulls met are listed newest first.
     * jsgf_build_fsg_internal (src/jsgf.c:508-525) hands logmath_log(weight) over as it is,
     * without the language weight the .fsg reader multiplies in (src/fsg_model.c:630) */
    for (i = 0; i < f->n_trans; ++i) {
        const int logp = f->jsgf ? ilog0(f->logbase, (double)f->prob[i])
                                 : (int32_t)((float)ilog0(f->logbase, (double)f->prob[i]) * cfg.lw);
        if (f->wid[i] >= 0) {
            if (trans_add(&md, f->from[i], f->to[i], logp, f->wid[i]) < 0)
                goto oom;
        } else {
            const int r = null_add(&md, f->from[i], f->to[i], logp);
            if (r == -2)
                goto oom;
            if (r == 1 && !f->jsgf) {
                if (nl_n == nl_cap) {
                    const int nc = nl_cap ? 2 * nl_cap : 32;
                    int *a = (int *)realloc(nl_link, sizeof(int) * (size_t)nc);
                    int *b = a ? (int *)realloc(nl_next, sizeof(int) * (size_t)nc) : NULL;
                    if (a) nl_link = a;
                    if (b) nl_next = b;
                    if (!b)
                        goto oom;
                    nl_cap = nc;
                }
                nl_link[nl_n] = dtab_find(&md.nulls[f->from[i]], f->to[i])->lnk[0];
                nl_next[nl_n] = nl_head;
                nl_head = nl_n++;
            }
        }
    }
    /* jsgf_build_fsg calls the closure without a list, which then makes its own: every state's
     * null transitions in the order of its table, each put in FRONT (src/fsg_model.c:164-176) */
    if (f->jsgf)
        for (s = 0; s < f->n_state; ++s)
            for (k = 0; k < md.nulls[s].n; ++k) {
                if (nl_n == nl_cap) {
                    const int nc = nl_cap ? 2 * nl_cap : 32;
                    int *a = (int *)realloc(nl_link, sizeof(int) * (size_t)nc);
                    int *b = a ? (int *)realloc(nl_next, sizeof(int) * (size_t)nc) : NULL;
                    if (a) nl_link = a;
                    if (b) nl_next = b;
                    if (!b)
                        goto oom;
                    nl_cap = nc;
                }
                nl_link[nl_n] = md.nulls[s].d[k].lnk[0];
                nl_next[nl_n] = nl_head;
                nl_head = nl_n++;
            }
    /* fsg_model_null_trans_closure, src/fsg_model.c:178-215 */
    for (;;) {
        int updated = 0, gn;
        for (gn = nl_head; gn >= 0; gn = nl_next[gn]) {
            const int l1 = nl_link[gn];
            const int mid = md.pool.to[l1];
            int j;
            for (j = 0; j < md.nulls[mid].n; ++j) {
                const int l2 = md.nulls[mid].d[j].lnk[0];
                const int from = md.pool.from[l1], to = md.pool.to[l2];
                const int r = null_add(&md, from, to, md.pool.logp[l1] + md.pool.logp[l2]);
                if (r == -2)
                    goto oom;
                if (r >= 0) {
                    updated = 1;
                    if (r > 0) {
                        if (nl_n == nl_cap) {
                            const int nc = nl_cap ? 2 * nl_cap : 32;
                            int *a = (int *)realloc(nl_link, sizeof(int) * (size_t)nc);
                            int *b = a ? (int *)realloc(nl_next, sizeof(int) * (size_t)nc) : NULL;
                            if (a) nl_link = a;
                            if (b) nl_next = b;
                            if (!b)
                                goto oom;
                            nl_cap = nc;
                        }
                        nl_link[nl_n] = dtab_find(&md.nulls[from], to)->lnk[0];
                        nl_next[nl_n] = nl_head;
                        nl_head = nl_n++;
                        /* (a table that grew may have moved: index it afresh) */
                    }
                }
            }
        }
        if (!updated)
            break;
    }
    if (searched && cfg.use_filler) {
        /* fsg_search_add_silences: <sil>, then dict_filler_start .. dict_filler_end - 1 (the
         * last filler word is dict_filler_end itself and is left out), <s> and </s> skipped */
        const int sw = ssw_dict_find(d, "<sil>"), start = ssw_dict_find(d, "<s>"),
                  fin = ssw_dict_find(d, "</s>");
        const int logsil = (int32_t)((float)ilog0(f->logbase, (double)cfg.silprob) * cfg.lw);
        const int logfil = (int32_t)((float)ilog0(f->logbase, (double)cfg.fillprob) * cfg.lw);
        int fw;
        for (fw = -1; fw < d->filler_end; fw = (fw < 0 ? d->filler_start : fw + 1)) {
            const int w = fw < 0 ? sw : fw;
            int vid;
            if (w < 0 || (fw >= 0 && (w == start || w == fin)))
                continue;
            if ((vid = vocab_add(c, &cap_vocab, d->word[w])) < 0)
                goto oom;
            c->is_sil[vid] = 1;
            for (s = 0; s < f->n_state; ++s)
                if (trans_add(&md, s, s, (fw < 0) ? logsil : logfil, vid) < 0)
                    goto oom;
        }
    }
    if (searched && cfg.use_altpron) {
        /* fsg_search_add_altpron over the vocabulary as it stands now */
        const int n_word = c->n_word;
        for (i = 0; i < n_word; ++i) {
            int w = ssw_dict_find(d, c->vocab[i]);
            if (w < 0)
                continue;
            while ((w = d->alt[w]) >= 0) {
                const int avid = vocab_add(c, &cap_vocab, d->word[w]);
                if (avid < 0)
                    goto oom;
                if (c->is_sil[i])
                    c->is_sil[avid] = 1;
                for (s = 0; s < f->n_state; ++s) {
                    int j;
                    for (j = 0; j < md.trans[s].n; ++j) {
                        dest_t *dd = &md.trans[s].d[j];
                        const int n0 = dd->n;
                        int added = 0;
                        /* every link of the list as it was that carries the word gets a copy
                         * in front of the list */
                        for (k = 0; k < n0; ++k) {
                            const int l = dd->lnk[k + added];
                            if (md.pool.wid[l] == i) {
                                const int nl2 = pool_add(&md.pool, md.pool.from[l], md.pool.to[l],
                                                         md.pool.logp[l], avid);
                                if (nl2 < 0 || dest_prepend(dd, nl2) < 0)
                                    goto oom;
                                ++added;
                            }
                        }
                    }
                }
            }
        }
    }
    /* flatten in fsg_model_arcs order */
    c->state_off = (int32_t *)calloc((size_t)f->n_state + 1, sizeof(int32_t));
    c->links = (ssw_fsg_link_t *)malloc(sizeof(ssw_fsg_link_t) * (size_t)(md.pool.n ? md.pool.n : 1));
    c->dict_wid = (int32_t *)malloc(sizeof(int32_t) * (size_t)(c->n_word ? c->n_word : 1));
    if (!c->state_off || !c->links || !c->dict_wid)
        goto oom;
    for (i = 0; i < c->n_word; ++i)
        c->dict_wid[i] = d ? ssw_dict_find(d, c->vocab[i]) : -1;
    for (s = 0; s < f->n_state; ++s) {
        int j, pass;
        c->state_off[s] = c->n_links;
        for (pass = 0; pass < 2; ++pass) {
            const dtab_t *t = pass ? &md.nulls[s] : &md.trans[s];
            for (j = 0; j < t->n; ++j)
                for (k = 0; k < t->d[j].n; ++k) {
                    const int l = t->d[j].lnk[k];
                    ssw_fsg_link_t *o = &c->links[c->n_links++];
                    o->from = md.pool.from[l];
                    o->to = md.pool.to[l];
                    o->logp = md.pool.logp[l];
                    o->wid = md.pool.wid[l];
                }
        }
    }
    c->state_off[f->n_state] = c->n_links;
    c->lw = cfg.lw;
    c->logbase = f->logbase;
    model_free(&md);
    free(nl_link);
    free(nl_next);
    return c;
oom:
    ssw_set_error("out of memory compiling the grammar");
    model_free(&md);
    free(nl_link);
    free(nl_next);
    ssw_fsg_compiled_free(c);
    return NULL;
}

/* ---- the object ----------------------------------------------------------------------- */
void
ssw_fsg_free(ssw_fsg_t *f)
{
    int i;
    if (f == NULL)
        return;
    for (i = 0; i < f->n_word; ++i)
        free(f->vocab[i]);
    free(f->vocab);
    free(f->name);
    free(f->from);
    free(f->to);
    free(f->wid);
    free(f->prob);
    free(f);
}

static ssw_fsg_t *
fsg_new(const ssw_model_t *m, const char *name, int n_state)
{
    ssw_fsg_t *f = (ssw_fsg_t *)calloc(1, sizeof(*f));
    if (f == NULL || (f->name = strdup(name ? name : "")) == NULL) {
        free(f);
        ssw_set_error("out of memory");
        return NULL;
    }
    f->n_state = n_state;
    f->logbase = ssw_model_host(m)->cfg.logbase;
    return f;
}

/* one more transition; word NULL or "" = null.  0, or -1 out of memory */
static int
fsg_push(ssw_fsg_t *f, int *cap_t, int *cap_w, int from, int to, float prob, const char *word)
{
    int wid = -1, i;
    if (word != NULL && word[0] != '\0') {
        for (i = 0; i < f->n_word; ++i)
            if (!strcmp(f->vocab[i], word))
                break;
        if (i == f->n_word) {
            if (f->n_word == *cap_w) {
                const int nc = *cap_w ? 2 * *cap_w : 16;
                char **v = (char **)realloc(f->vocab, sizeof(char *) * (size_t)nc);
                if (v == NULL)
                    return -1;
                f->vocab = v;
                *cap_w = nc;
            }
            if ((f->vocab[f->n_word] = strdup(word)) == NULL)
                return -1;
            ++f->n_word;
        }
        wid = i;
    }
    if (f->n_trans == *cap_t) {
        const int nc = *cap_t ? 2 * *cap_t : 32;
        int *a = (int *)realloc(f->from, sizeof(int) * (size_t)nc);
        int *b = a ? (int *)realloc(f->to, sizeof(int) * (size_t)nc) : NULL;
        int *c = b ? (int *)realloc(f->wid, sizeof(int) * (size_t)nc) : NULL;
        float *p = c ? (float *)realloc(f->prob, sizeof(float) * (size_t)nc) : NULL;
        if (a) f->from = a;
        if (b) f->to = b;
        if (c) f->wid = c;
        if (p) f->prob = p;
        if (!p)
            return -1;
        *cap_t = nc;
    }
    f->from[f->n_trans] = from;
    f->to[f->n_trans] = to;
    f->wid[f->n_trans] = wid;
    f->prob[f->n_trans] = prob;
    ++f->n_trans;
    return 0;
}

/* fsg_search_check_dict, src/fsg_search.c:120-141 */
static int
check_dict(const ssw_fsg_t *f, const ssw_dict_t *d)
{
    int i;
    for (i = 0; d != NULL && i < f->n_word; ++i)
        if (ssw_dict_find(d, f->vocab[i]) < 0) {
            ssw_set_error("The word '%s' is missing in the dictionary", f->vocab[i]);
            return -1;
        }
    return 0;
}

ssw_fsg_t *
ssw_fsg_create(const ssw_model_t *m, const ssw_dict_t *d, const char *name, int32_t n_states,
               int32_t start, int32_t final, int32_t n_trans, const int32_t *from,
               const int32_t *to, const float *prob, const char *const *word)
{
    ssw_fsg_t *f;
    int cap_t = 0, cap_w = 0, i;
    if (m == NULL || n_states < 1 || n_trans < 0 || (n_trans > 0 && (!from || !to || !prob))) {
        ssw_set_error("bad arguments to ssw_fsg_create");
        return NULL;
    }
    if (ssw_model_host(m)->n_ciphone > 64) {
        ssw_set_error("%d CI phones: the grammar search handles at most 64",
                      ssw_model_host(m)->n_ciphone);
        return NULL;
    }
    if (start < 0 || start >= n_states) {
        ssw_set_error("START_STATE declaration malformed");
        return NULL;
    }
    if (final < 0 || final >= n_states) {
        ssw_set_error("FINAL_STATE declaration malformed");
        return NULL;
    }
    if ((f = fsg_new(m, name, n_states)) == NULL)
        return NULL;
    f->start = start;
    f->final = final;
    for (i = 0; i < n_trans; ++i) {
        if (from[i] < 0 || from[i] >= n_states) {
            ssw_set_error("Invalid from-state %d", from[i]);
            goto bad;
        }
        if (to[i] < 0 || to[i] >= n_states) {
            ssw_set_error("Invalid to-state %d", to[i]);
            goto bad;
        }
        if (!(prob[i] > 0.0f) || prob[i] > 1.0f) {
            ssw_set_error("Transition %d: transition spec malformed; Expecting float as transition "
                          "probability", i);
            goto bad;
        }
        if (fsg_push(f, &cap_t, &cap_w, from[i], to[i], prob[i], word ? word[i] : NULL) < 0) {
            ssw_set_error("out of memory");
            goto bad;
        }
    }
    if (check_dict(f, d) < 0)
        goto bad;
    return f;
bad:
    ssw_fsg_free(f);
    return NULL;
}

/* ssw_fsg_create for the transitions jsgf_build_fsg_internal adds (src/jsgf.c:483-532): their
 * log probabilities take no language weight, and the closure lists the null transitions itself */
ssw_fsg_t *
ssw_fsg_create_jsgf(const ssw_model_t *m, const ssw_dict_t *d, const char *name, int32_t n_states,
                    int32_t start, int32_t final, int32_t n_trans, const int32_t *from,
                    const int32_t *to, const float *prob, const char *const *word)
{
    ssw_fsg_t *f = ssw_fsg_create(m, d, name, n_states, start, final, n_trans, from, to, prob, word);
    if (f != NULL)
        f->jsgf = 1;
    return f;
}

/* s3file_nextword: the next run of non-blank characters of the line; NULL at its end */
static const char *
next_word(const char **ptr, int *len)
{
    const char *p = *ptr, *w;
    while (*p == ' ' || *p == '\t' || *p == '\r')
        ++p;
    if (*p == '\0' || *p == '\n')
        return NULL;
    w = p;
    while (*p != '\0' && *p != '\n' && *p != ' ' && *p != '\t' && *p != '\r')
        ++p;
    *len = (int)(p - w);
    *ptr = p;
    return w;
}

/* the reference compares a line's first word with a keyword over the WORD's length
 * (strncmp(word, keyword, ptr - word)): a prefix of the keyword passes too */
static int
is_kw(const char *w, int len, const char *kw)
{
    return strncmp(w, kw, (size_t)len) == 0;
}

/* copy_header_value, src/fsg_model.c:473-503: skip lines until one starts with the keyword */
static int
header_value(char **lines, int n_lines, int *at, const char *name, const char *shortname,
             char *val, size_t val_len)
{
    while (*at < n_lines) {
        const char *line = lines[(*at)++], *ptr = line, *w;
        int len;
        if (*line == '#')
            continue;
        if ((w = next_word(&ptr, &len)) == NULL)
            continue;
        if ((shortname && is_kw(w, len, shortname)) || (name && is_kw(w, len, name))) {
            val[0] = '\0';
            if ((w = next_word(&ptr, &len)) != NULL)
                snprintf(val, val_len, "%.*s", len, w);
            return w != NULL;
        }
    }
    return -1;
}

ssw_fsg_t *
ssw_fsg_read(const ssw_model_t *m, const ssw_dict_t *d, const char *path)
{
    FILE *fp;
    char *buf = NULL, **lines = NULL, val[256], *endp;
    long size;
    int n_lines = 0, cap_lines = 0, at = 0, cap_t = 0, cap_w = 0, r;
    long n_state;
    ssw_fsg_t *f = NULL;

    if (m == NULL || path == NULL) {
        ssw_set_error("bad arguments to ssw_fsg_read");
        return NULL;
    }
    if (ssw_model_host(m)->n_ciphone > 64) {
        ssw_set_error("%d CI phones: the grammar search handles at most 64",
                      ssw_model_host(m)->n_ciphone);
        return NULL;
    }
    if ((fp = fopen(path, "rb")) == NULL) {
        ssw_set_error("Failed to open FSG file '%s' for reading", path);
        return NULL;
    }
    if (fseek(fp, 0, SEEK_END) != 0 || (size = ftell(fp)) < 0 || fseek(fp, 0, SEEK_SET) != 0
        || (buf = (char *)malloc((size_t)size + 1)) == NULL
        || fread(buf, 1, (size_t)size, fp) != (size_t)size) {
        fclose(fp);
        free(buf);
        ssw_set_error("Failed to open FSG file '%s' for reading", path);
        return NULL;
    }
    fclose(fp);
    buf[size] = '\0';
    {
        char *p = buf;
        while (*p) {
            char *e = strchr(p, '\n');
            if (n_lines == cap_lines) {
                const int nc = cap_lines ? 2 * cap_lines : 64;
                char **q = (char **)realloc(lines, sizeof(char *) * (size_t)nc);
                if (q == NULL) {
                    ssw_set_error("out of memory");
                    goto bad;
                }
                lines = q;
                cap_lines = nc;
            }
            lines[n_lines++] = p;
            if (e == NULL)
                break;
            *e = '\0';
            p = e + 1;
        }
    }
    if ((r = header_value(lines, n_lines, &at, "FSG_BEGIN", NULL, val, sizeof(val))) < 0) {
        ssw_set_error("FSG_BEGIN declaration missing");
        goto bad;
    }
    {
        char name[256];
        snprintf(name, sizeof(name), "%s", val);
        if (header_value(lines, n_lines, &at, "NUM_STATES", "N", val, sizeof(val)) < 0) {
            ssw_set_error("NUM_STATES declaration missing");
            goto bad;
        }
        n_state = strtol(val, &endp, 10);
        if (endp == val || n_state < 0 || n_state > 0x7fffffff) {
            ssw_set_error("NUM_STATES declaration malformed");
            goto bad;
        }
        if ((f = fsg_new(m, name, (int)n_state)) == NULL)
            goto bad;
    }
    if (header_value(lines, n_lines, &at, "START_STATE", "S", val, sizeof(val)) < 0) {
        ssw_set_error("START_STATE declaration missing");
        goto bad;
    }
    f->start = (int)strtol(val, &endp, 10);
    if (endp == val || f->start < 0 || f->start >= f->n_state) {
        ssw_set_error("START_STATE declaration malformed");
        goto bad;
    }
    if (header_value(lines, n_lines, &at, "FINAL_STATE", "F", val, sizeof(val)) < 0) {
        ssw_set_error("FINAL_STATE declaration missing");
        goto bad;
    }
    f->final = (int)strtol(val, &endp, 10);
    if (endp == val || f->final < 0 || f->final >= f->n_state) {
        ssw_set_error("FINAL_STATE declaration malformed");
        goto bad;
    }
    while (at < n_lines) {
        const char *line = lines[at++], *ptr = line, *w;
        const int lineno = at;
        int len;
        if (*line == '#')
            continue;
        if ((w = next_word(&ptr, &len)) == NULL)
            continue;
        if (is_kw(w, len, "FSG_END"))
            break;
        if (is_kw(w, len, "T") || is_kw(w, len, "TRANSITION")) {
            char num[64], word[512];
            int i, j;
            float p;
            if ((w = next_word(&ptr, &len)) == NULL) {
                ssw_set_error("Line[%d]: from-state missing", lineno);
                goto bad;
            }
            snprintf(num, sizeof(num), "%.*s", len, w);
            i = (int)strtol(num, &endp, 10);
            if (endp == num || i < 0 || i >= f->n_state) {
                ssw_set_error("Invalid from-state %d", i);
                goto bad;
            }
            if ((w = next_word(&ptr, &len)) == NULL) {
                ssw_set_error("Line[%d]: to-state missing", lineno);
                goto bad;
            }
            snprintf(num, sizeof(num), "%.*s", len, w);
            j = (int)strtol(num, &endp, 10);
            if (endp == num || j < 0 || j >= f->n_state) {
                ssw_set_error("Invalid to-state %d", j);
                goto bad;
            }
            if ((w = next_word(&ptr, &len)) == NULL) {
                ssw_set_error("Line[%d]: trans-prob missing", lineno);
                goto bad;
            }
            snprintf(num, sizeof(num), "%.*s", len, w);
            p = (float)atof(num);
            if ((p <= 0.0) || (p > 1.0)) {
                ssw_set_error("Line[%d]: transition spec malformed; Expecting float as transition "
                              "probability", lineno);
                goto bad;
            }
            word[0] = '\0';
            if ((w = next_word(&ptr, &len)) != NULL)
                snprintf(word, sizeof(word), "%.*s", len, w);
            if (fsg_push(f, &cap_t, &cap_w, i, j, p, word) < 0) {
                ssw_set_error("out of memory");
                goto bad;
            }
        }
    }
    if (check_dict(f, d) < 0)
        goto bad;
    free(lines);
    free(buf);
    return f;
bad:
    free(lines);
    free(buf);
    ssw_fsg_free(f);
    return NULL;
}

const char *
ssw_fsg_name(const ssw_fsg_t *f)
{
    return f ? f->name : NULL;
}

int32_t
ssw_fsg_n_states(const ssw_fsg_t *f)
{
    return f ? f->n_state : -1;
}

/* fsg_model_write, src/fsg_model.c:764-793 */
int32_t
ssw_fsg_write(const ssw_fsg_t *f, const ssw_dict_t *d, const ssw_first_pass_config_t *cfg,
              int32_t searched, char *out, int32_t out_len)
{
    ssw_fsg_compiled_t *c;
    size_t len = 0, cap = out_len > 0 ? (size_t)out_len : 0;
    char line[1024];
    int i, n;
    if (f == NULL || (searched && d == NULL)) {
        ssw_set_error("bad arguments to ssw_fsg_write");
        return -1;
    }
    if ((c = ssw_fsg_compile(f, d, cfg, searched)) == NULL)
        return -1;
#define PUT()                                                                      \
    do {                                                                           \
        if (n >= (int)sizeof(line)) /* (a JSGF token may be longer than the line) */ \
            n = (int)sizeof(line) - 1;                                             \
        if (out != NULL && len < cap) {                                            \
            const size_t room = cap - len - 1;                                     \
            memcpy(out + len, line, (size_t)n < room ? (size_t)n : room);          \
        }                                                                          \
        len += (size_t)n;                                                          \
    } while (0)
    n = snprintf(line, sizeof(line), "FSG_BEGIN %s\nNUM_STATES %d\nSTART_STATE %d\nFINAL_STATE %d\n",
                 f->name, c->n_state, c->start, c->final);
    PUT();
    for (i = 0; i < c->n_links; ++i) {
        const ssw_fsg_link_t *l = &c->links[i];
        /* logmath_exp(lmath, (int32)(logs2prob / lw)): an int divided by a float32 */
        const int32_t lg = (int32_t)((float)l->logp / c->lw);
        n = snprintf(line, sizeof(line), "TRANSITION %d %d %f %s\n", l->from, l->to,
                     pow(c->logbase, (double)lg), l->wid < 0 ? "" : c->vocab[l->wid]);
        PUT();
    }
    n = snprintf(line, sizeof(line), "FSG_END\n");
    PUT();
#undef PUT
    if (out != NULL && cap > 0)
        out[len < cap ? len : cap - 1] = '\0';
    ssw_fsg_compiled_free(c);
    return (int32_t)len;
}
