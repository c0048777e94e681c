/* slot_layout, senone_shape and slot_layout_prefix_fits (csrc/ssw_slot_layout.inc) on the CPU.
 * Tables: the files named on the command line (name n_cb path: raw int16 sen2cb, the shipped
 * models' -- tests/test_slot_layout_host.py writes them) and synthetic ones: one codebook, every
 * id isolated, runs of every length 1..9, a codebook with no senone, seeded random ones.
 * For both layouts of every table: every senone exactly once, groups in codebook order with
 * ascending ids, quad_s0 / quad_n against the slots; dense: equal to the loop it replaced, kept
 * here verbatim as it stood in upload_model; prefix: every quad s0 .. s0 + n - 1 then padding,
 * padding only where a run of consecutive ids ends.  One line per table for the test to read:
 *   table NAME dense Q prefix Q short K fits 0|1 shape2 R THREADS shape1 R THREADS
 * Built with -fsanitize=address,undefined. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../soundswallower_amd/csrc/ssw_slot_layout.inc"

static uint32_t rng_state = 0x5eed2026u;
static uint32_t
rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

#define FAIL(...)                                                                            \
    do {                                                                                     \
        printf("FAILED %s: ", name);                                                         \
        printf(__VA_ARGS__);                                                                 \
        printf("\n");                                                                        \
        return false;                                                                        \
    } while (0)

/* what both layouts promise */
static bool
check_common(const char *name, const SlotLayout &L, const std::vector<int16_t> &s2c, int n_cb)
{
    const int n_sen = (int)s2c.size();
    const size_t n_quads = L.quad_cb.size();
    if (L.slot_sen.size() != 4 * n_quads || L.quad_s0.size() != n_quads || L.quad_n.size() != n_quads)
        FAIL("sizes: %zu slots, %zu quads", L.slot_sen.size(), n_quads);
    std::vector<int> seen((size_t)n_sen, 0);
    int last_cb = -1, last_id = -1;
    for (size_t q = 0; q < n_quads; ++q) {
        const int cb = L.quad_cb[q];
        if (cb < last_cb || cb >= n_cb)
            FAIL("quad %zu: codebook %d after %d", q, cb, last_cb);
        if (cb != last_cb)
            last_id = -1;
        last_cb = cb;
        const int16_t *sj = &L.slot_sen[4 * q];
        if (sj[0] < 0)
            FAIL("quad %zu begins with padding", q);
        for (int j = 0; j < 4; ++j) {
            if (sj[j] < 0)
                continue;
            if (sj[j] >= n_sen || s2c[(size_t)sj[j]] != cb)
                FAIL("quad %zu slot %d: senone %d is not of codebook %d", q, j, sj[j], cb);
            if (sj[j] <= last_id)
                FAIL("quad %zu slot %d: id %d after %d", q, j, sj[j], last_id);
            last_id = sj[j];
            ++seen[(size_t)sj[j]];
        }
        /* quad_s0 / quad_n against the slots: n consecutive ids, then nothing but padding */
        int n = 1;
        while (n < 4 && sj[n] == sj[0] + n)
            ++n;
        bool form = true;
        for (int j = n; j < 4; ++j)
            form = form && sj[j] < 0;
        if (L.quad_s0[q] != sj[0] || L.quad_n[q] != (form ? n : 0))
            FAIL("quad %zu: s0 %d n %d, its slots say %d %d", q, L.quad_s0[q], L.quad_n[q], sj[0],
                 form ? n : 0);
    }
    for (int i = 0; i < n_sen; ++i)
        if (seen[(size_t)i] != 1)
            FAIL("senone %d appears %d times", i, seen[(size_t)i]);
    return true;
}

static bool
check_table(const char *name, const std::vector<int16_t> &s2c, int n_cb)
{
    const int n_sen = (int)s2c.size();
    /* exactly n_sen entries: an overrun of the table is an ASan report */
    const SlotLayout D = slot_layout(s2c.data(), n_sen, n_cb, false);
    const SlotLayout P = slot_layout(s2c.data(), n_sen, n_cb, true);
    if (!check_common(name, D, s2c, n_cb) || !check_common(name, P, s2c, n_cb))
        return false;
    {
        /* ---- the loop the dense layout replaced, verbatim (h-> bound to locals) ---- */
        std::vector<int16_t> slot_sen;
        std::vector<uint8_t> quad_cb;
        for (int c = 0; c < n_cb; ++c) {
            size_t start = slot_sen.size();
            for (int i = 0; i < n_sen; ++i)
                if (s2c[i] == c)
                    slot_sen.push_back((int16_t)i);
            while ((slot_sen.size() - start) % 4)
                slot_sen.push_back(-1);
            for (size_t q = start / 4; q < slot_sen.size() / 4; ++q)
                quad_cb.push_back((uint8_t)c);
        }
        /* ---- */
        if (slot_sen != D.slot_sen || quad_cb != D.quad_cb)
            FAIL("the dense layout is not the loop it replaced");
    }
    /* prefix: every quad has the form, and padding stands only where a run ends */
    int n_short = 0, n_runs = 0;
    for (size_t q = 0; q < P.quad_cb.size(); ++q) {
        const int n = P.quad_n[q];
        if (n < 1 || n > 4)
            FAIL("prefix quad %zu: n = %d", q, n);
        const int s0 = P.quad_s0[q];
        const bool begins_run = s0 == 0 || s2c[(size_t)s0 - 1] != P.quad_cb[q];
        n_runs += begins_run;
        if (!begins_run && (q == 0 || P.quad_cb[q - 1] != P.quad_cb[q] || P.quad_n[q - 1] != 4
                            || P.quad_s0[q - 1] + 4 != s0))
            FAIL("prefix quad %zu continues a run its neighbour does not hold", q);
        if (n < 4) {
            ++n_short;
            const int next = s0 + n; /* the run ends here: the next id is of another codebook */
            if (next < n_sen && s2c[(size_t)next] == P.quad_cb[q])
                FAIL("prefix quad %zu: padding inside a run (senone %d follows)", q, next);
        }
    }
    if (P.quad_cb.size() < D.quad_cb.size() || P.quad_cb.size() > D.quad_cb.size() + (size_t)n_runs)
        FAIL("%zu prefix quads against %zu dense ones and %d runs", P.quad_cb.size(),
             D.quad_cb.size(), n_runs);
    const int dq = (int)D.quad_cb.size(), pq = (int)P.quad_cb.size();
    const bool fits = slot_layout_prefix_fits(dq, pq, 1024);
    /* the rule, said the other way round: no shape of the prefix layout is larger */
    bool larger = false;
    for (int fpb = 1; fpb <= 2; ++fpb)
        for (int seven = 0; seven < 2; ++seven) {
            const SenoneShape d = senone_shape(dq, fpb, seven != 0, 0, 1024);
            const SenoneShape p = senone_shape(pq, fpb, seven != 0, 0, 1024);
            if (d.threads % 64 || d.threads < 256 || d.R < 1 || (long)d.R * d.threads < dq)
                FAIL("shape of %d quads: R %d, %d threads", dq, d.R, d.threads);
            larger = larger || p.R > d.R || p.threads > d.threads;
        }
    if (fits == larger)
        FAIL("slot_layout_prefix_fits = %d, a larger shape = %d", (int)fits, (int)larger);
    const SenoneShape s2 = senone_shape(fits ? pq : dq, 2, true, 0, 1024);
    const SenoneShape s1 = senone_shape(fits ? pq : dq, 1, true, 0, 1024);
    printf("table %s dense %d prefix %d short %d fits %d shape2 %d %d shape1 %d %d\n", name, dq, pq,
           n_short, (int)fits, s2.R, s2.threads, s1.R, s1.threads);
    return true;
}

int
main(int argc, char **argv)
{
    long n_tables = 0;
    for (int a = 1; a + 2 < argc; a += 3) {
        FILE *fp = fopen(argv[a + 2], "rb");
        if (fp == NULL) {
            printf("FAILED: cannot read %s\n", argv[a + 2]);
            return 1;
        }
        std::vector<int16_t> s2c;
        int16_t v;
        while (fread(&v, sizeof(v), 1, fp) == 1)
            s2c.push_back(v);
        fclose(fp);
        if (!check_table(argv[a], s2c, atoi(argv[a + 1])))
            return 1;
        ++n_tables;
    }
    {   /* one codebook: a single run */
        std::vector<int16_t> s2c(4099, 0);
        if (!check_table("one-codebook", s2c, 1))
            return 1;
        ++n_tables;
    }
    {   /* every id isolated: neighbours never share a codebook */
        std::vector<int16_t> s2c(4000);
        for (size_t i = 0; i < s2c.size(); ++i)
            s2c[i] = (int16_t)(i % 40);
        if (!check_table("isolated", s2c, 40))
            return 1;
        ++n_tables;
    }
    {   /* runs of every length 1..9, two codebooks taking turns; codebook 2 of 4 has no senone */
        std::vector<int16_t> s2c;
        for (int rep = 0; rep < 3; ++rep)
            for (int len = 1; len <= 9; ++len)
                for (int k = 0; k < len; ++k)
                    s2c.push_back((int16_t)((len & 1) ? (rep == 1 ? 3 : 0) : 1));
        if (!check_table("runs-1-9", s2c, 4))
            return 1;
        ++n_tables;
    }
    {   /* no senone at all in the first and the last codebook */
        std::vector<int16_t> s2c(37, 1);
        if (!check_table("empty-codebooks", s2c, 3))
            return 1;
        ++n_tables;
    }
    for (int t = 0; t < 24; ++t) { /* random run lengths and codebook counts */
        const int n_cb = 1 + (int)(rnd() % 48), max_run = 1 + (int)(rnd() % 40);
        std::vector<int16_t> s2c;
        const size_t n_sen = 1 + rnd() % 6000;
        while (s2c.size() < n_sen) {
            const int cb = (int)(rnd() % (uint32_t)n_cb), len = 1 + (int)(rnd() % (uint32_t)max_run);
            for (int k = 0; k < len && s2c.size() < n_sen; ++k)
                s2c.push_back((int16_t)cb);
        }
        const std::string nm = "random-" + std::to_string(t);
        if (!check_table(nm.c_str(), s2c, n_cb))
            return 1;
        ++n_tables;
    }
    printf("ok: %ld tables\n", n_tables);
    return 0;
}
