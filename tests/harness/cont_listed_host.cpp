// Host checks of what cont_listed_kernel (soundswallower_amd/csrc/ssw_k11_cont.inc) takes from the
// host and from plain functions, in one stand-alone program; tests/test_cont_listed_host.py
// builds it with -fsanitize=address,undefined from this file and ssw_model.c and runs it as a
// process of its own.
//
//   usage: cont_listed_host ( table DIR TOPN | select | rows )...
//       table   the continuous model in DIR (means, variances, mixture_weights, no mdef) loads,
//               ssw_host_build_cont_sm gives, for every (senone, stream, density, dimension),
//               exactly the floats of the mean, var and det tables where the layout says they
//               are, zeros in the padding, and the same again when it is rebuilt in place
//       select  cont_select_rank (ssw_cont_select.inc, the text the kernel includes) against the
//               sequential cont_insert: 1 to 5 densities, distances drawn from {WORST_DIST - 2^8,
//               WORST_DIST, 0, 1, NaN}, topn 1 to 5, equal ids and distances slot for slot
//       rows    cont_active_rows (ssw_active_set.inc): the bitmap row of every frame against a
//               frame-by-frame restatement of the active set and of acmod_flags2list's bridges,
//               with and without a seed, and its two refusals
//   Prints "ok ..." per check and exits 0; exits 1 saying what went wrong.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ssw_internal.h"

#define SSW_CONT_SEL_FN static inline
#include "ssw_cont_select.inc"
#include "ssw_active_set.inc"

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int
check_table(const char *dir, int topn)
{
    char p[3][600];
    ssw_config_t cfg;
    ssw_config_defaults(&cfg);
    cfg.topn = topn;
    cfg.device = SSW_DEVICE_NONE;
    snprintf(p[0], sizeof p[0], "%s/means", dir);
    snprintf(p[1], sizeof p[1], "%s/variances", dir);
    snprintf(p[2], sizeof p[2], "%s/mixture_weights", dir);
    ssw_host_model_t *h = ssw_host_model_load(NULL, p[0], p[1], NULL, p[2], NULL, &cfg);
    if (h == NULL) {
        fprintf(stderr, "%s: %s\n", dir, ssw_last_error());
        return -1;
    }
    if (!h->continuous || h->cont_rec_sm != NULL) {
        fprintf(stderr, "%s: not a continuous model, or the table exists before it is asked for\n", dir);
        return -1;
    }
    for (int pass = 0; pass < 2; ++pass) { /* made, then rebuilt in place */
        const float *before = h->cont_rec_sm;
        if (ssw_host_build_cont_sm(h) < 0) {
            fprintf(stderr, "%s: %s\n", dir, ssw_last_error());
            return -1;
        }
        if (pass == 1 && h->cont_rec_sm != before) {
            fprintf(stderr, "%s: the rebuild moved the table\n", dir);
            return -1;
        }
        const float *mp = h->mean, *vp = h->var, *dp = h->det;
        const size_t nd = (size_t)h->n_density;
        size_t used = 0, nonzero = 0;
        if (h->cont_sm_floats != h->cont_sm_sen * (size_t)h->n_cb || h->cont_sm_sen % 2 != 0)
            return -1;
        for (int c = 0; c < h->n_cb; ++c)
            for (int f = 0; f < h->n_feat; ++f) {
                const size_t vl = (size_t)h->veclen[f];
                const size_t at = (size_t)c * h->cont_sm_sen + h->cont_sm_off[f];
                if (at % 2 != 0 || at + nd * (2 * vl + 1) > h->cont_sm_floats)
                    return -1;
                const float *r = h->cont_rec_sm + at;
                for (int d = 0; d < h->n_density; ++d) {
                    for (size_t j = 0; j < vl; ++j) {
                        if (bits_of(r[2 * (j * nd + (size_t)d)]) != bits_of(*mp++)
                            || bits_of(r[2 * (j * nd + (size_t)d) + 1]) != bits_of(*vp++)) {
                            fprintf(stderr, "%s: senone %d stream %d density %d dimension %zu\n", dir, c, f, d, j);
                            return -1;
                        }
                    }
                    if (bits_of(r[2 * vl * nd + (size_t)d]) != bits_of(*dp++)) {
                        fprintf(stderr, "%s: det of senone %d stream %d density %d\n", dir, c, f, d);
                        return -1;
                    }
                }
                used += nd * (2 * vl + 1);
            }
        for (size_t i = 0; i < h->cont_sm_floats; ++i)
            nonzero += h->cont_rec_sm[i] != 0.0f;
        if (nonzero > used) { /* (the padding is zeros) */
            fprintf(stderr, "%s: %zu floats set, %zu belong to records\n", dir, nonzero, used);
            return -1;
        }
    }
    printf("ok table %s: %d senones, %d streams, %d densities, %zu floats a senone\n", dir, h->n_sen,
           h->n_feat, h->n_density, h->cont_sm_sen);
    ssw_host_model_free(h);
    return 0;
}

template <int TOPN>
static long
select_topn(const float *v, int nd)
{
    float dist[TOPN], rdist[TOPN];
    int id[TOPN], rid[TOPN];
    for (int k = 0; k < TOPN; ++k) {
        dist[k] = rdist[k] = SSW_CONT_WORST_DIST;
        id[k] = rid[k] = 0;
    }
    for (int d = 0; d < nd; ++d)
        cont_insert<TOPN>(dist, id, v[d], d);
    int filled = 0;
    for (int d = 0; d < nd; ++d) {
        const int rank = cont_select_rank(v[d], d, nd, [&](int e) { return v[e]; });
        if (rank >= nd || rank < -1)
            return -1;
        if (rank >= 0 && rank < TOPN) {
            if (filled & (1 << rank))
                return -1; /* two densities in one slot */
            filled |= 1 << rank;
            rdist[rank] = v[d];
            rid[rank] = d;
        }
    }
    for (int k = 0; k < TOPN; ++k)
        if (bits_of(dist[k]) != bits_of(rdist[k]) || id[k] != rid[k]) {
            fprintf(stderr, "select: topn %d, %d densities:", TOPN, nd);
            for (int d = 0; d < nd; ++d)
                fprintf(stderr, " %g", v[d]);
            fprintf(stderr, ": slot %d is (%g, %d) by insertion, (%g, %d) by rank\n", k, dist[k], id[k],
                    rdist[k], rid[k]);
            return -1;
        }
    return 1;
}

static int
check_select()
{
    const float vals[5] = { SSW_CONT_WORST_DIST - 256.0f, SSW_CONT_WORST_DIST, 0.0f, 1.0f, NAN };
    long n = 0;
    if (!(vals[0] < vals[1]))
        return -1;
    for (int nd = 1; nd <= 5; ++nd) {
        int total = 1;
        for (int i = 0; i < nd; ++i)
            total *= 5;
        for (int code = 0; code < total; ++code) {
            float v[5];
            for (int i = 0, c = code; i < nd; ++i, c /= 5)
                v[i] = vals[c % 5];
            const long r[5] = { select_topn<1>(v, nd), select_topn<2>(v, nd), select_topn<3>(v, nd),
                                select_topn<4>(v, nd), select_topn<5>(v, nd) };
            for (int k = 0; k < 5; ++k) {
                if (r[k] < 0)
                    return -1;
                n += r[k];
            }
        }
    }
    printf("ok select: %ld cases\n", n);
    return 0;
}

/* the set of frame t restated: seed + every phone entered by t, then acmod_flags2list's bridges
 * (src/acmod.c:966-975) over the ascending list */
static std::vector<uint32_t>
row_restated(int n_sen, int t, int np, const uint16_t *senid, const std::vector<int32_t> &first,
             const uint32_t *seed)
{
    const int nw32 = (n_sen + 31) / 32;
    std::vector<uint32_t> row((size_t)nw32, 0u);
    for (int w = 0; seed != NULL && w < nw32; ++w)
        row[(size_t)w] = seed[w];
    if (n_sen % 32 != 0)
        row[(size_t)nw32 - 1] &= (1u << (n_sen % 32)) - 1u;
    for (int i = 0; i < np; ++i)
        if (first[(size_t)i] <= t)
            for (int j = 0; j < 3; ++j)
                row[senid[3 * i + j] >> 5] |= 1u << (senid[3 * i + j] & 31);
    std::vector<uint32_t> out = row;
    int last = 0;
    for (int s = 0; s < n_sen; ++s)
        if ((row[(size_t)s >> 5] >> (s & 31)) & 1u) {
            while (s - last > 255) {
                last += 255;
                out[(size_t)last >> 5] |= 1u << (last & 31);
            }
            last = s;
        }
    return out;
}

static int
check_rows()
{
    uint32_t lcg = 12345u;
    auto rnd = [&](int n) { lcg = lcg * 1664525u + 1013904223u; return (int)((lcg >> 8) % (uint32_t)n); };
    int n_cases = 0;
    long n_frames_checked = 0;
    const int shapes[4] = { 5, 70, 1000, 5126 };
    for (int n_sen : shapes)
        for (int rep = 0; rep < 6; ++rep) {
            const int nw32 = (n_sen + 31) / 32;
            const int np = 1 + rnd(rep == 0 ? 1 : 12), nf = rep == 1 ? 0 : 1 + rnd(60);
            std::vector<uint16_t> senid((size_t)np * 3);
            for (auto &s : senid)
                s = (uint16_t)rnd(n_sen);
            std::vector<int32_t> sf((size_t)np), ef((size_t)np);
            int a = 0, b = 0;
            for (int i = 0; i < np; ++i) { /* windows that do not decrease; some unbounded */
                a += rnd(8);
                b = std::max(b, a) + rnd(12);
                sf[(size_t)i] = rep == 2 ? 0 : a;
                ef[(size_t)i] = rep == 2 ? INT_MAX : b;
            }
            std::vector<uint32_t> seed((size_t)nw32, 0u);
            for (int k = 0; k < 4; ++k) {
                const int s = rnd(n_sen);
                seed[(size_t)s >> 5] |= 1u << (s & 31);
            }
            for (int with_seed = 0; with_seed < 2; ++with_seed) {
                std::vector<uint32_t> rows(3, 0xdeadbeefu); /* (appended to what is there) */
                std::vector<int32_t> rof((size_t)std::max(nf, 1), -1), first;
                const uint32_t *sd = with_seed ? seed.data() : NULL;
                if (cont_active_rows(n_sen, nf, np, senid.data(), sf.data(), ef.data(), sd, 7, rows,
                                     rof.data()) < 0) {
                    fprintf(stderr, "rows: refused: %s\n", ssw_last_error());
                    return -1;
                }
                if (active_first_frames(sf.data(), ef.data(), np, nf, first) < 0)
                    return -1;
                if ((rows.size() - 3) % (size_t)nw32 != 0 || rows[0] != 0xdeadbeefu)
                    return -1;
                const int n_rows = (int)((rows.size() - 3) / (size_t)nw32);
                for (int t = 0; t < nf; ++t) {
                    const int r = rof[(size_t)t] - 7;
                    if (r < 0 || r >= n_rows || (t > 0 && rof[(size_t)t] < rof[(size_t)t - 1])) {
                        fprintf(stderr, "rows: frame %d reads row %d of %d\n", t, r, n_rows);
                        return -1;
                    }
                    const std::vector<uint32_t> want = row_restated(n_sen, t, np, senid.data(), first, sd);
                    if (memcmp(want.data(), rows.data() + 3 + (size_t)r * nw32, 4 * (size_t)nw32) != 0) {
                        fprintf(stderr, "rows: %d senones, case %d, frame %d: the row differs\n", n_sen, rep, t);
                        return -1;
                    }
                    ++n_frames_checked;
                }
                if (nf > 0 && rof[(size_t)nf - 1] - 7 != n_rows - 1)
                    return -1; /* no row that no frame reads */
                ++n_cases;
            }
        }
    { /* the refusals */
        const uint16_t senid[6] = { 0, 1, 2, 3, 4, 70 };
        const int32_t sf[2] = { 0, 3 }, ef[2] = { 5, 9 }, sf_bad[2] = { 4, 3 };
        std::vector<uint32_t> rows;
        int32_t rof[10];
        if (cont_active_rows(70, 10, 2, senid, sf, ef, NULL, 0, rows, rof) >= 0
            || strstr(ssw_last_error(), "senone 70 of 70") == NULL)
            return -1;
        if (cont_active_rows(71, 10, 2, senid, sf_bad, ef, NULL, 0, rows, rof) >= 0
            || strstr(ssw_last_error(), "must not decrease") == NULL)
            return -1;
        if (cont_active_rows(71, 10, 0, senid, sf, ef, NULL, 0, rows, rof) >= 0)
            return -1;
    }
    printf("ok rows: %d utterances, %ld frames\n", n_cases, n_frames_checked);
    return 0;
}

int
main(int argc, char **argv)
{
    int a = 1;
    while (a < argc) {
        if (!strcmp(argv[a], "table") && a + 2 < argc) {
            if (check_table(argv[a + 1], atoi(argv[a + 2])) < 0) {
                fprintf(stderr, "table %s: FAILED\n", argv[a + 1]);
                return 1;
            }
            a += 3;
        } else if (!strcmp(argv[a], "select")) {
            if (check_select() < 0)
                return 1;
            a += 1;
        } else if (!strcmp(argv[a], "rows")) {
            if (check_rows() < 0) {
                fprintf(stderr, "rows: FAILED\n");
                return 1;
            }
            a += 1;
        } else {
            fprintf(stderr, "usage: cont_listed_host ( table DIR TOPN | select | rows )...\n");
            return 1;
        }
    }
    return 0;
}
