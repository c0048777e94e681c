/* ssw_cont_select.inc -- compute_dist's top-N selection (src/ms_gauden.c:397-429) for the
 * continuous-density kernels (K11), in two forms: the sequential insertion cont_score_kernel runs
 * in a lane's registers, and the RANK of a density among its codebook's, which cont_listed_kernel
 * computes across the lanes of a group with no insertion at all.
 * Part of the single translation unit ssw_kernels.hip (included there before ssw_k11_cont.inc);
 * tests/harness/cont_listed_host.cpp compiles the same text for the host (SSW_CONT_SEL_FN) and
 * holds the two forms against each other exhaustively. */

#define SSW_CONT_WORST_DIST (-2147483648.0f) /* WORST_DIST, src/ms_gauden.c */

/* compute_dist's insertion (src/ms_gauden.c:418-428) into a list kept best first: the density is
 * taken when v >= the worst entry, and stands before the first entry with v >= entry -- new before
 * equal.  One pass of compare-and-swap: from that entry on, the value carried is the entry
 * displaced, which is >= every entry behind it. */
template <int TOPN>
SSW_CONT_SEL_FN void
cont_insert(float (&dist)[TOPN], int (&id)[TOPN], float v, int d)
{
#pragma unroll
    for (int k = 0; k < TOPN; ++k) {
        const bool take = v >= dist[k]; /* (false for a NaN) */
        const float ov = dist[k];
        const int od = id[k];
        dist[k] = take ? v : ov;
        id[k] = take ? d : od;
        v = take ? ov : v;
        d = take ? od : d;
    }
}

/* The same list without the sequence.  The list starts as topn entries (WORST_DIST, density 0)
 * and the densities arrive in index order.
 *   - A density with !(v >= WORST_DIST) -- below it, or a NaN -- is never taken: every entry of
 *     the list is >= WORST_DIST at all times.  Call the others ELIGIBLE.
 *   - The list is always sorted by value, descending, and an arrival stands before the first
 *     entry it is >= to: before every entry of its own value.  Entries of equal value are
 *     therefore in DESCENDING index order, and the start-up entries, which came first of all,
 *     stand behind every eligible density of value WORST_DIST.
 *   - An entry leaves only off the end, pushed by an arrival that stands before it.
 * So after the last density the list holds the first topn of the eligible densities in the order
 * (value descending, index descending) -- an entry that is among them is never the one pushed
 * off, since fewer than topn stand before it at any time -- and start-up entries behind them.
 * A density's slot is its RANK: the count of eligible densities that precede it in that order;
 * it is in the list when the rank is below topn.  -0.0f and 0.0f compare equal here as there.
 *
 * value_of(e): the distance of density e, 0 <= e < n_density (a lane shuffle in the kernel, an
 * array read on the host).  Returns the rank of density d of value v, or -1 when it is not
 * eligible.  No index depends on a value. */
template <class ValueOf>
SSW_CONT_SEL_FN int
cont_select_rank(float v, int d, int n_density, ValueOf value_of)
{
    int rank = 0;
    for (int e = 0; e < n_density; ++e) {
        const float ve = value_of(e);
        const bool elig = ve >= SSW_CONT_WORST_DIST;
        const bool before = ve > v || (ve == v && e > d);
        rank += (elig && before) ? 1 : 0;
    }
    return v >= SSW_CONT_WORST_DIST ? rank : -1;
}
