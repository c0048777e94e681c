/* ssw_fe_log.inc -- the natural logarithm of fe_mel_cep (src/fe_sigproc.c:609-622), correctly
 * rounded.  Part of the single translation unit ssw_kernels.hip (included there before
 * ssw_k8_fe.inc); plain C++ besides, so tests/harness/fe_log_host.cpp runs it on the CPU.
 *
 * The reference calls libm's log on a double.  A good libm's log is the correctly rounded value
 * for all but a few arguments in 100,000 (glibc states 0.52 ulp); the device library's is one
 * ulp away a few times in 1,000, and for audio so quiet that every mel value sits beside the
 * 1e-4 floor the DCT cancels the nearly equal logs until a float ulp no longer hides a double
 * one.  So the logarithm is computed here to about 100 bits in pairs of doubles and rounded once:
 *
 *   x = 2^e m, sqrt(1/2) <= m < sqrt(2);   s = (m - 1) / (m + 1), |s| < 0.1716
 *   log x = e ln 2 + 2 s (1 + s^2 / 3 + s^4 / 5 + ...)
 *
 * m - 1 is exact and m + 1 is an exact pair; the terms from s^16 / 17 on are below 6e-13 of the
 * sum and are summed in double (their error is below 1e-28 of the result), the first eight in
 * pairs; ln 2 is three doubles, e times the first an exact pair.  Every step is +, -, *, / or an
 * fma used only to get the exact error of a product.  Zero, negative, subnormal and non-finite
 * arguments go to the library's log: the front end's are at least 1e-4 unless a sample was not
 * finite. */
#if defined(__HIPCC__)
#define SSW_FE_HD __host__ __device__ __forceinline__
#else
#define SSW_FE_HD static inline
#endif

struct FeDD {
    double hi, lo; /* hi + lo, |lo| <= ulp(hi) / 2 */
};

SSW_FE_HD FeDD
fe_dd_fast_sum(double a, double b) /* |a| >= |b| */
{
    const double s = a + b;
    return FeDD{ s, b - (s - a) };
}

SSW_FE_HD FeDD
fe_dd_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return FeDD{ s, (a - (s - bb)) + (b - bb) };
}

SSW_FE_HD FeDD
fe_dd_prod(double a, double b)
{
    const double p = a * b;
    return FeDD{ p, __builtin_fma(a, b, -p) };
}

SSW_FE_HD FeDD
fe_dd_add(FeDD a, FeDD b)
{
    FeDD s = fe_dd_sum(a.hi, b.hi);
    const FeDD t = fe_dd_sum(a.lo, b.lo);
    s = fe_dd_fast_sum(s.hi, s.lo + t.hi);
    return fe_dd_fast_sum(s.hi, s.lo + t.lo);
}

SSW_FE_HD FeDD
fe_dd_mul(FeDD a, FeDD b)
{
    const FeDD p = fe_dd_prod(a.hi, b.hi);
    return fe_dd_fast_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}

/* a / b for a double a */
SSW_FE_HD FeDD
fe_dd_div(double a, FeDD b)
{
    const double q1 = a / b.hi;
    const FeDD p = fe_dd_prod(q1, b.hi);
    const double r = ((a - p.hi) - p.lo) - q1 * b.lo; /* a - p.hi is exact: q1 b.hi is within an ulp of a */
    return fe_dd_fast_sum(q1, r / b.hi);
}

SSW_FE_HD double
fe_log(double x)
{
    /* ln 2 = L1 + L2 + L3 to 159 bits */
    const double L1 = 0x1.62e42fefa39efp-1, L2 = 0x1.abc9e3b39803fp-56, L3 = 0x1.7b57a079a1934p-111;
    if (!(x >= 0x1p-1022 && x <= 0x1.fffffffffffffp+1023))
        return log(x);
    /* x = 2^e m with m in [1, 2), then m in [sqrt(1/2), sqrt(2)): by factors of two, exactly */
    int e = 0;
    double m = x;
    while (m >= 0x1p+64) {
        m *= 0x1p-64;
        e += 64;
    }
    while (m < 0x1p-64) {
        m *= 0x1p+64;
        e -= 64;
    }
    while (m >= 0x1.6a09e667f3bcdp+0) {
        m *= 0.5;
        e += 1;
    }
    while (m < 0x1.6a09e667f3bcdp-1) {
        m *= 2.0;
        e -= 1;
    }
    const FeDD s = fe_dd_div(m - 1.0, fe_dd_sum(m, 1.0));
    const FeDD s2 = fe_dd_mul(s, s);
    /* the tail 1/17 + s^2 / 19 + ... + s^28 / 45 (the next term is below 2e-24 of it) in double */
    double t = 1.0 / 45.0;
    for (int k = 21; k >= 8; --k)
        t = t * s2.hi + 1.0 / (double)(2 * k + 1);
    /* P = 1 + s^2 / 3 + ... + s^14 / 15 + s^16 t in pairs, 1 / (2k + 1) as a pair */
    FeDD P = fe_dd_mul(s2, FeDD{ t, 0.0 });
    for (int k = 7; k >= 0; --k) {
        const double d = (double)(2 * k + 1), c = 1.0 / d;
        const FeDD ck = fe_dd_fast_sum(c, __builtin_fma(-c, d, 1.0) / d);
        P = fe_dd_add(P, ck);
        if (k > 0)
            P = fe_dd_mul(P, s2);
    }
    FeDD lm = fe_dd_mul(s, P);
    lm.hi *= 2.0;
    lm.lo *= 2.0;
    const double ed = (double)e;
    FeDD el = fe_dd_add(fe_dd_prod(ed, L1), fe_dd_prod(ed, L2));
    el = fe_dd_fast_sum(el.hi, el.lo + ed * L3);
    return fe_dd_add(el, lm).hi;
}
