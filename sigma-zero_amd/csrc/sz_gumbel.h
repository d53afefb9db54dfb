// sz_gumbel.h — the scalar arithmetic of the Gumbel root search (sz_set_gumbel; include/sigmazero.h is the rule): a logarithm and an exponential
// written from + - * / and integer bit operations only, and the sequential-halving level of a root-child visit.  libm's and the device maths
// library's log / exp do not round alike, so the rule carries its own; every operator here is one IEEE f64 rounding (-ffp-contract=off) and
// tests/gumbelref.py repeats each function operator for operator.  Plain C++: the same text compiles for the host and for the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SZG_FN __host__ __device__ __forceinline__
#else
#define SZG_FN static inline
#endif

#define SZG_SQRT2 1.4142135623730951            /* the f64 nearest sqrt(2) */
#define SZG_LN2 0.6931471805599453              /* the f64 nearest ln 2, 0x3FE62E42FEFA39EF */
#define SZG_INV_LN2 1.4426950408889634          /* the f64 nearest 1 / ln 2 */
#define SZG_LN2_HI 6.93147180369123816490e-01   /* 0x3FE62E42FEE00000: ln 2 with its low 21 bits clear, k * LN2_HI is exact for |k| < 2^21 */
#define SZG_LN2_LO 1.90821492927058770002e-10   /* 0x3DEA39EF35793C76: ln 2 - LN2_HI */
#define SZG_EXP_CUTOFF (-700.0)                 /* sexp(y) = 0 below: the results above stay normal numbers (2^-1010 at the least) */

SZG_FN uint64_t szg_bits(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
SZG_FN double szg_f64(uint64_t u) { double x; __builtin_memcpy(&x, &u, 8); return x; }

// slog(x), x > 0 a normal f64 (every (double) of a positive f32 is one): x = 2^e * m with m in [sqrt(1/2), sqrt(2)) by bit operations,
// s = (m - 1) / (m + 1), |s| <= 0.1716, ln m = 2s * (1 + s^2/3 + s^4/5 + ... + s^18/19) by Horner in s^2 (ten terms: the first one left out,
// s^20 / 21, is below 2.3e-17 < 2^-53), then + e * LN2.
SZG_FN double sz_slog(double x) {
    const uint64_t u = szg_bits(x);
    int e = (int)((u >> 52) & 0x7ff) - 1023;
    double m = szg_f64((u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL);      // [1, 2)
    if (m >= SZG_SQRT2) { m = m * 0.5; e = e + 1; }
    const double s = (m - 1.0) / (m + 1.0);
    const double s2 = s * s;
    double p = 1.0 / 19.0;
    p = p * s2 + 1.0 / 17.0;
    p = p * s2 + 1.0 / 15.0;
    p = p * s2 + 1.0 / 13.0;
    p = p * s2 + 1.0 / 11.0;
    p = p * s2 + 1.0 / 9.0;
    p = p * s2 + 1.0 / 7.0;
    p = p * s2 + 1.0 / 5.0;
    p = p * s2 + 1.0 / 3.0;
    p = p * s2 + 1.0;
    return (2.0 * s) * p + (double)e * SZG_LN2;
}

// sexp(y), y <= 0: 0 below SZG_EXP_CUTOFF (and for a NaN); k = floor(y * (1 / ln 2) + 0.5), r = (y - k * LN2_HI) - k * LN2_LO, |r| <= 0.3466,
// e^r = sum of r^j / j! for j = 0..13 by Horner (the first term left out, r^14 / 14!, is below 4.2e-18 < 2^-53), scaled by 2^k through the
// exponent bits.
SZG_FN double sz_sexp(double y) {
    if (!(y >= SZG_EXP_CUTOFF)) return 0.0;
    const double k = __builtin_floor(y * SZG_INV_LN2 + 0.5);
    const double r = (y - k * SZG_LN2_HI) - k * SZG_LN2_LO;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 1.0 / 2.0;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return szg_f64(szg_bits(p) + ((uint64_t)(int64_t)k << 52));
}

// The sequential-halving level of root-child visit t (0-based) of n, m_eff children considered: the rounds completed before the round t
// falls in.  L = max(1, ceil(log2 m_eff)); a phase with c considered children has r = max(1, n / (L * c)) rounds of c visits, then
// c <- max(2, c / 2); the first phase has c = m_eff.  The walk ends in the phase t falls in: at most about 8 + 2L iterations for t < n.
SZG_FN int sz_gumbel_level(int t, int n, int m_eff) {
    if (m_eff < 1) m_eff = 1;
    int L = 0;
    while ((1 << L) < m_eff) L++;
    if (L < 1) L = 1;
    int c = m_eff, t0 = 0, level = 0;
    for (;;) {
        int r = n / (L * c);
        if (r < 1) r = 1;
        const int span = r * c;
        if (t < t0 + span) return level + (t - t0) / c;
        t0 += span; level += r;
        c = c / 2;
        if (c < 2) c = 2;
    }
}
