// sz_lcb.h — the scalar arithmetic of the per-edge value spread and of lower-confidence-bound move selection (sz_set_lcb; include/sigmazero.h is
// the rule): a square root written from + - * / and integer bit operations only, the mean, spread, radius and bound of one root child, and the
// candidate test.  The device maths library's sqrt is not relied on to round like libm's, so the rule carries its own; every operator here is
// one IEEE f64 rounding (-ffp-contract=off) and tests/lcbref.py repeats each function operator for operator.  Plain C++: the same text compiles
// for the host and for the device.
//
// The second moment.  Beside W (the sum of the values backed up through an edge) the tree keeps Q, the sum of their squares, in f64, one per
// edge, zeroed where the edge is created and added to wherever W is added to, in the same order: Q = Q + sv * sv for a value sv = +-v, v the
// (double) of the network's f32 value or a terminal / proven -1, 0, +1.  The product of two such doubles is exact (24 x 24 significant bits),
// the sum takes one rounding.  A budget counted out at once (a terminal root) adds (tv * tv) * (double)k for its k simulations.
//
// One child c of the root, with the tree's counted visits N_c >= 2, value sum W_c and square sum Q_c (W and Q are stored from the child's side
// to move; the sign turns the mean to the mover's, wave_ending's convention):
//     m_c   = -(W_c / (double)N_c)
//     s_c   = Q_c / (double)N_c - m_c * m_c;   if (!(s_c > 0.0)) s_c = 0.0          the biased variance, clamped (a NaN is clamped too)
//     r_c   = z * ssqrt(s_c / (double)(N_c - 1))                                     z standard errors of the mean, unbiased variance
//     lcb_c = m_c - r_c
// With N_c < 2 the child has no bound (NaN) and is no candidate.  Child c is a candidate iff N_c >= 2 && n_c >= 1 && (double)n_c >= p *
// (double)n_c*, n the counts the move choice reads (pruned on a forced board) and c* their first maximum.
#pragma once
#include "sz_gumbel.h"

SZG_FN double sz_lcb_nan() { return szg_f64(0x7ff8000000000000ULL); }

// ssqrt(x), x = 0.0 or a positive normal f64.  x = 2^e * m with m in [1, 2) by bit operations; an odd e gives one factor 2 to m, so e is
// even and m lies in [1, 4).  y = 0.5 * (1.0 + m) is above sqrt(m) by at most 0.5 (at m = 4: 2.5 against 2), and six Heron steps
// y = 0.5 * (y + m / y) square the relative error each time (0.25, 0.025, 3.0e-4, 4.6e-8, 1.1e-15, below 2^-53): the sixth leaves the rounding
// of its own three operators.  The result is y * 2^(e/2), the power of two built by bits: the product is exact.  ssqrt(0.0) = 0.0 (-0.0 too).
// Anything else (negative, subnormal, infinite, NaN) is treated as 0.0 and counted in *bad.
SZG_FN double sz_ssqrt(double x, int* bad) {
    if (x == 0.0) return 0.0;
    const uint64_t u = szg_bits(x);
    const int be = (int)((u >> 52) & 0x7ff);
    if ((u >> 63) != 0 || be == 0 || be == 0x7ff) { *bad = *bad + 1; return 0.0; }
    int e = be - 1023;
    uint64_t mb = (u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;             // [1, 2)
    if (e & 1) { mb = mb + 0x0010000000000000ULL; e = e - 1; }                      // [2, 4); two's complement: -3 & 1 == 1, -3 - 1 == -4
    const double m = szg_f64(mb);
    double y = 0.5 * (1.0 + m);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    return y * szg_f64((uint64_t)(int64_t)(e / 2 + 1023) << 52);                    // e is even: e / 2 is exact; 2^-511 .. 2^511
}

// m_c: the mover's mean value of the child's visits
SZG_FN double sz_lcb_mean(double w, int n) { return -(w / (double)n); }

// s_c: the biased variance of the values backed up through the child, never negative
SZG_FN double sz_lcb_spread(double q, int n, double m) {
    double s = q / (double)n - m * m;
    if (!(s > 0.0)) s = 0.0;
    return s;
}

// r_c: z standard errors of the mean
SZG_FN double sz_lcb_radius(double z, double s, int n, int* bad) { return z * sz_ssqrt(s / (double)(n - 1), bad); }

// lcb_c of a child with the tree's N, W, Q; NaN with N < 2
SZG_FN double sz_lcb_value(int n, double w, double q, double z, int* bad) {
    if (n < 2) return sz_lcb_nan();
    const double m = sz_lcb_mean(w, n);
    return m - sz_lcb_radius(z, sz_lcb_spread(q, n, m), n, bad);
}

// the candidate test: N_c the tree's count, n_c the count the move choice reads, n_star = n_c*
SZG_FN bool sz_lcb_candidate(int N_c, int n_c, int n_star, double p) { return N_c >= 2 && n_c >= 1 && (double)n_c >= p * (double)n_star; }

// the move on one thread, for the host: the first maximum of lcb over the candidates as the kernels find it (lane l keeps the first strict
// maximum among c = l, l + 64, ...; then the xor butterfly with offsets 32..1 keeps the larger value, the lower index on a tie), c* (the first
// maximum of n_c) without a candidate.  lcb_out[0..K) receives every child's bound.  Returns the move; *cstar, *ncand, *bad as the kernel's.
static inline int sz_lcb_move_host(const int* n, const int* N, const double* W, const double* Q, int K, double z, double p, double* lcb_out, int* cstar,
                                   int* ncand, int* bad) {
    int cs = 0;
    for (int c = 1; c < K; c++) if (n[c] > n[cs]) cs = c;
    double best[64]; int bi[64];
    int cand = 0;
    *bad = 0;
    for (int l = 0; l < 64; l++) { best[l] = 0.0; bi[l] = 0x7fffffff; }
    for (int c = 0; c < K; c++) {
        const double v = sz_lcb_value(N[c], W[c], Q[c], z, bad);
        lcb_out[c] = v;
        if (!sz_lcb_candidate(N[c], n[c], n[cs], p)) continue;
        cand++;
        const int l = c & 63;
        if (bi[l] == 0x7fffffff || v > best[l]) { best[l] = v; bi[l] = c; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        double nb[64]; int ni[64];
        for (int l = 0; l < 64; l++) {
            const double ob = best[l ^ off]; const int oi = bi[l ^ off];
            nb[l] = best[l]; ni[l] = bi[l];
            if (oi != 0x7fffffff && (bi[l] == 0x7fffffff || ob > best[l] || (ob == best[l] && oi < bi[l]))) { nb[l] = ob; ni[l] = oi; }
        }
        for (int l = 0; l < 64; l++) { best[l] = nb[l]; bi[l] = ni[l]; }
    }
    *cstar = cs; *ncand = cand;
    return bi[0] == 0x7fffffff ? cs : bi[0];
}
