// sz_kldgain.h — the scalar arithmetic of KLD-gain early stopping (sz_set_kld_stop; include/sigmazero.h is the rule): one root child's term of
// the Kullback-Leibler divergence of the root's visit distribution at the last snapshot from the one now.  Every operator is one IEEE f64
// rounding (-ffp-contract=off), the logarithm is sz_gumbel.h's sz_slog, and tests/kldref.py repeats the function operator for operator.
// Plain C++: the same text compiles for the host and for the device.
#pragma once
#include "sz_gumbel.h"

// term_c = o * ln(o / n), o = prev_c / prev_total, n = now_c / new_total.  A child without a visit at the snapshot has no term: 0.0.  Visits
// never fall within a search, so now_c >= prev_c > 0 where a term is formed: o / n is a positive normal f64 and sz_slog's precondition holds.
// now_c == prev_c and new_total == prev_total give o == n, o / n == 1.0 and sz_slog(1.0) == 0.0: the term is exactly 0.
SZG_FN double sz_kld_term(int prev_c, int prev_total, int now_c, int new_total) {
    if (prev_c == 0) return 0.0;
    const double o = (double)prev_c / (double)prev_total;
    const double n = (double)now_c / (double)new_total;
    return o * sz_slog(o / n);
}

// the same term on two probabilities formed by the caller (the search summary's policy surprise, sz_summary.h): o * ln(o / n).  o / n must be
// a positive normal f64; the caller sees to it.
SZG_FN double sz_kld_term(double o, double n) { return o * sz_slog(o / n); }
