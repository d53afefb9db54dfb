// sz_cpuct.h — the scalar arithmetic of the visit-dependent exploration rate (sz_set_cpuct; include/sigmazero.h is the rule): the f32 that takes
// c_puct's place in ucb_value / ucb_u at a parent with n_p visits.  Every operator is one IEEE f64 rounding (-ffp-contract=off), the logarithm is
// sz_gumbel.h's sz_slog, and tests/puctref.py repeats the function operator for operator.  Plain C++: the same text compiles for the host and
// for the device.
#pragma once
#include "sz_gumbel.h"

// c(n_p) = init + factor * ln((n_p + base + 1) / base).  base >= 1 and n_p >= 0, so x > 1 and sz_slog's precondition holds.  factor == 0 gives
// init exactly: sz_slog(x) is finite, 0.0 * finite = +-0.0, and init + +-0.0 is init (+0.0 for init = +0.0).
SZG_FN float sz_cpuct(float init, float base, float factor, int n_p) {
    const double x = (((double)n_p + (double)base) + 1.0) / (double)base;
    return (float)((double)init + (double)factor * sz_slog(x));
}
