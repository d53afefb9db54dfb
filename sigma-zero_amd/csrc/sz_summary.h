// sz_summary.h — the scalar arithmetic of the search summary (sz_set_search_summary; include/sigmazero.h is the rule): what a finished search
// hands to the trainer beside the visit counts.  root_q and best_q, the search's own value of the root from the mover's side, and the policy
// surprise KL(target || prior) of the ply's record against the priors the search used.  Every operator is one IEEE f64 rounding
// (-ffp-contract=off), the logarithm is sz_gumbel.h's sz_slog, the term is sz_kldgain.h's sz_kld_term, and tests/summaryref.py repeats each
// function operator for operator.  Plain C++: the same text compiles for the host and for the device.
//
// Two kernels (csrc/sz_engine.hip) call these around k_play, one wavefront per board: k_summary_pre while the tree is intact (k_play compacts
// the store in place under reuse_subtree, and the next search overwrites it otherwise), k_summary_post when the ply's record exists (the pruned
// counts of a forced-playouts board exist nowhere else).
//
// Child order: k_play writes rec_action[c] / rec_visits[c] for c = 0..n in one loop over the root's children es[first + c] / em[first + c]
// ("for (int c = lane; c < SZ_MAX_CHILDREN; c += 64)" at the head of k_play), and policy-target pruning rewrites rec_visits[c] at the same c.
// The record's child order is therefore the tree root's child order, and k_summary_pre's prior copy P[c] = es[first + c].P lines up with
// k_summary_post's n_c = rec_visits[c] without a look-up by action.
//
// sz_slog's precondition (a positive normal f64) against t_c / P_c: a term is formed only for n_c > 0, so 2^-31 < t_c <= 1.  Expansion drops
// moves whose renormalised prior is 0, so a stored P_c is a positive f32; as an f64 every positive f32, subnormal ones included, is a normal
// number of at least 2^-149, and root noise leaves a prior finite.  t_c / P_c then lies in (2^-160, 2^149]: normal.  The rule still states what
// a prior outside that does, so that no input reaches sz_slog unchecked: a P_c that is not a normal positive finite f32 (zero, negative,
// subnormal, infinite, NaN) gives the term 0.0, and the term is counted (sz_search_summary_stats' second counter).
#pragma once
#include "sz_kldgain.h"

#define SZS_F32_MIN_NORMAL 1.17549435e-38f      /* 2^-126 */
#define SZS_F32_MAX 3.40282347e+38f

SZG_FN double sz_summary_nan() { return szg_f64(0x7ff8000000000000ULL); }

// child c's term of wsum(N_c >= 1 ? W_c : 0.0): an unvisited child's W is 0.0 in the tree already; the rule does not depend on it
SZG_FN double sz_summary_value_term(int n_c, double w_c) { return n_c >= 1 ? w_c : 0.0; }

// root_q = -(wsum / (double)total): W is stored from the child's side to move, the sign turns it to the mover's
SZG_FN double sz_summary_root_q(double wsum, int total) { return -(wsum / (double)total); }

// best_q = -(W_c* / (double)N_c*), c* the first maximum of N_c: wave_ending's m, operator for operator
SZG_FN double sz_summary_best_q(double w, int n) { return -(w / (double)n); }

// a stored prior a term may be formed on; a NaN fails the first comparison
SZG_FN bool sz_summary_prior_ok(float p) { return p >= SZS_F32_MIN_NORMAL && p <= SZS_F32_MAX; }

// child c's term of the surprise: t_c * slog(t_c / P_c), t_c = n_c / rtotal, for a child the record gives a visit; 0.0 otherwise.
// *dropped counts the terms the precondition rule above left out.
SZG_FN double sz_summary_term(int n_c, int rtotal, float p, int* dropped) {
    if (n_c <= 0) return 0.0;
    if (!sz_summary_prior_ok(p)) { *dropped = *dropped + 1; return 0.0; }
    const double t = (double)n_c / (double)rtotal;
    return sz_kld_term(t, (double)p);
}

// wsum on one thread, for the host: lane l adds the terms c = l, l + 64, l + 128, l + 192 ascending from 0.0, then the xor butterfly with
// offsets 32..1 (v_l = v_l + v_(l xor off)), lane 0's value.  The kernels do the same with one lane per l (wave_sum_f64).
template <typename TermF>
static inline double sz_summary_wsum_host(TermF term, int K) {
    double v[64], w[64];
    for (int l = 0; l < 64; l++) {
        double acc = 0.0;
        for (int c = l; c < K; c += 64) acc = acc + term(c);
        v[l] = acc;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; l++) w[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 64; l++) v[l] = w[l];
    }
    return v[0];
}
