// sz_engine.hip — batched MCTS self-play engine for MI355X (gfx950), hand-written HIP.
//
// Replaces, for thousands of concurrent boards, the per-game Python tree of the reference:
//   MCTS0.search            /root/reference/mcts.py:39-122
//   Node.select/get_ucb     /root/reference/mctsnode.py:23-37
//   Node.expand             /root/reference/mctsnode.py:39-54
//   Node.backpropagate      /root/reference/mctsnode.py:56-63
//   ChessTensor.move_piece / get_representation / get_value_and_terminated
//                           /root/reference/chess_tensor.py:88-172
//   actionsToTensor / tensorToAction (legal-move mask, child order)  chess_tensor.py:190-410
//   play_game's sampling + bookkeeping                               /root/reference/sim.py:46-97
//
// Execution model: ONE WAVEFRONT (64 lanes) OWNS ONE BOARD.
//   * tree = flat SoA in HBM per board: EdgeStat{W f64, N i32, P f32} (16 B, one dwordx4 per child,
//     a node's children are contiguous => coalesced span reads), EdgeMeta (16 B, read only for the
//     selected child), position records (80 B) for visited nodes only;
//   * select: lanes = children, UCB in the reference's exact fp32 op order, wave64 butterfly argmax
//     with lowest-index tie-break (torch.argmax semantics);
//   * move generation: lanes = squares (sz_chess.h), 73 ballots produce the legal-move mask directly
//     in action-index order, so children come out sorted with prefix popcounts (no sort);
//   * expand: masked renormalise with a fixed summation order (lane-strided partials + xor butterfly),
//     bit-identical to oracle/oc_mcts.c; backprop: the descent path sits in LDS, one lane per level,
//     no atomics (one leaf per board per step) => bitwise deterministic;
//   * encode: history bitboards staged in LDS; NCHW f32/bf16 (one 8-cell row per lane per store), NHWC bf16, or the
//     bit-packed NHWC image of 1 KiB per board (one 16-byte store per lane) that the MFMA stem expands itself.
// No MFMA here by design: this is latency/HBM-bound integer work; the network is the MFMA consumer.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <limits>
#include <tuple>
#include <type_traits>
#include <vector>
#include "sz_chess.h"
#include "sz_gumbel.h"
#include "sz_cpuct.h"
#include "sz_kldgain.h"
#include "sz_summary.h"
#include "sz_lcb.h"
#include "../../include/sigmazero.h"

// ------------------------------------------------------------------------------------------------
// device data
// ------------------------------------------------------------------------------------------------
struct alignas(16) EdgeStat { double W; int N; float P; };
struct alignas(16) EdgeMeta { int first; int node; unsigned short n; unsigned short action; signed char term; signed char tval; unsigned short pad; };

// NON-REFERENCE option (sz_set_solver): EdgeMeta.pad holds the proven result R of the edge's node for the side to move there (bits 0-1, the
// codes of sz_root_proven) and `complete` (bit 2: expansion kept every legal move as a child).  Zero when the option is off.
enum { PR_UNKNOWN = 0, PR_WIN = 1, PR_DRAW = 2, PR_LOSS = 3, PR_MASK = 3, PR_COMPLETE = 4 };

enum { ST_ACTIVE = 1, ST_PENDING = 2, ST_DONE = 4, ST_GAMEOVER = 8, ST_ERROR = 16, ST_SEARCHING = 32,
       ST_QUIET = 64,           // this search's root gets no root noise (sz_set_search_root_noise's quiet[b]); set by k_search_begin, gone after k_play
       ST_FORCED = 128 };       // this search's root forces playouts and its record is pruned (sz_set_forced_playouts' boards[b]); set by k_search_begin, gone after k_play

struct alignas(16) Ctl {
    int status, n_nodes, n_edges, sims_done;
    int pend_node, pend_depth, game_ply, err;
    unsigned long long n_expand, n_term, sum_depth, sum_k;
    int max_edges, game_result, reuse_ready, n_pend;    // reuse_ready: the store holds the subtree of the move just played (sz_config.reuse_subtree)
};                                                      // n_pend: leaves waiting for the network (sz_set_leaf_batching only)

struct View {
    int B, S, n_cap, e_cap, p_cap, learning, chess960, planes_dtype;
    float c_puct, noise;
    unsigned long long* dbg;    // diagnostic (sz_debug_step_stamps): 8 u64 per board, s_memtime at the phase boundaries of k_search_step; NULL = off
    int reuse;                  // NON-REFERENCE option (sz_config.reuse_subtree): keep the chosen child's subtree as the next search's tree
    int* nmap;                  // reuse only: [B][n_cap] scratch map node id -> new index of the edge that owns it, during k_play's compaction
    const int* slot;            // optional (sz_compact): row of board b in the network batch (planes / policy / value); NULL = identity
    const float* root_gamma;    // optional (non-reference) true Dirichlet root noise: [B][SZ_MAX_MOVES] Gamma(alpha,1) draws; NULL = reference behaviour
    const int* budget;          // optional (non-reference, sz_set_search_budgets): simulations of board b in 0..S; NULL = S everywhere (S stays the capacity)
    unsigned long long* sstat;  // solver only (sz_set_solver): [B][2] simulations ended on a proven non-terminal node, nodes proven by the update rule
    SzPos* npos; SzPos* ring; EdgeStat* es; EdgeMeta* em; int* gpath; u64* pmask; Ctl* ctl;
    // per-ply training record
    uint8_t* rec_planes; int* rec_action; int* rec_visits; int* rec_nchild; uint8_t* rec_colour; int* rec_chosen;
    uint8_t* rec_over; int8_t* rec_result; uint8_t* rec_active;
};

#define PMASK_STRIDE 80     // u64 words per board (73 used)

// NON-REFERENCE option (sz_set_leaf_batching): up to L leaves per board per step, steered apart by a virtual loss `lam` per descent in
// flight.  The in-flight count k of an edge is kept apart from W / N (W + lam - lam is not exact in f64).  Allocated on first use only.
struct Batch {
    int L; float lam;
    int* vk;        // [B][e_cap] descents in flight through each edge; zeroed as edges are created (the root edge at search begin)
    int* path;      // [B][L][p_cap] descent path of pending leaf i (path[0] = root edge)
    u64* mask;      // [B][L][PMASK_STRIDE] its legal-move mask
    int* depth;     // [B][L] its depth
};
#define LDS_HIST_WORDS 64   // 8 history slots x 8 words
#define LDS_MASK_WORDS 80

// ------------------------------------------------------------------------------------------------
// wave helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ u64 uni64(u64 x) {
    u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)x), hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(x >> 32));
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ double uni_f64(double x) { return __longlong_as_double((long long)uni64((u64)__double_as_longlong(x))); }
__device__ __forceinline__ SzPos load_pos(const SzPos* ptr) {
    SzPos p = *ptr;
    for (int k = 0; k < 6; k++) p.pc[k] = uni64(p.pc[k]);
    p.white = uni64(p.white); p.meta = uni64(p.meta); p.key = uni64(p.key); p.castling = uni64(p.castling);
    return p;
}
__device__ __forceinline__ float wave_sum_butterfly(float v) {
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ size_t planes_board_bytes(int dtype) {
    return dtype == SZ_PLANES_F32 ? (size_t)SZ_NUM_PLANES * 64 * 4 : (dtype == SZ_PLANES_BF16 ? (size_t)SZ_NUM_PLANES * 64 * 2 :
           (dtype == SZ_PLANES_NHWC128_BITS ? (size_t)1024 : (size_t)64 * 128 * 2));
}
// lane-indexed ballot (bit v = view square v) -> real-square bitboard
__device__ __forceinline__ u64 view_to_squares(u64 m, int white) {
    return white ? __builtin_bswap64(m) : __builtin_bswap64(sz_brev(m));
}

// ------------------------------------------------------------------------------------------------
// Node.get_ucb (mctsnode.py:33-37) in torch's float32 operation order; see oracle/oc_mcts.c:oc_ucb.
// Compiled with -ffp-contract=off: each operator is one IEEE rounding.
// ------------------------------------------------------------------------------------------------
// its two terms, each on its own for sz_set_forced_playouts' pruning, which holds q fixed while it lowers the visit count under u
__device__ __forceinline__ float ucb_q(int vc, double wsum) {
    float vsum = (float)wsum;
    float t1 = (float)vc + 1e-6f;
    return 1.0f - ((vsum / t1) + 1.0f) / 2.0f;
}
__device__ __forceinline__ float ucb_u(int vc, float prior, float sqrt_parent, float c) {
    float r = 1.0f / (float)(vc + 1);
    return ((r * sqrt_parent) * c) * prior;
}
__device__ __forceinline__ float ucb_value(int vc, double wsum, float prior, float sqrt_parent, float c) {
    float q = ucb_q(vc, wsum);
    float u = ucb_u(vc, prior, sqrt_parent, c);
    return q + u;
}

// The NON-REFERENCE options reach a kernel as a pack FO... of option structs (ForcedOpts, FpuOpts, GumbelOpts, EndOpts below), each one more, last
// argument: an option's instantiation is the one that takes its struct, k_search_step<VL, SOLVE, ForcedOpts> against k_search_step<VL, SOLVE>,
// whose argument list, and with it every line of its code, is what it was before the option existed.  has_opt: T is in the pack; opt_of: its member.
template <typename T, typename... FO> constexpr bool has_opt = (std::is_same_v<FO, T> || ...);
template <typename T, typename F, typename... R>
__device__ __forceinline__ const T& opt_of(const F& f, const R&... r) {
    if constexpr (std::is_same_v<T, F>) return f; else return opt_of<T>(r...);
}

// SOLVE (sz_set_solver): selection runs over the children that are not proven WIN (a child whose side to move wins is a refuted move); over all
// of them when every child is WIN.  wave_skip_wins: some child is not WIN, so the WIN children are skipped (uniform; false without SOLVE).
template <bool SOLVE>
__device__ __forceinline__ bool wave_skip_wins(const EdgeMeta* cm, int n) {
    bool skip_wins = false;
    if constexpr (SOLVE) {
        bool open = false;
        for (int c = lane_id(); c < n; c += 64) open |= (cm[c].pad & PR_MASK) != PR_WIN;
        skip_wins = __ballot(open) != 0;
    }
    return skip_wins;
}

// Node.select (mctsnode.py:23-31): argmax of get_ucb over the n contiguous children, first maximum wins (torch.argmax).
// Lanes = children; wave64 xor-butterfly with lowest-index tie-break.  ucb_out (optional, test hook) receives every child's value.
// VL (sz_set_leaf_batching): child c scores as if its k[c] descents in flight had each returned a loss for the parent, vc = N + k,
// wsum = W + lam*k (f64); parentVC = N + k of the parent (N alone without VL).  k == 0 everywhere gives the VL = false result exactly.
// SOLVE: wave_skip_wins.  ucb_value, its operation order and the tie-break are the same in all instantiations.
// FPU (sz_set_fpu; include/sigmazero.h is the rule): the score of an unvisited child (n_c = N_c + k_c == 0) is replaced by q0 + ucb_u(0, P_c, sq,
// c_puct), q0 = (v0 + 1) / 2.  mode / value: the site's (the root's at depth 0, the tree's below; uniform); pN / pW: the parent's own stored
// edge; all four are unread without FPU.  v0 and with it q0 are formed once per parent and are the same in every lane: the xor butterfly leaves
// one sum in all 64 (f32 addition commutes), and it is read back through readfirstlane so that the compiler knows.  mode == SZ_FPU_REFERENCE
// scores every child as without FPU.  With FPU ucb_out receives skipped WIN children too; without, the skip comes before the child is read.
template <bool VL, bool SOLVE, bool FPU>
__device__ __forceinline__ int wave_select_child(const EdgeStat* ch, const EdgeMeta* cm, const int* k, int n, int parentVC, float c_puct, float lam,
                                                 int mode, float value, int pN, double pW, float* ucb_out) {
    const int lane = lane_id();
    const float sq = (float)sqrt((double)parentVC);                     // math.sqrt(self.visit_count) in double, then a float32 operand
    const bool skip_wins = wave_skip_wins<SOLVE>(cm, n);
    float q0 = 0.5f;
    if constexpr (FPU) {
        if (mode != SZ_FPU_REFERENCE) {
            float v0 = value;
            if (mode == SZ_FPU_REDUCTION) {
                float part = 0.f;                                        // the prior mass of the visited children, a label does not matter
                for (int c = lane; c < n; c += 64) {
                    const EdgeStat s = ch[c];
                    int nc = s.N;
                    if constexpr (VL) nc += k[c];
                    if (nc >= 1) part = part + s.P;
                }
                const float mass = __int_as_float(uni(__float_as_int(wave_sum_butterfly(part))));
                const float vp = (float)pW / ((float)pN + 1e-6f);
                v0 = vp - (value * (float)sqrt((double)mass));
            }
            if (!(v0 >= -1.0f)) v0 = -1.0f;
            if (v0 > 1.0f) v0 = 1.0f;
            q0 = (v0 + 1.0f) / 2.0f;
        }
    }
    float best = 0.f; int bi = 0x7fffffff;
    for (int c = lane; c < n; c += 64) {
        if constexpr (SOLVE && !FPU) { if (skip_wins && (cm[c].pad & PR_MASK) == PR_WIN) continue; }
        const EdgeStat s = ch[c];
        int kc = 0;
        if constexpr (VL) kc = k[c];
        const int nc = s.N + kc;
        float u;
        if (!FPU || nc >= 1 || mode == SZ_FPU_REFERENCE) {
            if constexpr (VL) u = ucb_value(nc, s.W + (double)lam * (double)kc, s.P, sq, c_puct);
            else u = ucb_value(s.N, s.W, s.P, sq, c_puct);
        } else u = q0 + ucb_u(0, s.P, sq, c_puct);
        if (ucb_out) ucb_out[c] = u;
        if constexpr (SOLVE && FPU) { if (skip_wins && (cm[c].pad & PR_MASK) == PR_WIN) continue; }
        if (bi == 0x7fffffff || u > best) { best = u; bi = c; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        float ob = __shfl_xor(best, off); int oi = __shfl_xor(bi, off);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    return uni(bi);
}

// NON-REFERENCE option (sz_set_forced_playouts): what the FORCED instantiations take on top of View, an argument of their own like BeginOpts
struct ForcedOpts {
    float k;                    // the forced constant of the searches begun since the last sz_search_begin
    const uint8_t* boards;      // [B] != 0: the board's next search is forced and pruned; k_search_begin latches it into ST_FORCED
    unsigned long long* stat;   // [B][2] root selections decided by a forced child, visits pruning took out of the records
};

// NON-REFERENCE option (sz_set_endings): the per-board state of the ending rules, reset when a game starts on the board ...
struct EndState { int rs[2]; int ds; int would_ply; int would_kind; int would_colour; };     // resign streak per colour, draw streak, the holdout mark (would_ply -1 = none)
enum { END_STREAK_MAX = 65535 };                                                             // streaks saturate here: the largest patience
// ... and what k_play's ENDING instantiations take on top of View, and of ForcedOpts when both options are on: k_play<SOLVE, EndOpts>,
// k_play<SOLVE, ForcedOpts, EndOpts>.  k_search_begin and k_search_step have no ending variant: the option lives in sz_play alone.
struct EndOpts {
    sz_ending_options o;        // o.proven is already 0 when the solver is off
    EndState* state;            // [B]
    const uint8_t* holdout;     // [B] != 0: a firing rule marks the board and ends nothing
    uint8_t* kind;              // [B] SZ_END_* of the last sz_play (0 for a board that did not play in it) ...
    double* mval;               // [B] ... and the mover's value m it saw (NaN likewise)
    unsigned long long* stat;   // [B][4] resignations, adjudicated draws, proven endings, holdout marks
};

// NON-REFERENCE option (sz_set_move_temperature): what k_play's TEMPERATURE instantiations take on top of View, after ForcedOpts and before EndOpts
// when those options are on: k_play<SOLVE, [ForcedOpts,] TempOpts[, EndOpts]>.  Never beside GumbelOpts (Gumbel chooses its own move).
// k_search_begin, k_search_step and k_play_moves have no variant: the option lives in sz_play's move choice alone.
struct TempOpts {
    sz_temperature_options o;
    const double* temps;        // [B] the caller's temperatures, read by every sz_play while the option is on
    double* work;               // [B][SZ_MAX_MOVES] the per-child weights, formed by the lanes, summed by one lane in child order
    int* nelig;                 // [B] eligible children of the last sz_play (0 for a board that did not play in it) ...
    double* pch;                // [B] ... and w_chosen / S (NaN likewise)
    unsigned long long* stat;   // [B][3] plays sampled by the rule, greedy plays under the option, visited children excluded
};
enum { TEMP_SAMPLED = 0, TEMP_GREEDY = 1, TEMP_PROVEN = 2 };                                  // how wave_temperature came to its move

// NON-REFERENCE option (sz_set_lcb; include/sigmazero.h is the rule, sz_lcb.h the scalar arithmetic): the second moment of every edge and
// lower-confidence-bound move selection.  Two structs, each the last member of its pack.  SpreadOpts is what the instantiations of
// k_search_begin and k_search_step that keep the second moment take on top of everything else: k_search_begin<VL, SOLVE, [ForcedOpts,] SpreadOpts>,
// k_search_step<VL, SOLVE, [ForcedOpts,] [FpuOpts,] [PuctOpts,] SpreadOpts>.  Q is written at these sites and nowhere else:
//   zeroed    the root edge of a fresh root (k_search_begin); the children at expansion (k_search_step, beside s.W = 0.0; s.N = 0)
//   Q += sv^2 wave_backprop, every caller: the network leaf (every pending leaf under leaf batching, in leaf order), the solver's proven stop (a
//             proven root counts its budget out through it, one simulation at a time), the visited terminal, the new terminal
//   counted   the terminal root in k_search_begin: Q = (tv * tv) * (double)S beside W = tv * (double)S
// LcbOpts is what k_play's instantiations take after every other option: k_play<SOLVE, [ForcedOpts,] [PuctOpts,] [TempOpts,] [EndOpts,] LcbOpts>.
// Never beside GumbelOpts / GumbelTreeOpts, never on a reuse_subtree engine (wave_keep_subtree does not compact Q).
struct SpreadOpts {
    double* Q;                  // [B][e_cap] the sum of the squares of the values backed up through each edge, edge-indexed like Batch::vk
};
struct LcbOpts {
    sz_lcb_options o;
    const double* Q;            // SpreadOpts::Q
    int* move;                  // [B] the rule's move (child index) of the last sz_play, -1 for a board that made no choice ...
    int* cstar;                 // [B] ... the first maximum of the counts the move choice reads (-1 likewise) ...
    double* lcb2;               // [B][2] ... their two bounds (NaN likewise, and where the child has N < 2) ...
    int* ncand;                 // [B] ... the number of candidates (0 likewise) ...
    uint8_t* decided;           // [B] ... and whether the rule decided the move played (0 likewise)
    unsigned long long* stat;   // [B][3] plays the rule decided, plays where its move differs from c*, ssqrt arguments treated as 0.0
};

// forced playouts at a root (sz_set_forced_playouts): child c with n_c = N_c + k_c >= 1 visits is forced while n_c < sqrt((k * P_c) * T) in f64,
// T = parentVC - 1.  Returns the forced child with the lowest index, -1 when none is forced: the arg-max decides as everywhere.  Lanes = children
// as in wave_select_child; with SOLVE a child proven WIN is not forced whenever the arg-max skips WIN children.  A NaN or negative product forces nothing.
template <bool VL, bool SOLVE>
__device__ __forceinline__ int wave_forced_child(const EdgeStat* ch, const EdgeMeta* cm, const int* k, int n, int parentVC, float fk) {
    const int lane = lane_id();
    const bool skip_wins = wave_skip_wins<SOLVE>(cm, n);
    const double T = (double)(parentVC - 1);
    int fi = 0x7fffffff;
    for (int c = lane; c < n && fi == 0x7fffffff; c += 64) {
        if constexpr (SOLVE) { if (skip_wins && (cm[c].pad & PR_MASK) == PR_WIN) continue; }
        const EdgeStat s = ch[c];
        int nc = s.N;
        if constexpr (VL) nc += k[c];
        if (nc >= 1 && (double)nc < sqrt(((double)fk * (double)s.P) * T)) fi = c;
    }
    for (int off = 32; off >= 1; off >>= 1) { const int oi = __shfl_xor(fi, off); if (oi < fi) fi = oi; }
    fi = uni(fi);
    return fi == 0x7fffffff ? -1 : fi;
}

// selection at the root of a forced board without first-play urgency: the lowest forced child if there is one (*forced = true), else the arg-max
// as everywhere.  With FPU k_search_step composes the two itself.
template <bool VL, bool SOLVE>
__device__ __forceinline__ int wave_select_root_forced(const EdgeStat* ch, const EdgeMeta* cm, const int* k, int n, int parentVC, float c_puct, float lam, float fk,
                                                       bool* forced) {
    int bi = wave_forced_child<VL, SOLVE>(ch, cm, k, n, parentVC, fk);
    *forced = bi >= 0;
    if (bi < 0) bi = wave_select_child<VL, SOLVE, false>(ch, cm, k, n, parentVC, c_puct, lam, SZ_FPU_REFERENCE, 0.f, 0, 0.0, nullptr);
    return bi;
}

// NON-REFERENCE option (sz_set_fpu): what the FPU instantiations of k_search_step take on top of View, and of ForcedOpts when both options are
// on: k_search_step<VL, SOLVE, FpuOpts>, k_search_step<VL, SOLVE, ForcedOpts, FpuOpts>.  k_search_begin and k_play have no FPU variant.
struct FpuOpts { sz_fpu_options o; };

// NON-REFERENCE option (sz_set_cpuct): what the instantiations with a visit-dependent exploration rate take on top of View, after ForcedOpts and
// FpuOpts and before TempOpts when those options are on: k_search_step<VL, SOLVE, [ForcedOpts,] [FpuOpts,] PuctOpts> and, because pruning is its
// only use of c, k_play<SOLVE, ForcedOpts, PuctOpts[, TempOpts][, EndOpts]>.  Never beside GumbelOpts / GumbelTreeOpts.  k_search_begin and
// k_play_moves have no variant.
struct PuctOpts { sz_cpuct_options o; };
// the f32 that takes c_puct's place at a parent with n_p visits (include/sigmazero.h is the rule; sz_cpuct.h the arithmetic): the root's triple
// where a child of the root is selected and in pruning, the tree's below.  n_p and root are uniform, and so is the result.
__device__ __forceinline__ float puct_c(const sz_cpuct_options& o, int n_p, bool root) {
    return sz_cpuct(root ? o.root_init : o.tree_init, root ? o.root_base : o.tree_base, root ? o.root_factor : o.tree_factor, n_p);
}

// NON-REFERENCE option (sz_set_gumbel): what the GUMBEL instantiations take on top of View, before FpuOpts when both options are on:
// k_search_step<false, false, GumbelOpts[, FpuOpts]> and k_play<false, GumbelOpts>.  k_search_begin has no variant: the root's network value is
// kept where the root is expanded, in k_search_step.  Leaf batching, the solver, forced playouts and endings are refused with the option.
struct GumbelOpts {
    sz_gumbel_options o;
    const double* g;            // [B][SZ_MAX_MOVES] Gumbel(0,1) draws by root child, NULL = all zeros
    float* vhat;                // [B] the root's network value, written where the root is expanded
    float* policy;              // [B][SZ_MAX_MOVES] the improved policy of the last sz_play
    double* vmix;               // [B] ... and its v_mix
    double* work;               // [B][SZ_MAX_MOVES] k_play's per-child terms, summed by one lane in child order
    unsigned long long* stat;   // [B][2] root selections made by the rule, of them over all children because none was at the level
};

// the mover's value of a visited root child in [0, 1] (a child's W is stored from the child's side to move) ...
__device__ __forceinline__ double gumbel_q(const EdgeStat& s) { return 0.5 - 0.5 * (s.W / (double)s.N); }
// ... and the factor of sigma(x) = (((double)c_visit + (double)maxN) * (double)c_scale) * x
__device__ __forceinline__ double gumbel_sigma_factor(const sz_gumbel_options& o, int maxN) { return ((double)o.c_visit + (double)maxN) * (double)o.c_scale; }

__device__ __forceinline__ int wave_max_visits(const EdgeStat* ch, int n) {
    int mx = 0;
    for (int c = lane_id(); c < n; c += 64) { const int nc = ch[c].N; if (nc > mx) mx = nc; }
    for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(mx, off); if (o > mx) mx = o; }
    return uni(mx);
}

// the arg-max of s_c = (g_c + slog(P_c)) + sigma(q_c) (the sigma term 0.0 at N_c = 0) over the children with N_c == level, over all of them with
// level < 0; sf = gumbel_sigma_factor.  wave_select_child's loop, butterfly and first-maximum tie-break in f64.  -1: no child is at the level.
__device__ __forceinline__ int wave_gumbel_best(const EdgeStat* ch, const double* g, int n, int level, double sf) {
    const int lane = lane_id();
    double best = 0.0; int bi = 0x7fffffff;
    for (int c = lane; c < n; c += 64) {
        const EdgeStat s = ch[c];
        if (level >= 0 && s.N != level) continue;
        const double gl = (g ? g[c] : 0.0) + sz_slog((double)s.P);
        double sig = 0.0;
        if (s.N >= 1) sig = sf * gumbel_q(s);
        const double sc = gl + sig;
        if (bi == 0x7fffffff || sc > best) { best = sc; bi = c; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        double ob = __shfl_xor(best, off); int oi = __shfl_xor(bi, off);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    bi = uni(bi);
    return bi == 0x7fffffff ? -1 : bi;
}

// root selection at root-child visit t of a search of `goal` simulations (sz_set_gumbel): the level of t by sequential halving over
// m_eff = min(max_considered, n) children, then the best child at that level; *fallback = no child was there and all were considered
__device__ __forceinline__ int wave_select_root_gumbel(const EdgeStat* ch, const double* g, int n, int t, int goal, const sz_gumbel_options& o, bool* fallback) {
    const int m_eff = o.max_considered < n ? o.max_considered : n;
    const int level = sz_gumbel_level(t, goal - 1, m_eff);
    const double sf = gumbel_sigma_factor(o, wave_max_visits(ch, n));
    int bi = wave_gumbel_best(ch, g, n, level, sf);
    *fallback = bi < 0;
    if (bi < 0) bi = wave_gumbel_best(ch, g, n, -1, sf);
    return bi;
}

// NON-REFERENCE option (sz_set_gumbel_tree, on top of sz_set_gumbel): what k_search_step<false, false, GumbelTreeOpts> takes in GumbelOpts' place.
// k_play and k_search_begin have no variant: sz_play receives the GumbelOpts part.  FpuOpts is never beside it: under the rule neither of
// sz_set_fpu's sites is consulted.
struct GumbelTreeOpts : GumbelOpts {
    float* nval;                // [B][n_cap] the network value of every node by node id, written where the node is expanded
    unsigned long long* tstat;  // [B] selections below the root made by the rule
};
// the GumbelOpts of a pack that holds GumbelOpts or GumbelTreeOpts
template <typename F, typename... R>
__device__ __forceinline__ const GumbelOpts& gumbel_of(const F& f, const R&... r) {
    if constexpr (std::is_base_of_v<GumbelOpts, F>) return f; else return gumbel_of(r...);
}

// wsum of sz_set_gumbel_tree: the lanes' partial sums through the xor butterfly.  f64 addition commutes, so all 64 lanes end with the same bits;
// read back through readfirstlane so that the compiler knows.
__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return uni_f64(v);
}

// selection below the root under sz_set_gumbel_tree (include/sigmazero.h is the rule): the arg-max over the children ch[0..n), n >= 1, of
// softmax(slog(P_c) + sigma(completed q_c))_c - N_c / (1 + sumN), first maximum, wave_gumbel_best's loop and butterfly tie-break.  vhat: the
// parent's own network value.  Lanes = children, up to four per lane, whose z_c / e_c stay in registers.  score_out [n] and vmix_out (both
// optional, the test hook) receive every child's score and v_mix.
__device__ __forceinline__ int wave_select_tree_gumbel(const EdgeStat* ch, int n, const sz_gumbel_options& o, float vhat, double* score_out, double* vmix_out) {
    constexpr int R = (SZ_MAX_CHILDREN + 63) / 64;
    const int lane = lane_id();
    int maxN = 0, sumN = 0; double pq = 0.0, pm = 0.0;
    for (int c = lane; c < n; c += 64) {
        const EdgeStat s = ch[c];
        if (s.N > maxN) maxN = s.N;
        sumN += s.N;
        double tq = 0.0, tm = 0.0;
        if (s.N >= 1) { tq = (double)s.P * gumbel_q(s); tm = (double)s.P; }
        pq = pq + tq; pm = pm + tm;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const int om = __shfl_xor(maxN, off); if (om > maxN) maxN = om;
        sumN += __shfl_xor(sumN, off);
    }
    maxN = uni(maxN); sumN = uni(sumN);
    pq = wave_sum_f64(pq); pm = wave_sum_f64(pm);
    const double sf = gumbel_sigma_factor(o, maxN);
    const double v01 = 0.5 + 0.5 * (double)vhat;
    double vmix = v01;
    if (sumN != 0) vmix = (v01 + (double)sumN * (pq / pm)) / (1.0 + (double)sumN);
    double z[R]; double zmax = 0.0; bool any = false;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int c = lane + 64 * j;
        z[j] = 0.0;
        if (c < n) {
            const EdgeStat s = ch[c];
            z[j] = sz_slog((double)s.P) + sf * (s.N >= 1 ? gumbel_q(s) : vmix);
            if (!any || z[j] > zmax) { zmax = z[j]; any = true; }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double oz = __shfl_xor(zmax, off); const int oa = __shfl_xor((int)any, off);
        if (oa && (!any || oz > zmax)) { zmax = oz; any = true; }
    }
    zmax = uni_f64(zmax);
    double se = 0.0;
#pragma unroll
    for (int j = 0; j < R; j++) {
        if (lane + 64 * j < n) { z[j] = sz_sexp(z[j] - zmax); se = se + z[j]; }
    }
    se = wave_sum_f64(se);
    const double dn = 1.0 + (double)sumN;
    double best = 0.0; int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int c = lane + 64 * j;
        if (c < n) {
            const double sc = (z[j] / se) - ((double)ch[c].N / dn);
            if (score_out) score_out[c] = sc;
            if (bi == 0x7fffffff || sc > best) { best = sc; bi = c; }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        double ob = __shfl_xor(best, off); int oi = __shfl_xor(bi, off);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    if (vmix_out && lane == 0) *vmix_out = vmix;
    return uni(bi);
}

// sz_play on a Gumbel board: the move (the best child among the most visited) and the completed-Q improved policy of the root's children
// ch[0..n), n >= 1.  work[0..n) (LDS or global) carries the per-child terms between the lanes that form them and lane 0, which adds them up
// in ascending child order.  policy_out[0..SZ_MAX_MOVES) and *vmix_out are written; returns the move (uniform).
__device__ __forceinline__ int wave_gumbel_play(const EdgeStat* ch, const double* g, int n, const sz_gumbel_options& o, float vhat, double* work,
                                                float* policy_out, double* vmix_out) {
    const int lane = lane_id();
    const int maxN = wave_max_visits(ch, n);
    const double sf = gumbel_sigma_factor(o, maxN);
    const int move = wave_gumbel_best(ch, g, n, maxN, sf);
    const double v01 = 0.5 + 0.5 * (double)vhat;
    for (int c = lane; c < n; c += 64) { const EdgeStat s = ch[c]; work[c] = s.N >= 1 ? (double)s.P * gumbel_q(s) : 0.0; }
    __threadfence_block();
    __syncthreads();
    double vmix = v01;
    if (lane == 0) {
        int sumN = 0; double pq = 0.0, pm = 0.0;
        for (int c = 0; c < n; c++) {
            const EdgeStat s = ch[c];
            sumN += s.N;
            if (s.N >= 1) { pq = pq + work[c]; pm = pm + (double)s.P; }
        }
        if (sumN != 0) vmix = (v01 + (double)sumN * (pq / pm)) / (1.0 + (double)sumN);
    }
    vmix = uni_f64(vmix);
    __syncthreads();
    double zmax = 0.0; bool any = false;
    for (int c = lane; c < n; c += 64) {
        const EdgeStat s = ch[c];
        const double z = sz_slog((double)s.P) + sf * (s.N >= 1 ? gumbel_q(s) : vmix);
        work[c] = z;
        if (!any || z > zmax) { zmax = z; any = true; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double oz = __shfl_xor(zmax, off); const int oa = __shfl_xor((int)any, off);
        if (oa && (!any || oz > zmax)) { zmax = oz; any = true; }
    }
    zmax = uni_f64(zmax);
    for (int c = lane; c < n; c += 64) work[c] = sz_sexp(work[c] - zmax);      // a lane reads back what it wrote itself
    __threadfence_block();
    __syncthreads();
    double se = 0.0;
    if (lane == 0) for (int c = 0; c < n; c++) se = se + work[c];
    se = uni_f64(se);
    for (int c = lane; c < SZ_MAX_CHILDREN; c += 64) policy_out[c] = c < n ? (float)(work[c] / se) : 0.0f;
    if (lane == 0) *vmix_out = vmix;
    return move;
}

// policy-target pruning of a finished search (sz_set_forced_playouts): vis[0..n) holds the root children's counted visits N_c on entry and the
// pruned counts n' on return (LDS, lanes = children).  c* = the first maximum of N_c keeps its count; every other visited child loses visits one
// at a time, at most m_c = min(N_c, floor(sqrt((k * P_c) * (rootN - 1)))) of them, while its PUCT value with q held at the counted N_c, W_c stays
// below c*'s; a child left with one visit loses that too.  Returns the visits taken out (uniform); *cstar_out (optional) = c*.
__device__ __forceinline__ int wave_prune(const EdgeStat* ch, int n, int rootN, float c_puct, float fk, int* vis, int* cstar_out) {
    const int lane = lane_id();
    int bn = -1, bi = 0x7fffffff;
    for (int c = lane; c < n; c += 64) { const int nc = vis[c]; if (nc > bn) { bn = nc; bi = c; } }
    for (int off = 32; off >= 1; off >>= 1) {
        const int on = __shfl_xor(bn, off), oi = __shfl_xor(bi, off);
        if (on > bn || (on == bn && oi < bi)) { bn = on; bi = oi; }
    }
    const int cs = uni(bi);
    const float sq = (float)sqrt((double)rootN);
    const EdgeStat top = ch[cs];
    const float best = ucb_value(vis[cs], top.W, top.P, sq, c_puct);
    const double T = (double)(rootN - 1);
    int cut = 0;
    for (int c = lane; c < n; c += 64) {
        const int nc = vis[c];
        if (c == cs || nc < 1) continue;
        const EdgeStat s = ch[c];
        const double lim = sqrt(((double)fk * (double)s.P) * T);
        int m = 0;                                                          // NaN (a NaN prior, a negative product): nothing is pruned
        if (lim >= (double)nc) m = nc; else if (lim >= 0.0) m = (int)floor(lim);
        const float q = ucb_q(nc, s.W);
        int np = nc;
        for (int i = 0; i < m; i++) {
            const int cand = np - 1;
            if (q + ucb_u(cand, s.P, sq, c_puct) < best) np = cand; else break;
        }
        if (np < nc && np <= 1) np = 0;
        vis[c] = np;
        cut += nc - np;
    }
    for (int off = 32; off >= 1; off >>= 1) cut += __shfl_xor(cut, off);
    if (cstar_out && lane == 0) *cstar_out = cs;
    return uni(cut);
}

// the ending rules of sz_set_endings on a finished search (sz_play): ch[0..n) the root's children with their counted visits (lanes = children),
// code the root's proven code (PR_UNKNOWN without the solver), colour the side to move (1 white), ply the root's ply.  c* = the first maximum
// of N_c, m = -(W_c* / N_c*) in f64.  Order: proven root (o.proven; streaks untouched, holdout ignored), then the streaks are advanced, then
// resign before draw.  On a holdout board a firing rule records the board's first mark (*marked = true) and ends nothing.  Returns the kind
// that ends the game (SZ_END_NONE: the ply is played); st is advanced in place, *m_out = m.  Every lane returns the same.
__device__ __forceinline__ int wave_ending(const EdgeStat* ch, int n, int code, int colour, int ply, EndState& st, const sz_ending_options& o, bool holdout,
                                           double* m_out, bool* marked) {
    const int lane = lane_id();
    int bn = -1, bi = 0x7fffffff;
    for (int c = lane; c < n; c += 64) { const int nc = ch[c].N; if (nc > bn) { bn = nc; bi = c; } }
    for (int off = 32; off >= 1; off >>= 1) {
        const int on = __shfl_xor(bn, off), oi = __shfl_xor(bi, off);
        if (on > bn || (on == bn && oi < bi)) { bn = on; bi = oi; }
    }
    const EdgeStat top = ch[uni(bi)];
    const double m = -(top.W / (double)top.N);
    *m_out = m;
    *marked = false;
    if (o.proven && code != PR_UNKNOWN) return SZ_END_PROVEN;
    const int col = colour ? 1 : 0;
    if (m <= (double)o.resign_value) { if (st.rs[col] < END_STREAK_MAX) st.rs[col]++; } else st.rs[col] = 0;
    if (fabs(m) <= (double)o.draw_value) { if (st.ds < END_STREAK_MAX) st.ds++; } else st.ds = 0;
    const bool fire_resign = o.resign_patience > 0 && st.rs[col] >= o.resign_patience && ply >= o.resign_min_ply;
    const bool fire_draw = o.draw_patience > 0 && st.ds >= o.draw_patience && ply >= o.draw_min_ply;
    int kind = fire_resign ? SZ_END_RESIGN : (fire_draw ? SZ_END_DRAW : SZ_END_NONE);
    if (kind != SZ_END_NONE && holdout) {
        if (st.would_ply < 0) { st.would_ply = ply; st.would_kind = kind; st.would_colour = col; *marked = true; }
        kind = SZ_END_NONE;
    }
    return kind;
}
// the result of a game ended by `kind`: +1 white wins, -1 black wins, 0 draw
__device__ __forceinline__ int ending_result(int kind, int code, int colour) {
    const int mover = colour ? 1 : -1;
    if (kind == SZ_END_RESIGN) return -mover;
    if (kind == SZ_END_PROVEN) return code == PR_WIN ? mover : (code == PR_LOSS ? -mover : 0);
    return 0;
}

// the move of sz_play under sz_set_move_temperature (include/sigmazero.h is the rule): ch[0..n) the root's children with their counted N and W,
// vis[0..n) the counts today's sampling reads (LDS: the counted visits, or wave_prune's pruned counts), T the board's temperature, u its
// uniform, pmove the first child proven LOSS of a root proven WIN (-1: none, or no solver).  The lanes form the weights w_c into work[0..n)
// (one sz_slog and one sz_sexp per child), lane 0 adds them up in child order and runs today's two sequential passes over w_c / S.
// *kind = TEMP_*; *nelig, *pch and *excl as sz_fetch_temperature and sz_temperature_stats report them.  Every lane returns the same.
__device__ __forceinline__ int wave_temperature(const EdgeStat* ch, const int* vis, int n, const sz_temperature_options& o, double T, double u, int pmove,
                                                double* work, int* kind, int* nelig, double* pch, int* excl) {
    const int lane = lane_id();
    int bn = -1, bi = 0x7fffffff;
    for (int c = lane; c < n; c += 64) { const int nc = vis[c]; if (nc > bn) { bn = nc; bi = c; } }
    for (int off = 32; off >= 1; off >>= 1) {
        const int on = __shfl_xor(bn, off), oi = __shfl_xor(bi, off);
        if (on > bn || (on == bn && oi < bi)) { bn = on; bi = oi; }
    }
    const int cs = uni(bi);
    const double voff = (double)o.visit_offset;
    const double astar = (double)uni(bn) + voff;
    *nelig = 1; *pch = 1.0; *excl = 0;
    if (pmove >= 0) { *kind = TEMP_PROVEN; return pmove; }
    if (u < 0.0 || !(T > 0.0) || astar <= 0.0) { *kind = TEMP_GREEDY; return cs; }
    *kind = TEMP_SAMPLED;
    const EdgeStat top = ch[cs];
    const double floor_m = -(top.W / (double)top.N) - (double)o.value_cutoff;
    double lstar = 0.0;
    if (T != 1.0) lstar = sz_slog(astar);
    int ne = 0, ex = 0;
    for (int c = lane; c < n; c += 64) {
        const int nc = vis[c];
        double w = 0.0;
        if (nc >= 1) {
            const double a = (double)nc + voff;
            bool ok = a > 0.0;
            if (ok && o.use_cutoff) { const EdgeStat s = ch[c]; ok = -(s.W / (double)s.N) >= floor_m; }
            if (ok) {
                ne++;
                if (T == 1.0) w = a;
                else { double d = sz_slog(a) - lstar; if (d > 0.0) d = 0.0; w = sz_sexp(d / T); }
            } else ex++;
        }
        work[c] = w;
    }
    for (int off = 32; off >= 1; off >>= 1) { ne += __shfl_xor(ne, off); ex += __shfl_xor(ex, off); }
    __threadfence_block();
    __syncthreads();
    int chosen = 0; double p = 0.0;
    if (lane == 0) {
        double S = 0.0;
        for (int c = 0; c < n; c++) S = S + work[c];
        double acc = 0.0;
        for (int c = 0; c < n; c++) acc += work[c] / S;
        const double last = acc;
        acc = 0.0;
        int idx = 0;
        for (int c = 0; c < n; c++) { acc += work[c] / S; if (acc / last <= u) idx = c + 1; }
        if (idx >= n) idx = n - 1;
        chosen = idx; p = work[idx] / S;
    }
    *nelig = uni(ne); *excl = uni(ex); *pch = uni_f64(p);
    return uni(chosen);
}

// the move of sz_set_lcb on a finished search (include/sigmazero.h is the rule, sz_lcb.h the arithmetic): ch[0..n) the root's children with the
// tree's N and W, Q[0..n) their square sums, vis[0..n) the counts the move choice reads.  Lanes = children: c* is the first maximum of vis
// (wave_ending's butterfly), every child's bound is formed once (lcb_out, optional, receives them), and the first maximum of the bounds over the
// candidates is found with wave_select_child's butterfly and lowest-index tie-break.  Without a candidate the move is c*.  *lcb_move / *lcb_star:
// the bounds of the move and of c* (NaN with N < 2); *ncand: the candidates; *bad: ssqrt arguments treated as 0.0.  Every lane returns the same.
__device__ __forceinline__ int wave_lcb(const EdgeStat* ch, const double* Q, const int* vis, int n, const sz_lcb_options& o, double* lcb_out, int* cstar,
                                        double* lcb_move, double* lcb_star, int* ncand, int* bad) {
    const int lane = lane_id();
    int bn = -1, ci = 0x7fffffff;
    for (int c = lane; c < n; c += 64) { const int nc = vis[c]; if (nc > bn) { bn = nc; ci = c; } }
    for (int off = 32; off >= 1; off >>= 1) {
        const int on = __shfl_xor(bn, off), oi = __shfl_xor(ci, off);
        if (on > bn || (on == bn && oi < ci)) { bn = on; ci = oi; }
    }
    const int cs = uni(ci), nstar = uni(bn);
    const double z = (double)o.stdevs, p = (double)o.min_visit_prop;
    double best = 0.0, vstar = sz_lcb_nan(); int bi = 0x7fffffff;
    int cand = 0, nbad = 0;
    for (int c = lane; c < n; c += 64) {
        const EdgeStat s = ch[c];
        const double val = sz_lcb_value(s.N, s.W, Q[c], z, &nbad);
        if (lcb_out) lcb_out[c] = val;
        if (c == cs) vstar = val;
        if (!sz_lcb_candidate(s.N, vis[c], nstar, p)) continue;
        cand++;
        if (bi == 0x7fffffff || val > best) { best = val; bi = c; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off); const int oi = __shfl_xor(bi, off);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
        cand += __shfl_xor(cand, off); nbad += __shfl_xor(nbad, off);
    }
    bi = uni(bi);
    // c*'s bound lives in the lane that owns c* (cs & 63): hand it to every lane
    vstar = __shfl(vstar, cs & 63);
    *cstar = cs; *ncand = uni(cand); *bad = uni(nbad);
    *lcb_star = uni_f64(vstar);
    if (bi == 0x7fffffff) { *lcb_move = *lcb_star; return cs; }
    *lcb_move = uni_f64(best);
    return bi;
}

// solver update after a backup whose last node path[d] has just become proven: walk towards the root; the parent of a newly proven node is
// recomputed from its children alone (lanes = children): WIN if any child is LOSS, else, when it is complete and every child is proven,
// DRAW if any child is DRAW, else LOSS.  The walk ends at the first node that stays UNKNOWN.  Returns the number of nodes proven.
__device__ __forceinline__ int wave_solver_update(EdgeMeta* em, const int* path, int d) {
    const int lane = lane_id();
    int proved = 0;
    for (int j = d; j > 0; j--) {
        const int p = path[j - 1];
        const EdgeMeta pm = em[p];
        const int first = uni(pm.first), n = uni((int)pm.n), ppad = uni((int)pm.pad);
        bool loss = false, draw = false, open = false;
        for (int c = lane; c < n; c += 64) {
            const int r = em[first + c].pad & PR_MASK;
            loss |= r == PR_LOSS; draw |= r == PR_DRAW; open |= r == PR_UNKNOWN;
        }
        const int r = __ballot(loss) ? PR_WIN : (((ppad & PR_COMPLETE) && !__ballot(open)) ? (__ballot(draw) ? PR_DRAW : PR_LOSS) : PR_UNKNOWN);
        if (r == (ppad & PR_MASK)) break;
        if (lane == 0) em[p].pad = (unsigned short)((ppad & ~PR_MASK) | r);
        __threadfence_block();
        proved++;
    }
    return proved;
}

// the root-noise mix of sz_set_root_noise / sz_set_search_root_noise over the K children ch[0..K) of a root, g = the board's Gamma draws:
// gs from lane-strided partial sums (lane l adds g[l], g[l+64], ... ascending) and an xor butterfly, then P = 0.75*P + 0.25*(g/gs) in place.
// One function for both sites: the d == 0 expansion of k_search_step (fresh root) and k_search_begin's reuse branch (kept root).
__device__ __forceinline__ void wave_root_noise(EdgeStat* ch, const float* g, int K) {
    const int lane = lane_id();
    float gs = 0.f;
    for (int c = lane; c < K; c += 64) gs = gs + g[c];
    gs = wave_sum_butterfly(gs);
    for (int c = lane; c < K; c += 64) ch[c].P = (0.75f * ch[c].P) + (0.25f * (g[c] / gs));
}

// what k_search_begin alone reads of sz_set_visit_targets / sz_set_search_root_noise: an argument of its own, so that View, which every kernel takes, stays as it is
struct BeginOpts {
    const int* target;          // sz_set_visit_targets: root visit target t of board b in 0..S, NULL = off.  k_search_begin turns it into the new
    int* goal;                  //   simulations of this search, goal[b] (t on a fresh root, max(0, t + 1 - N_kept) on a kept one); View::budget points at goal
    const uint8_t* quiet;       // sz_set_search_root_noise: quiet[b] != 0 = no root noise for board b; NULL = no board is quiet
};

struct BoardPtrs {
    SzPos* npos; SzPos* ring; EdgeStat* es; EdgeMeta* em; int* gpath; u64* pmask; Ctl* ctl;
};
// simulations this board's search runs: its own budget (sz_set_search_budgets), else num_searches
__device__ __forceinline__ int board_budget(const View& v, int b) { return v.budget ? uni(v.budget[b]) : v.S; }
__device__ __forceinline__ BoardPtrs board_ptrs(const View& v, int b) {
    BoardPtrs p;
    p.npos = v.npos + (size_t)b * v.n_cap;
    p.ring = v.ring + (size_t)b * SZ_RING;
    p.es = v.es + (size_t)b * v.e_cap;
    p.em = v.em + (size_t)b * v.e_cap;
    p.gpath = v.gpath + (size_t)b * v.p_cap;
    p.pmask = v.pmask + (size_t)b * PMASK_STRIDE;
    p.ctl = v.ctl + b;
    return p;
}

// where pending leaf li of board b keeps its descent path, legal-move mask and depth, and its row in the network batch (planes / policy /
// value).  VL = false: the board's one leaf, in its own records at row slot(b).  VL = true (sz_set_leaf_batching): leaf li of L, at row slot(b)*L + li.
struct LeafPtrs { int* path; u64* mask; int* depth; size_t row; };
template <bool VL>
__device__ __forceinline__ LeafPtrs leaf_ptrs(const View& v, const BoardPtrs& bp, const Batch& vb, int b, int row, int li) {
    LeafPtrs p;
    if constexpr (VL) {
        const size_t i = (size_t)b * vb.L + li;
        p.path = vb.path + i * v.p_cap; p.mask = vb.mask + i * PMASK_STRIDE; p.depth = vb.depth + i; p.row = (size_t)(row * vb.L + li);
    } else {
        p.path = bp.gpath; p.mask = bp.pmask; p.depth = &bp.ctl->pend_depth; p.row = (size_t)row;
    }
    return p;
}

// position `j` plies before a node at tree depth D whose root sits at game ply root_ply
__device__ __forceinline__ const SzPos* ancestor_ptr(const BoardPtrs& bp, const int* path, int D, int root_ply, int j) {
    int dj = D - j;
    if (dj >= 0) return bp.npos + bp.em[path[dj]].node;
    int ply = root_ply + dj;
    if (ply < 0 || -dj >= SZ_RING) return nullptr;
    return bp.ring + (ply & (SZ_RING - 1));
}

// ------------------------------------------------------------------------------------------------
// Move generation for position X (uniform), one lane per square.  Fills mask[0..72] in LDS and
// returns n_legal / ep_legal / checkers (uniform).
// ------------------------------------------------------------------------------------------------
__device__ void wave_movegen(const SzPos& X, int chess960, u64* mask_lds, int& n_legal, int& ep_legal, u64& checkers) {
    const int lane = lane_id();
    SzInfo I = sz_info(X);
    const int s = lane ^ sz_view_flip(I.white);
    const bool need = (I.need >> s) & 1;
    bool att = false;
    if (need) att = sz_danger_at(X, I, s);
    u64 danger = view_to_squares(__ballot(att), I.white);
    u64 T;
    if (s == I.ksq) T = sz_king_targets(X, I, danger, chess960);
    else T = sz_piece_targets(X, I, s);
    const bool is_pawn = (X.pc[SZ_P] >> s) & 1;
    int ep = szm_ep(X.meta);
    ep_legal = (ep >= 0) ? (__ballot(is_pawn && ((T >> ep) & 1)) != 0) : 0;
    // legal-move mask in action-index order (chess_tensor.py:190-218): 73 ballots over the lane's plane bits (sz_lane_plane_bits)
    const SzPlaneBits pb = sz_lane_plane_bits(T, is_pawn, lane, I.white);
    int n = 0;
#pragma unroll
    for (int pl = 0; pl < SZ_MASK_WORDS; pl++) {
        const uint32_t word = pl < 56 ? pb.q[pl / 7] : (pl < 64 ? pb.kn : pb.up);
        const int sh = pl < 56 ? pl % 7 : (pl < 64 ? pl - 56 : (pl - 64) % 3);
        const u64 w = __ballot((word >> sh) & 1u);
        if (lane == 0) mask_lds[pl] = w;
        n += __popcll(w);
    }
    n_legal = n;
    checkers = I.checkers;
}

// earlier occurrences of X (key) within the reversible window: Board.is_repetition walk-back, lanes = plies
__device__ int wave_count_reps(const BoardPtrs& bp, const int* path, int D, int root_ply, const SzPos& X) {
    if (szm_irrev(X.meta)) return 0;
    const int lane = lane_id();
    int window = szm_half(X.meta);
    if (window > SZ_RING - 1) window = SZ_RING - 1;
    int reps = 0;
    for (int base = 0; base < window; base += 64) {
        int j = base + lane + 1;
        bool in = j <= window;
        const SzPos* a = in ? ancestor_ptr(bp, path, D, root_ply, j) : nullptr;
        bool stop = in && (a == nullptr);
        bool eq = false;
        if (a) { u64 k = a->key, m = a->meta; eq = (k == X.key); stop = szm_irrev(m) != 0; }
        u64 eqm = __ballot(eq), stm = __ballot(stop || !in);
        if (stm) {
            int sidx = __builtin_ctzll(stm);
            u64 keep = (sidx >= 63) ? ~0ULL : ((2ULL << sidx) - 1);
            reps += __popcll(eqm & keep);
            break;
        }
        reps += __popcll(eqm);
    }
    return reps > 4 ? 4 : reps;
}

// stage the 8 history positions (leaf + 7 ancestors) as 8x8 u64 words in LDS
__device__ void wave_load_history(const BoardPtrs& bp, const int* path, int D, int root_ply, const SzPos& X, u64* hist_lds) {
    const int lane = lane_id();
    const int t = lane >> 3, w = lane & 7;
    u64 val = 0;
    if (t == 0) {
        val = w == 0 ? X.pc[0] : w == 1 ? X.pc[1] : w == 2 ? X.pc[2] : w == 3 ? X.pc[3] : w == 4 ? X.pc[4] : w == 5 ? X.pc[5] : w == 6 ? X.white : X.meta;
    } else {
        const SzPos* a = ancestor_ptr(bp, path, D, root_ply, t);
        if (a) val = ((const u64*)a)[w];
    }
    hist_lds[lane] = val;
}

// chess_tensor.py:131-142 get_representation for the leaf whose history sits in hist_lds.
// Every lane owns (plane, row): 8 cells = one 32-byte (f32) or 16-byte (bf16) store, fully coalesced.
__device__ void wave_encode(const u64* hist_lds, const SzPos& X, void* out_board, int dtype, uint8_t* packed_out) {
    const int lane = lane_id();
    const int vw = szm_turn(X.meta);
    if (dtype == SZ_PLANES_NHWC128_BITS && out_board) {
        // bit-packed NHWC image, 1 KiB per board = ONE 16-byte store per lane: lane l = psub*16 + cq owns channels
        // cq*8..cq*8+7; byte q of its uint4 = those 8 channel bits at position q*4 + psub (view order).  The stem
        // kernel (csrc/sz_nn.hip stage_tile_bits) expands the bits to bf16 while staging its LDS tile.
        const int cq = lane & 15, psub = lane >> 4;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int c = cq * 8 + k;
            u64 bb = (c < 112) ? sz_hist_plane(hist_lds + (c / 14) * 8, c % 14, vw) : (c < SZ_NUM_PLANES ? sz_aux_plane(X, c - 112) : 0ULL);
            // view position p <-> board square p ^ sz_view_flip: ^56 (white) = byte swap, ^7 (black) = bit reversal + byte swap
            bb = __builtin_bswap64(vw ? bb : __brevll(bb));
            bb >>= psub;
            const uint32_t lo = (uint32_t)bb, hi = (uint32_t)(bb >> 32);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                w[q >> 2] |= ((lo >> (4 * q)) & 1u) << ((q & 3) * 8 + k);
                w[2 + (q >> 2)] |= ((hi >> (4 * q)) & 1u) << ((q & 3) * 8 + k);
            }
        }
        ((uint4*)out_board)[lane] = make_uint4(w[0], w[1], w[2], w[3]);
        if (!packed_out) return;
        out_board = nullptr;
    }
    if (dtype == SZ_PLANES_NHWC128_BF16 && out_board) {
        // NHWC image [64 positions][128 channels] bf16 = 16 KB = 16 wave-instructions of 1 KiB, each fully contiguous:
        // in store q lane l covers position q*4 + (l>>4), channels (l&15)*8 .. +7.  A lane's 8 channel bitboards do not
        // depend on q, so they are formed once (8 planes per lane instead of 119) and only shifted per position.
        const int cq = lane & 15, psub = lane >> 4, flip = sz_view_flip(vw);
        u64 bb[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int c = cq * 8 + k;
            bb[k] = (c < 112) ? sz_hist_plane(hist_lds + (c / 14) * 8, c % 14, vw) : (c < SZ_NUM_PLANES ? sz_aux_plane(X, c - 112) : 0ULL);
        }
        uint4* dst = (uint4*)out_board + lane;
#pragma unroll 4
        for (int q = 0; q < 16; q++) {
            const int sq = (q * 4 + psub) ^ flip;
            uint4 o;
            o.x = (((bb[0] >> sq) & 1) ? 0x3F80u : 0u) | (((bb[1] >> sq) & 1) ? 0x3F800000u : 0u);
            o.y = (((bb[2] >> sq) & 1) ? 0x3F80u : 0u) | (((bb[3] >> sq) & 1) ? 0x3F800000u : 0u);
            o.z = (((bb[4] >> sq) & 1) ? 0x3F80u : 0u) | (((bb[5] >> sq) & 1) ? 0x3F800000u : 0u);
            o.w = (((bb[6] >> sq) & 1) ? 0x3F80u : 0u) | (((bb[7] >> sq) & 1) ? 0x3F800000u : 0u);
            dst[q * 64] = o;
        }
        if (!packed_out) return;
        out_board = nullptr;
    }
    const int r = lane & 7;
    for (int i = 0; i < 15; i++) {
        int c = i * 8 + (lane >> 3);
        if (c >= SZ_NUM_PLANES) break;
        u64 bb = (c < 112) ? sz_hist_plane(hist_lds + (c / 14) * 8, c % 14, vw) : sz_aux_plane(X, c - 112);
        uint32_t bits = sz_row_bits(bb, r, vw);
        if (packed_out) packed_out[c * 8 + r] = (uint8_t)bits;
        if (!out_board) continue;
        if (dtype == SZ_PLANES_F32) {
            float4* dst = (float4*)out_board + (size_t)(c * 8 + r) * 2;
            float4 a, b2;
            a.x = (bits & 1) ? 1.f : 0.f; a.y = (bits & 2) ? 1.f : 0.f; a.z = (bits & 4) ? 1.f : 0.f; a.w = (bits & 8) ? 1.f : 0.f;
            b2.x = (bits & 16) ? 1.f : 0.f; b2.y = (bits & 32) ? 1.f : 0.f; b2.z = (bits & 64) ? 1.f : 0.f; b2.w = (bits & 128) ? 1.f : 0.f;
            dst[0] = a; dst[1] = b2;
        } else {
            uint4 o;                                       // bf16 1.0 = 0x3F80
            o.x = ((bits & 1) ? 0x3F80u : 0u) | ((bits & 2) ? 0x3F800000u : 0u);
            o.y = ((bits & 4) ? 0x3F80u : 0u) | ((bits & 8) ? 0x3F800000u : 0u);
            o.z = ((bits & 16) ? 0x3F80u : 0u) | ((bits & 32) ? 0x3F800000u : 0u);
            o.w = ((bits & 64) ? 0x3F80u : 0u) | ((bits & 128) ? 0x3F800000u : 0u);
            ((uint4*)out_board)[c * 8 + r] = o;
        }
    }
}

// Node.backpropagate: one lane per level of the descent path (path[0] = root edge ... path[d] = leaf edge)
__device__ __forceinline__ void wave_backprop(EdgeStat* es, const int* path, int d, double v) {
    for (int j = lane_id(); j <= d; j += 64) {
        EdgeStat* e = es + path[j];
        double sv = ((d - j) & 1) ? -v : v;
        e->W = e->W + sv;
        e->N = e->N + 1;
    }
    __threadfence_block();
}
// ... and under sz_set_lcb (SpreadOpts): the square of the same sv beside it, in the same order.  sv * sv is exact, the sum one rounding.
__device__ __forceinline__ void wave_backprop(EdgeStat* es, double* Q, const int* path, int d, double v) {
    for (int j = lane_id(); j <= d; j += 64) {
        const int ei = path[j];
        EdgeStat* e = es + ei;
        double sv = ((d - j) & 1) ? -v : v;
        e->W = e->W + sv;
        e->N = e->N + 1;
        Q[ei] = Q[ei] + sv * sv;
    }
    __threadfence_block();
}

// make a new position from `parent` by action index and finish it (movegen, key, repetition, terminal).
// D = tree depth of the new position; path[0..D-1] are the edges above it.
__device__ SzPos wave_create_position(const BoardPtrs& bp, const SzPos& parent, int action, int chess960, const int* path, int D,
                                      int root_ply, u64* mask_lds) {
    int from, to, promo;
    sz_action_decode(parent, action, from, to, promo);
    SzPos X = sz_make_move(parent, from, to, promo, chess960);
    int n_legal, ep_legal; u64 checkers;
    wave_movegen(X, chess960, mask_lds, n_legal, ep_legal, checkers);
    X.key = sz_hash_key(X, ep_legal);
    int reps = wave_count_reps(bp, path, D, root_ply, X);
    X.meta = sz_finish_meta(X, checkers, n_legal, ep_legal, reps);
    return X;
}

// ------------------------------------------------------------------------------------------------
// kernel: start games (ChessTensor.start_board)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_new_games(View v, const int* scharnagl, const uint8_t* active) {
    extern __shared__ u64 lds64[];
    const int b = blockIdx.x;
    BoardPtrs bp = board_ptrs(v, b);
    if (active && !active[b]) return;
    int n = scharnagl ? scharnagl[b] : -1;
    SzPos X = sz_startpos(n);
    int n_legal, ep_legal; u64 checkers;
    wave_movegen(X, v.chess960, lds64 + LDS_HIST_WORDS, n_legal, ep_legal, checkers);
    X.key = sz_hash_key(X, ep_legal);
    X.meta = sz_finish_meta(X, checkers, n_legal, ep_legal, 0);
    if (lane_id() == 0) {
        bp.ring[0] = X;
        Ctl c = *bp.ctl;                                  // the cumulative counters (n_expand, n_term, sum_depth, sum_k, max_edges) survive a refill
        c.status = ST_ACTIVE; c.n_nodes = c.n_edges = c.sims_done = 0; c.pend_node = c.pend_depth = c.game_ply = c.err = 0; c.game_result = 0; c.reuse_ready = 0;
        *bp.ctl = c;
    }
}

__global__ void k_set_active(View v, const uint8_t* active) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= v.B) return;
    Ctl* c = v.ctl + b;
    int st = c->status & ~(ST_ACTIVE);
    if (active[b]) st |= ST_ACTIVE;
    c->status = st;
}

// network-batch rows for the boards that will search (active, game not over, no error), in board order: one workgroup, chunked scan.
// IN_SEARCH (sz_compact_searching): the boards that still search (searching, not done, no error) instead.
template <bool IN_SEARCH>
__device__ __forceinline__ bool compact_live(int st) {
    return IN_SEARCH ? ((st & ST_SEARCHING) && !(st & (ST_DONE | ST_ERROR))) : ((st & ST_ACTIVE) && !(st & (ST_GAMEOVER | ST_ERROR)));
}
template <bool IN_SEARCH>
__global__ __launch_bounds__(1024) void k_compact(View v, int* slot, int* n_live) {
    __shared__ int cnt[1024];
    const int t = threadIdx.x, per = (v.B + 1023) / 1024, lo = t * per, hi = min(v.B, lo + per);
    int c = 0;
    for (int b = lo; b < hi; b++) c += compact_live<IN_SEARCH>(v.ctl[b].status) ? 1 : 0;
    cnt[t] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                     // inclusive Hillis-Steele scan over the 1024 chunk counts
        int add = t >= off ? cnt[t - off] : 0;
        __syncthreads();
        cnt[t] += add;
        __syncthreads();
    }
    int base = cnt[t] - c;
    for (int b = lo; b < hi; b++) slot[b] = compact_live<IN_SEARCH>(v.ctl[b].status) ? base++ : -1;
    if (t == 1023) *n_live = cnt[1023];
}

// sz_compact_searching: move the pending network inputs of the boards that keep a row, `rows` rows of row_u4 uint4 each per board, from
// rows old_slot(b)*rows.. of `src` to rows new_slot(b)*rows.. of `dst`.  One workgroup per board.  It runs twice, caller's buffer -> the
// engine's staging buffer (to_stage: src rows by the old mapping) and back (src rows by the new one): a board's new row can be another live
// board's old row, so a copy in place would race.  Boards whose row does not change are left alone.
__global__ __launch_bounds__(256) void k_move_rows(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* old_slot, const int* new_slot, int rows,
                                                   int row_u4, int to_stage) {
    const int b = blockIdx.x;
    const int ns = new_slot[b];
    if (ns < 0) return;
    const int os = old_slot ? old_slot[b] : b;
    if (os < 0 || os == ns) return;
    const size_t n = (size_t)rows * row_u4;
    const uint4* s = src + (size_t)(to_stage ? os : ns) * n;
    uint4* d = dst + (size_t)ns * n;
    for (size_t i = threadIdx.x; i < n; i += 256) d[i] = s[i];
}

// sz_set_search_options changed leaves_per_step or the solver on a reuse_subtree engine: no board continues on its kept subtree (built without
// `complete` bits, or before the in-flight counts existed); the next search of every board starts from a fresh root
__global__ void k_drop_subtrees(View v) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < v.B) v.ctl[b].reuse_ready = 0;
}

// finish an uploaded game record (status only; the ring was copied by the host)
__global__ void k_after_upload(View v, int b, int ply) {
    Ctl* c = v.ctl + b;
    Ctl z = *c;                                           // cumulative counters kept, per-game fields reset
    z.status = ST_ACTIVE; z.n_nodes = z.n_edges = z.sims_done = 0; z.pend_node = z.pend_depth = z.err = 0; z.game_result = 0; z.game_ply = ply; z.reuse_ready = 0;
    *c = z;
}

// sz_set_endings' per-board state starts again with a game: the boards sz_new_games starts (board < 0; active == NULL: all), or the one board
// sz_upload_game fills.  Launched only while the array exists.
__global__ void k_reset_endings(EndState* st, const uint8_t* active, int B, int board) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (board >= 0 ? b != board : (active && !active[b])) return;
    EndState z; z.rs[0] = z.rs[1] = z.ds = 0; z.would_ply = -1; z.would_kind = z.would_colour = 0;
    st[b] = z;
}

// ------------------------------------------------------------------------------------------------
// kernel: search begin — create roots (mcts.py:43-46), root movegen + terminal test, encode root planes
// ------------------------------------------------------------------------------------------------
// VL: leaf batching on (sz_set_leaf_batching): the root is pending leaf 0 (leaf_ptrs), its network input goes to row slot(b)*L
// SOLVE: proven results on (sz_set_solver): a terminal root is labelled like any terminal position
// Both (sz_set_search_options) and either with reuse_subtree: the same code; a kept subtree carries its labels and has no descent in flight
// FO = ForcedOpts (sz_set_forced_playouts): the board's bit of fo.boards is latched into its status word beside ST_QUIET
template <bool VL, bool SOLVE, typename... FO>
__global__ __launch_bounds__(64) void k_search_begin(View v, void* planes, Batch vb, BeginOpts o, FO... fo) {
    constexpr bool FORCED = has_opt<ForcedOpts, FO...>;
    constexpr bool SPREAD = has_opt<SpreadOpts, FO...>;
    extern __shared__ u64 lds64[];
    u64* hist = lds64; u64* mask = lds64 + LDS_HIST_WORDS; int* path = (int*)(lds64 + LDS_HIST_WORDS + LDS_MASK_WORDS);
    const int b = blockIdx.x, lane = lane_id();
    BoardPtrs bp = board_ptrs(v, b);
    int status = uni(bp.ctl->status);
    if (v.rec_active && lane == 0) v.rec_active[b] = 0;
    if (o.goal && lane == 0) o.goal[b] = 0;                   // sz_set_visit_targets: a board that does not search makes no simulation
    if (!(status & ST_ACTIVE) || (status & (ST_GAMEOVER | ST_ERROR))) {
        if (lane == 0) bp.ctl->status = status & ~(ST_PENDING | ST_DONE | ST_SEARCHING);
        return;
    }
    if (v.slot && uni(v.slot[b]) < 0) {
        // the board became live after the last sz_compact: it has no row in the network batch.  Refuse loudly instead of searching nothing.
        if (lane == 0) { bp.ctl->status = (status & ~(ST_PENDING | ST_DONE | ST_SEARCHING)) | ST_ERROR; if (!bp.ctl->err) bp.ctl->err = SZ_ERR_STATE; }
        return;
    }
    const int root_ply = uni(bp.ctl->game_ply);
    const int qbit = (o.quiet && uni((int)o.quiet[b])) ? ST_QUIET : 0;
    int fbit = 0;
    if constexpr (FORCED) fbit = uni((int)opt_of<ForcedOpts>(fo...).boards[b]) ? ST_FORCED : 0;
    SzPos X = load_pos(bp.ring + (root_ply & (SZ_RING - 1)));
    path[0] = 0;
    if (v.reuse && uni(bp.ctl->reuse_ready) && uni(bp.ctl->n_nodes) <= v.S && 2 * (long long)uni(bp.ctl->n_edges) <= v.e_cap && v.S > 0) {
        // NON-REFERENCE option: the store already holds the subtree below the move just played (k_play compacted it to the front: edge 0 /
        // node 0 = that child, now the root, with its visit count and value sum).  The search continues on it: nothing to expand here, so
        // the board does not wait for the network; sz_search_begin's descent-only launch selects its first leaf.
        wave_load_history(bp, path, 0, root_ply, X, hist);
        __syncthreads();
        wave_encode(hist, X, nullptr, v.planes_dtype, v.rec_planes ? v.rec_planes + (size_t)b * SZ_NUM_PLANES * 8 : nullptr);   // training record of the root only
        // sz_set_visit_targets: the kept root's visits count towards the target; the search ends with root N = max(N_kept, 1 + t).  goal == 0: done here
        int goal = 1;
        if (o.target) { goal = uni(o.target[b]) + 1 - uni(bp.es[0].N); if (goal < 0) goal = 0; }
        // sz_set_search_root_noise: the kept root was expanded as an inner node, so its children hold the clean renormalised policy; mix them in place
        if (v.learning && v.root_gamma && !qbit) {
            const EdgeMeta rm = bp.em[0];
            wave_root_noise(bp.es + uni(rm.first), v.root_gamma + (size_t)b * SZ_MAX_MOVES, uni((int)rm.n));
        }
        if (lane == 0) {
            bp.npos[0] = X;
            Ctl* c = bp.ctl;
            if (o.target) o.goal[b] = goal;
            c->status = (status & ST_ACTIVE) | ST_SEARCHING | qbit | fbit | (goal == 0 ? ST_DONE : 0); c->sims_done = 0; c->pend_node = -1; c->pend_depth = 0; c->reuse_ready = 0;
            if constexpr (VL) c->n_pend = 0;                    // no root evaluation in flight: every in-flight count of the kept tree is 0, k[0] included
            if (v.rec_colour) v.rec_colour[b] = (uint8_t)szm_turn(X.meta);
        }
        return;
    }
    if (lane == 0) {
        bp.ctl->reuse_ready = 0;
        bp.npos[0] = X;
        EdgeStat s; s.W = 0.0; s.N = 1; s.P = 0.f;                 // root.visit_count = 1 (mcts.py:46)
        bp.es[0] = s;
        EdgeMeta m; m.first = -1; m.node = 0; m.n = 0; m.action = 0; m.term = (signed char)szm_term(X.meta);
        m.tval = (signed char)(szm_loss(X.meta) ? -1 : 0); m.pad = 0;
        if constexpr (SOLVE) { if (szm_term(X.meta)) m.pad = szm_loss(X.meta) ? PR_LOSS : PR_DRAW; }
        bp.em[0] = m;
        bp.gpath[0] = 0;
        if constexpr (SPREAD) opt_of<SpreadOpts>(fo...).Q[(size_t)b * v.e_cap] = 0.0;      // sz_set_lcb: the root edge is created
    }
    int st = (status & ST_ACTIVE) | ST_SEARCHING | qbit | fbit;
    const int budget = o.target ? uni(o.target[b]) : board_budget(v, b);     // a fresh root: the visit target is a budget
    if (o.target && lane == 0) o.goal[b] = budget;
    if (szm_term(X.meta) || budget <= 0) {
        // a terminal root: every simulation re-visits it (mcts.py:104-109); children stay empty
        if (lane == 0) {
            int S = budget > 0 ? budget : 0;
            double tv = szm_loss(X.meta) ? -1.0 : 0.0;
            bp.es[0].W = tv * (double)S; bp.es[0].N = 1 + S;
            if constexpr (SPREAD) opt_of<SpreadOpts>(fo...).Q[(size_t)b * v.e_cap] = (tv * tv) * (double)S;      // sz_set_lcb: the budget counted out at once
            Ctl* c = bp.ctl; c->status = st | ST_DONE; c->n_nodes = 1; c->n_edges = 1; c->sims_done = S;
            c->n_term += (unsigned long long)S; c->pend_node = -1; c->pend_depth = 0;
            if constexpr (VL) c->n_pend = 0;
        }
        return;
    }
    int n_legal, ep_legal; u64 checkers;
    wave_movegen(X, v.chess960, mask, n_legal, ep_legal, checkers);
    __syncthreads();
    const int row = v.slot ? uni(v.slot[b]) : b;              // network batch row of this board (compacted batches: live boards first)
    const LeafPtrs lf = leaf_ptrs<VL>(v, bp, vb, b, row, 0);  // the root is pending leaf 0
    for (int i = lane; i < SZ_MASK_WORDS; i += 64) lf.mask[i] = mask[i];
    wave_load_history(bp, path, 0, root_ply, X, hist);
    __syncthreads();
    wave_encode(hist, X, (planes && row >= 0) ? (char*)planes + lf.row * planes_board_bytes(v.planes_dtype) : nullptr, v.planes_dtype,
                v.rec_planes ? v.rec_planes + (size_t)b * SZ_NUM_PLANES * 8 : nullptr);
    if (lane == 0) {
        Ctl* c = bp.ctl;
        c->status = st | ST_PENDING; c->n_nodes = 1; c->n_edges = 1; c->sims_done = 0; c->pend_node = 0; c->pend_depth = 0;
        if (v.rec_colour) v.rec_colour[b] = (uint8_t)szm_turn(X.meta);
        if constexpr (VL) {
            c->n_pend = 1; *lf.depth = 0; lf.path[0] = 0;
            vb.vk[(size_t)b * v.e_cap] = 1;                     // the root's own evaluation is in flight
        }
    }
}


// ------------------------------------------------------------------------------------------------
// kernel: one lock-step iteration (expand + backprop of the evaluated leaf, then select / move /
// terminal test / encode of the next one)
// ------------------------------------------------------------------------------------------------
#define STEP_STAMP(k) do { if (v.dbg) { unsigned long long _t = __builtin_amdgcn_s_memtime(); if (lane_id() == 0) v.dbg[(size_t)blockIdx.x * 8 + (k)] = _t; } } while (0)
// VL = false: the reference's search, one leaf per board per step.  VL = true (sz_set_leaf_batching): every pending leaf is expanded and
// backed up in gather order (its k taken back along its path), then descents with virtual loss gather up to L new leaves; a terminal leaf
// is backed up on the spot, a descent that ends on a leaf already pending in this step (a collision) ends the gather.
// SOLVE = true (sz_set_solver): proven results are carried up the tree; a descent ends at the first proven node on its way.
// VL && SOLVE (sz_set_search_options): both at once; a proven stop puts nothing in flight and the gather goes on, a pending leaf is unknown.
// One body for the four: selection is wave_select_child<VL, SOLVE, FPU>, a pending leaf's path / mask / depth / network row come from
// leaf_ptrs<VL>; only the in-flight counts, n_pend, the collision break and "gather on" against "one leaf, stop" sit under if constexpr (VL).
// The options change the one selection site, in this order, and nothing else in the descent:
// FO has ForcedOpts (sz_set_forced_playouts): at depth 0 of a board with ST_FORCED wave_forced_child decides when it finds a forced child
// (without FpuOpts through wave_select_root_forced, which is that and the arg-max).
// FO has GumbelOpts (sz_set_gumbel, VL = SOLVE = false only, never with ForcedOpts): the selection at depth 0 is wave_select_root_gumbel, and the
// root's network value is kept when the root is expanded.
// FO = GumbelTreeOpts (sz_set_gumbel_tree, in GumbelOpts' place and alone): on top of that every expanded node's network value is kept by node
// id, and the selection at depth >= 1 is wave_select_tree_gumbel, which reads the parent's.
// FO has FpuOpts (sz_set_fpu): the arg-max that decides otherwise scores unvisited children by the site's first-play value, the root's at
// depth 0 and the tree's below.
// FO has PuctOpts (sz_set_cpuct, never with GumbelOpts): every selection reads puct_c at its parent's count in c_puct's place, the root's triple
// at depth 0 and the tree's below.
template <bool VL, bool SOLVE, typename... FO>
__global__ __launch_bounds__(64, 4) void k_search_step(View v, const float* __restrict__ policy, const float* __restrict__ value, void* planes, Batch vb, FO... fo) {
    constexpr bool FORCED = has_opt<ForcedOpts, FO...>;
    constexpr bool FPU = has_opt<FpuOpts, FO...>;
    constexpr bool GTREE = has_opt<GumbelTreeOpts, FO...>;
    constexpr bool GUMBEL = has_opt<GumbelOpts, FO...> || GTREE;
    static_assert(!GUMBEL || (!VL && !SOLVE && !FORCED), "sz_set_gumbel refuses leaf batching, the solver and forced playouts");
    static_assert(!GTREE || !FPU, "sz_set_gumbel_tree consults neither site of sz_set_fpu");
    constexpr bool PUCT = has_opt<PuctOpts, FO...>;
    static_assert(!GUMBEL || !PUCT, "sz_set_gumbel and sz_set_cpuct refuse each other");
    constexpr bool SPREAD = has_opt<SpreadOpts, FO...>;
    static_assert(!GUMBEL || !SPREAD, "sz_set_gumbel and sz_set_lcb refuse each other");
    extern __shared__ u64 lds64[];
    u64* hist = lds64; u64* mask = lds64 + LDS_HIST_WORDS; int* path = (int*)(lds64 + LDS_HIST_WORDS + LDS_MASK_WORDS);
    const int b = blockIdx.x, lane = lane_id();
    BoardPtrs bp = board_ptrs(v, b);
    int status = uni(bp.ctl->status);
    if (!(status & ST_SEARCHING) || (status & (ST_DONE | ST_ERROR))) return;
    int n_nodes = uni(bp.ctl->n_nodes), n_edges = uni(bp.ctl->n_edges), sims = uni(bp.ctl->sims_done);
    const int root_ply = uni(bp.ctl->game_ply);
    const int budget = board_budget(v, b);                    // this board's simulations (num_searches unless sz_set_search_budgets)
    const int row = v.slot ? uni(v.slot[b]) : b;              // network batch row of this board
    if (row < 0) return;
    if ((status & ST_PENDING) && !policy) return;             // descent-only launch (sz_search_begin with reuse): boards that already wait for the network sit it out
    unsigned long long n_expand = 0, n_term = 0, sum_depth = 0, sum_k = 0;
    unsigned long long n_stop = 0, n_proved = 0;                // solver: simulations ended on a proven non-terminal node, nodes proven by the update
    unsigned long long n_forced = 0;                            // forced playouts: root selections decided by a forced child
    unsigned long long n_gumbel = 0, n_fallback = 0;            // Gumbel: root selections made by the rule, of them over all children
    unsigned long long n_gtree = 0;                             // sz_set_gumbel_tree: selections below the root made by the rule
    int err = 0;
    STEP_STAMP(0);

    if (status & ST_PENDING) {
      const int n_leaves = VL ? uni(bp.ctl->n_pend) : 1;
      for (int li = 0;;) {                                              // VL = false: one pass, no loop
        // ---- mcts.py:77-109 for the leaf evaluated by the network (batched: every pending leaf, in gather order) -------------------
        const LeafPtrs lf = leaf_ptrs<VL>(v, bp, vb, b, row, li);
        const int d = uni(*lf.depth), node = VL ? 0 : uni(bp.ctl->pend_node);
        for (int j = lane; j <= d; j += 64) path[j] = lf.path[j];
        for (int i = lane; i < SZ_MASK_WORDS; i += 64) mask[i] = lf.mask[i];
        __syncthreads();
        const float* pol = policy + lf.row * SZ_NUM_ACTIONS;
            // masked sum in the fixed order: per-lane partial over planes ascending, then xor butterfly.
            // Only planes that hold a legal move are fetched (~20 of 73), and in groups of 16 INDEPENDENT loads: a load-wait-add chain per
            // plane cost one full memory latency each, and fetching all 73 planes made the kernel bandwidth-bound at 4096 boards.  The
            // value and action of every legal move are stashed in LDS in ascending action order, so the second half works on the K <= 218
            // children directly (lane = child: coalesced child records) instead of walking the planes again.
            const int path_alloc = v.p_cap > 256 ? v.p_cap : 256;
            float* sval = (float*)(path + path_alloc);                          // [<= 218] policy value of legal move c
            unsigned short* sact = (unsigned short*)(sval + 220);               // [<= 218] its action index
            u64 ne0 = __ballot(mask[lane] != 0);                                // planes 0..63 with at least one legal move
            u64 ne1 = __ballot(lane < SZ_MASK_WORDS - 64 && mask[64 + (lane < SZ_MASK_WORDS - 64 ? lane : 0)] != 0);   // planes 64..72
            constexpr int PCH = 16;
            float acc = 0.0f;
            int n_moves = 0;
            while (ne0 | ne1) {
                int pls[PCH];
    #pragma unroll
                for (int k = 0; k < PCH; k++) {                                  // next PCH non-empty planes, ascending (uniform)
                    int pl = -1;
                    if (ne0) { pl = __builtin_ctzll(ne0); ne0 &= ne0 - 1; }
                    else if (ne1) { pl = 64 + __builtin_ctzll(ne1); ne1 &= ne1 - 1; }
                    pls[k] = pl;
                }
                float pv[PCH];
    #pragma unroll
                for (int k = 0; k < PCH; k++) pv[k] = pol[(pls[k] >= 0 ? pls[k] : 0) * 64 + lane];     // issued back to back; plane 0 stands in for "none"
    #pragma unroll
                for (int k = 0; k < PCH; k++) {
                    const int pl = pls[k];
                    if (pl >= 0) {                                               // uniform
                        const bool mine = (mask[pl] >> lane) & 1;
                        if (mine) acc = acc + pv[k];
                        const u64 mm = __ballot(mine);
                        if (mine) {
                            const int r = n_moves + __popcll(mm & ((1ULL << lane) - 1));
                            sval[r] = pv[k];
                            sact[r] = (unsigned short)(pl * 64 + lane);
                        }
                        n_moves += __popcll(mm);
                    }
                }
            }
            const float total = wave_sum_butterfly(acc);
            __syncthreads();                                                     // one wave per workgroup: makes the LDS stash visible
            const int first = n_edges;
            int kept = 0;
            const int leaf_edge = path[d];
            for (int base = 0; base < n_moves; base += 64) {
                const int c = base + lane;
                const bool mine = c < n_moves;
                float p = 0.0f;
                if (mine) p = sval[c] / total;                                  // policy /= torch.sum(policy)
                const bool keep = mine && !(p == 0.0f);                         // policy.nonzero() (NaN stays)
                const u64 km = __ballot(keep);
                if (keep) {
                    if (v.learning && !v.root_gamma) p = (0.75f * p) + (0.25f * v.noise);   // (1-eps)*probs + eps*noise
                    const int slot = first + kept + __popcll(km & ((1ULL << lane) - 1));
                    if (slot < v.e_cap) {
                        EdgeStat s; s.W = 0.0; s.N = 0; s.P = p;
                        bp.es[slot] = s;
                        if constexpr (VL) vb.vk[(size_t)b * v.e_cap + slot] = 0;
                        if constexpr (SPREAD) opt_of<SpreadOpts>(fo...).Q[(size_t)b * v.e_cap + slot] = 0.0;
                        EdgeMeta m; m.first = -1; m.node = -1; m.n = 0; m.action = sact[c]; m.term = 0; m.tval = 0; m.pad = 0;
                        bp.em[slot] = m;
                    }
                }
                kept += __popcll(km);
            }
            if (first + kept > v.e_cap) { err = SZ_ERR_CAPACITY; kept = 0; }
            if (v.learning && v.root_gamma && d == 0 && kept > 0 && !(status & ST_QUIET)) {
                // non-reference option (sz_set_root_noise): AlphaZero's root-only noise.  The K Gamma(alpha,1) draws of this board,
                // normalised over its K children, are one Dirichlet(alpha) sample of dimension K; inner nodes keep their priors.
                // A quiet board (ST_QUIET, sz_set_search_root_noise) keeps its clean priors.
                __threadfence_block();                                      // the children were written by other lanes of this wave
                wave_root_noise(bp.es + first, v.root_gamma + (size_t)b * SZ_MAX_MOVES, kept);
            }
            if (lane == 0) {
                bp.em[leaf_edge].first = first; bp.em[leaf_edge].n = (unsigned short)kept;
                if constexpr (SOLVE) { if (!err && kept == n_moves) bp.em[leaf_edge].pad |= PR_COMPLETE; }     // no move was dropped for a zero prior
            }
            n_edges += kept;
            (void)node;
        const double val = (double)value[lf.row];                        // node.value = value.item()
        if constexpr (GUMBEL) { if (d == 0 && lane == 0) gumbel_of(fo...).vhat[b] = value[lf.row]; }     // sz_set_gumbel: the root's network value
        if constexpr (GTREE) {                                          // sz_set_gumbel_tree: every node's, read by selections later in this launch
            if (lane == 0 && node >= 0 && node < v.n_cap) opt_of<GumbelTreeOpts>(fo...).nval[(size_t)b * v.n_cap + node] = value[lf.row];
            __threadfence_block();
        }
        if constexpr (VL) {                                             // its descent is no longer in flight
            for (int j = lane; j <= d; j += 64) vb.vk[(size_t)b * v.e_cap + path[j]] -= 1;
        }
        if constexpr (SPREAD) wave_backprop(bp.es, opt_of<SpreadOpts>(fo...).Q + (size_t)b * v.e_cap, path, d, val);
        else wave_backprop(bp.es, path, d, val);
        sims++; n_expand++; sum_depth += d; sum_k += kept;
        if constexpr (!VL) break;
        __syncthreads();                                                // path, mask and stash in LDS are reused by the next leaf
        if (++li >= n_leaves) break;
      }
        status &= ~ST_PENDING;
    }
    STEP_STAMP(1);

    // ---- next simulation(s): mcts.py:49-64 ------------------------------------------------------
    int n_pend = 0;                                                     // batched: leaves gathered in this step
    int* vk = VL ? vb.vk + (size_t)b * v.e_cap : nullptr;
    while (sims + n_pend < budget && (!VL || n_pend < vb.L) && !err) {
        int d = 0, cur = 0;
        path[0] = 0;
        EdgeMeta m = bp.em[0];
        int parentN = bp.es[0].N;
        if constexpr (VL) parentN += vk[0];
        m.first = uni(m.first); int mn = uni((int)m.n); parentN = uni(parentN);
        int proven = PR_UNKNOWN;                                        // solver: result of the first proven node on the way, the root included
        if constexpr (SOLVE) proven = uni((int)m.pad & PR_MASK);
        while (mn > 0 && !proven) {                                     // Node.select
            int bi = -1;
            EdgeStat ps;                                                // sz_set_fpu: vp comes from the parent's own stored edge (cur; the root is edge 0)
            if constexpr (FPU) ps = bp.es[cur];
            float c_puct = v.c_puct;                                    // sz_set_cpuct: the rate at this parent's count, once per selection
            if constexpr (PUCT) c_puct = puct_c(opt_of<PuctOpts>(fo...).o, parentN, d == 0);
            // In order: a forced child of the root (sz_set_forced_playouts), else the Gumbel rule at the root (sz_set_gumbel), else the arg-max.
            // Without FPU the forced root keeps its own composition, wave_select_root_forced, and counts through `forced`: folded into the
            // sequence below, three of the four k_search_step<.., ForcedOpts> instantiations spill 8 to 24 bytes more per lane.
            bool forced = false;
            if constexpr (FORCED && FPU) {
                if (d == 0 && (status & ST_FORCED)) bi = wave_forced_child<VL, SOLVE>(bp.es + m.first, bp.em + m.first, vk + m.first, mn, parentN, opt_of<ForcedOpts>(fo...).k);
                n_forced += bi >= 0 ? 1 : 0;
            }
            if (GUMBEL && d == 0) {
                // sz_set_gumbel: only depth 0 changes.  One leaf per step and nothing in flight: sims - 1 root-child visits were made before this one
                if constexpr (GUMBEL) {
                    const GumbelOpts& go = gumbel_of(fo...);
                    bool fallback;
                    bi = wave_select_root_gumbel(bp.es + m.first, go.g ? go.g + (size_t)b * SZ_MAX_MOVES : nullptr, mn, sims - 1, budget, go.o, &fallback);
                    n_gumbel++; n_fallback += fallback ? 1 : 0;
                }
            } else if (GTREE) {
                // sz_set_gumbel_tree: completed-Q selection below the root, with the parent's own network value (a parent with children was expanded)
                if constexpr (GTREE) {
                    const GumbelTreeOpts& gt = opt_of<GumbelTreeOpts>(fo...);
                    const float vh = __int_as_float(uni(__float_as_int(gt.nval[(size_t)b * v.n_cap + uni(m.node)])));
                    bi = wave_select_tree_gumbel(bp.es + m.first, mn, gt.o, vh, nullptr, nullptr);
                    n_gtree++;
                }
            } else if (FORCED && !FPU && d == 0 && (status & ST_FORCED)) {
                if constexpr (FORCED)
                    bi = wave_select_root_forced<VL, SOLVE>(bp.es + m.first, bp.em + m.first, vk + m.first, mn, parentN, c_puct, vb.lam, opt_of<ForcedOpts>(fo...).k, &forced);
            } else if (bi < 0) {
                if constexpr (FPU) {
                    // sz_set_fpu: the root's mode and value at depth 0, the tree's below
                    const sz_fpu_options& fp = opt_of<FpuOpts>(fo...).o;
                    bi = wave_select_child<VL, SOLVE, true>(bp.es + m.first, bp.em + m.first, vk + m.first, mn, parentN, c_puct, vb.lam, d == 0 ? fp.root_mode : fp.tree_mode,
                                                            d == 0 ? fp.root_value : fp.tree_value, uni(ps.N), uni_f64(ps.W), nullptr);
                } else
                    bi = wave_select_child<VL, SOLVE, false>(bp.es + m.first, bp.em + m.first, vk + m.first, mn, parentN, c_puct, vb.lam, SZ_FPU_REFERENCE, 0.f, 0, 0.0, nullptr);
            }
            n_forced += forced ? 1 : 0;
            cur = m.first + bi;
            d++;
            if (d >= v.p_cap) { err = SZ_ERR_CAPACITY; break; }
            path[d] = cur;
            m = bp.em[cur];
            parentN = uni(bp.es[cur].N + (VL ? vk[cur] : 0));
            m.first = uni(m.first); mn = uni((int)m.n);
            if constexpr (SOLVE) proven = uni((int)m.pad & PR_MASK);
        }
        if (err) break;
        STEP_STAMP(2);
        if constexpr (SOLVE) {
            if (proven) {                                               // the simulation ends here with the proven value (terminal leaves included)
                if constexpr (SPREAD) wave_backprop(bp.es, opt_of<SpreadOpts>(fo...).Q + (size_t)b * v.e_cap, path, d, proven == PR_WIN ? 1.0 : (proven == PR_DRAW ? 0.0 : -1.0));
                else wave_backprop(bp.es, path, d, proven == PR_WIN ? 1.0 : (proven == PR_DRAW ? 0.0 : -1.0));
                sims++; n_term++; sum_depth += d;
                if (!uni((int)m.term)) n_stop++;
                continue;
            }
        }
        int node = uni(m.node);
        if (node >= 0) {
            if (VL && !uni((int)m.term) && m.first < 0) break;          // batched: a collision with a leaf pending in this step ends the gather
            // visited leaf without children: a terminal position (mcts.py:104-109)
            double tv = (double)(int)m.tval;
            if constexpr (SPREAD) wave_backprop(bp.es, opt_of<SpreadOpts>(fo...).Q + (size_t)b * v.e_cap, path, d, tv);
            else wave_backprop(bp.es, path, d, tv);
            sims++; n_term++; sum_depth += d;
            continue;
        }
        // first visit: node.game = deepcopy(parent.game); move_piece(action)   (mcts.py:57-59)
        if (n_nodes >= v.n_cap) { err = SZ_ERR_CAPACITY; break; }
        const int parent_node = uni(bp.em[path[d - 1]].node);
        SzPos P = load_pos(bp.npos + parent_node);
        SzPos X = wave_create_position(bp, P, (int)uni((int)m.action), v.chess960, path, d, root_ply, mask);
        STEP_STAMP(3);
        const int nid = n_nodes++;
        const int is_term = szm_term(X.meta);
        if (lane == 0) {
            bp.npos[nid] = X;
            EdgeMeta* em = bp.em + cur;
            em->node = nid; em->term = (signed char)is_term; em->tval = (signed char)(szm_loss(X.meta) ? -1 : 0);
            if constexpr (SOLVE) { if (is_term) em->pad = szm_loss(X.meta) ? PR_LOSS : PR_DRAW; }
        }
        __threadfence_block();
        if (is_term) {                                                  // get_value_and_terminated -> (0|-1, True)
            double tv = szm_loss(X.meta) ? -1.0 : 0.0;
            if constexpr (SPREAD) wave_backprop(bp.es, opt_of<SpreadOpts>(fo...).Q + (size_t)b * v.e_cap, path, d, tv);
            else wave_backprop(bp.es, path, d, tv);
            sims++; n_term++; sum_depth += d;
            if constexpr (SOLVE) n_proved += wave_solver_update(bp.em, path, d);
            continue;
        }
        // non-terminal leaf: hand it to the network as pending leaf n_pend (always 0 without batching)
        __syncthreads();
        const LeafPtrs lf = leaf_ptrs<VL>(v, bp, vb, b, row, n_pend);
        for (int i = lane; i < SZ_MASK_WORDS; i += 64) lf.mask[i] = mask[i];
        for (int j = lane; j <= d; j += 64) {
            lf.path[j] = path[j];
            if constexpr (VL) vk[path[j]] += 1;                         // batched: its descent goes in flight (k + 1 along its path)
        }
        if constexpr (VL) { if (lane == 0) *lf.depth = d; }
        wave_load_history(bp, path, d, root_ply, X, hist);
        __syncthreads();
        wave_encode(hist, X, (char*)planes + lf.row * planes_board_bytes(v.planes_dtype), v.planes_dtype, nullptr);
        status |= ST_PENDING;
        if constexpr (VL) {                                             // batched: the gather goes on
            __threadfence_block();
            __syncthreads();
            n_pend++;
            continue;
        }
        if (lane == 0) { bp.ctl->pend_node = nid; *lf.depth = d; }
        STEP_STAMP(4);
        break;
    }
    if (sims >= budget && !(status & ST_PENDING)) status |= ST_DONE;
    if (err) status |= ST_ERROR;
    if (lane == 0) {
        Ctl* c = bp.ctl;
        c->status = status; c->n_nodes = n_nodes; c->n_edges = n_edges; c->sims_done = sims;
        c->n_expand += n_expand; c->n_term += n_term; c->sum_depth += sum_depth; c->sum_k += sum_k;
        if (n_edges > c->max_edges) c->max_edges = n_edges;
        if (err && !c->err) c->err = err;
        if constexpr (VL) c->n_pend = n_pend;
        if constexpr (SOLVE) { v.sstat[(size_t)b * 2] += n_stop; v.sstat[(size_t)b * 2 + 1] += n_proved; }
        if constexpr (FORCED) opt_of<ForcedOpts>(fo...).stat[(size_t)b * 2] += n_forced;
        if constexpr (GUMBEL) { gumbel_of(fo...).stat[(size_t)b * 2] += n_gumbel; gumbel_of(fo...).stat[(size_t)b * 2 + 1] += n_fallback; }
        if constexpr (GTREE) opt_of<GumbelTreeOpts>(fo...).tstat[b] += n_gtree;
    }
}

// boards still waiting for the network (sz_pending_boards): one workgroup
__global__ __launch_bounds__(1024) void k_count_pending(View v, int* out) {
    __shared__ int tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    int c = 0;
    for (int b = threadIdx.x; b < v.B; b += 1024) c += (v.ctl[b].status & ST_PENDING) ? 1 : 0;
    if (c) atomicAdd(&tot, c);
    __syncthreads();
    if (threadIdx.x == 0) *out = tot;
}

// ------------------------------------------------------------------------------------------------
// kernel: root readout (mcts.py:113-122)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_root_children(View v, int* action, int* visits, int* n_child, float* prior, double* wsum) {
    const int b = blockIdx.x, lane = lane_id();
    BoardPtrs bp = board_ptrs(v, b);
    int status = bp.ctl->status;
    int n = 0, first = 0;
    if (status & ST_SEARCHING) { EdgeMeta m = bp.em[0]; n = m.n; first = m.first; }
    if (lane == 0) n_child[b] = n;
    for (int c = lane; c < SZ_MAX_CHILDREN; c += 64) {
        size_t o = (size_t)b * SZ_MAX_CHILDREN + c;
        if (c < n) {
            EdgeStat s = bp.es[first + c];
            action[o] = bp.em[first + c].action; visits[o] = s.N;
            if (prior) prior[o] = s.P;
            if (wsum) wsum[o] = s.W;
        } else {
            action[o] = -1; visits[o] = 0;
            if (prior) prior[o] = 0.f;
            if (wsum) wsum[o] = 0.0;
        }
    }
}

// proven results of the root and of its children in action order (sz_root_proven); all 0 on a board that has no search or no solver
__global__ __launch_bounds__(64) void k_root_proven(View v, int8_t* root, int8_t* child) {
    const int b = blockIdx.x, lane = lane_id();
    BoardPtrs bp = board_ptrs(v, b);
    int n = 0, first = 0, r = 0;
    if (bp.ctl->status & ST_SEARCHING) { EdgeMeta m = bp.em[0]; n = m.n; first = m.first; r = m.pad & PR_MASK; }
    if (lane == 0) root[b] = (int8_t)r;
    for (int c = lane; c < SZ_MAX_CHILDREN; c += 64)
        child[(size_t)b * SZ_MAX_CHILDREN + c] = (int8_t)(c < n ? (bp.em[first + c].pad & PR_MASK) : 0);
}

// ------------------------------------------------------------------------------------------------
// NON-REFERENCE option (sz_config.reuse_subtree): re-root the board's tree at edge e_c, a child of the root, in place.  What k_play does
// with the move it chose and k_play_moves with the move it was given.  reuse_ready is set when a subtree was kept and left as it is
// otherwise (never visited, or a leaf: nothing to keep): it is 0 on entry (k_search_begin's, or k_play_moves' own write).
// ------------------------------------------------------------------------------------------------
__device__ void wave_keep_subtree(const View& v, const BoardPtrs& bp, int b, int e_c) {
    const int lane = lane_id();
    // Spans are bump-allocated in node-creation order and a node is created after its parent, so walking the nodes in id order visits the kept
    // spans in ascending address order: every span moves DOWN (destination <= source), in place, no second buffer.  nmap[nid] = new index of the
    // edge that owns node nid (-1 = not in the kept subtree); the chosen child becomes edge 0 / node 0.
    const int n_nodes = uni(bp.ctl->n_nodes);
    const EdgeMeta cm = bp.em[e_c];
    const int nid_c = uni(cm.node), n_c = uni((int)cm.n);
    if (nid_c < 0 || n_c == 0) return;                               // never visited, or a leaf: nothing to keep (reuse_ready stays 0)
    int* nmap = v.nmap + (size_t)b * v.n_cap;
    for (int i = lane; i < n_nodes; i += 64) nmap[i] = -1;
    const EdgeStat cs = bp.es[e_c];
    __threadfence_block();
    if (lane == 0) { bp.es[0] = cs; bp.em[0] = cm; nmap[nid_c] = 0; }
    __threadfence_block();
    int cursor = 1, new_nid = 0;
    for (int nid = nid_c; nid < n_nodes; nid++) {
        const int e_new = uni(nmap[nid]);
        if (e_new < 0) continue;
        EdgeMeta m = bp.em[e_new];                                   // already moved; `first` still points at the old span, which no copy has reached yet
        const int ofirst = uni(m.first), on = uni((int)m.n);
        for (int base = 0; base < on; base += 64) {
            const int k = base + lane;
            EdgeStat s2; EdgeMeta m2;
            if (k < on) { s2 = bp.es[ofirst + k]; m2 = bp.em[ofirst + k]; }
            __threadfence_block();
            if (k < on) {
                bp.es[cursor + k] = s2; bp.em[cursor + k] = m2;
                if (m2.node >= 0) nmap[m2.node] = cursor + k;
            }
            __threadfence_block();
        }
        if (lane == 0) {
            SzPos pz = bp.npos[nid];
            bp.npos[new_nid] = pz;
            bp.em[e_new].first = on > 0 ? cursor : -1;
            bp.em[e_new].node = new_nid;
        }
        __threadfence_block();
        cursor += on;
        new_nid++;
    }
    if (lane == 0) { Ctl* c = bp.ctl; c->n_nodes = new_nid; c->n_edges = cursor; c->reuse_ready = 1; }
}

// ------------------------------------------------------------------------------------------------
// kernel: sample + play (sim.py:63-76) and game-over test (sim.py:46, 86-97)
// ------------------------------------------------------------------------------------------------
// SOLVE (sz_set_solver): on a root proven WIN the move played is the first child proven LOSS, whatever the uniform
// FO = ForcedOpts (sz_set_forced_playouts): on a board with ST_FORCED the record and the move choice use the pruned counts of wave_prune; the
// tree, and with it the subtree kept below, keeps the counted visits
// FO ends in EndOpts (sz_set_endings): wave_ending decides on the counted visits whether the game ends here instead of a move
// FO = GumbelOpts (sz_set_gumbel, SOLVE = false only): the move is wave_gumbel_play's, the board's uniform is not read, and the improved policy,
// v_mix and the root's network value are left for sz_fetch_gumbel; the record keeps the counted visits
// FO holds TempOpts (sz_set_move_temperature): the move is wave_temperature's, from the counts the sampling reads (pruned on a forced board), after
// the ending decision; the record and the subtree kept are untouched
// FO holds PuctOpts (sz_set_cpuct, only beside ForcedOpts): wave_prune reads the root triple's c at the root's counted N in c_puct's place
template <bool SOLVE, typename... FO>
__global__ __launch_bounds__(64) void k_play(View v, const double* uniforms, FO... fo) {
    constexpr bool FORCED = has_opt<ForcedOpts, FO...>;
    constexpr bool ENDING = has_opt<EndOpts, FO...>;
    constexpr bool GUMBEL = has_opt<GumbelOpts, FO...>;
    constexpr bool TEMP = has_opt<TempOpts, FO...>;
    constexpr bool PUCT = has_opt<PuctOpts, FO...>;
    static_assert(!PUCT || (FORCED && !GUMBEL), "policy-target pruning is k_play's only use of the exploration rate");
    static_assert(!GUMBEL || (!SOLVE && !FORCED && !ENDING && !TEMP), "sz_set_gumbel refuses the solver, forced playouts, endings and the move temperature");
    constexpr bool LCB = has_opt<LcbOpts, FO...>;
    static_assert(!GUMBEL || !LCB, "sz_set_gumbel and sz_set_lcb refuse each other");
    extern __shared__ u64 lds64[];
    u64* mask = lds64 + LDS_HIST_WORDS; int* path = (int*)(lds64 + LDS_HIST_WORDS + LDS_MASK_WORDS);
    int* vis_lds = path + 8;
    const int b = blockIdx.x, lane = lane_id();
    BoardPtrs bp = board_ptrs(v, b);
    int status = uni(bp.ctl->status);
    if constexpr (ENDING) {                                              // a board that does not play in this sz_play: kind 0, m NaN
        if (lane == 0) { opt_of<EndOpts>(fo...).kind[b] = SZ_END_NONE; opt_of<EndOpts>(fo...).mval[b] = __longlong_as_double(0x7ff8000000000000LL); }
    }
    if constexpr (TEMP) {                                                // likewise: no eligible child, p NaN
        if (lane == 0) { opt_of<TempOpts>(fo...).nelig[b] = 0; opt_of<TempOpts>(fo...).pch[b] = __longlong_as_double(0x7ff8000000000000LL); }
    }
    if constexpr (LCB) {                                                 // likewise: no move, no c*, no bound, no candidate, not decided
        if (lane == 0) {
            const LcbOpts& lo = opt_of<LcbOpts>(fo...);
            lo.move[b] = -1; lo.cstar[b] = -1; lo.lcb2[(size_t)b * 2] = sz_lcb_nan(); lo.lcb2[(size_t)b * 2 + 1] = sz_lcb_nan(); lo.ncand[b] = 0; lo.decided[b] = 0;
        }
    }
    if (!(status & ST_SEARCHING) || !(status & ST_DONE) || (status & (ST_ERROR | ST_GAMEOVER))) return;
    EdgeMeta rm = bp.em[0];
    const int n = uni((int)rm.n), first = uni(rm.first);
    const int root_ply = uni(bp.ctl->game_ply);
    int total = 0;
    for (int c = lane; c < SZ_MAX_CHILDREN; c += 64) {
        int nv = 0, act = -1;
        if (c < n) { nv = bp.es[first + c].N; act = bp.em[first + c].action; }
        vis_lds[c] = nv;
        total += nv;
        if (v.rec_action) { v.rec_action[(size_t)b * SZ_MAX_CHILDREN + c] = act; v.rec_visits[(size_t)b * SZ_MAX_CHILDREN + c] = nv; }
    }
    for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off);
    __syncthreads();
    if (n == 0 || total == 0) {                                          // ZeroDivisionError in the reference (mcts.py:118-120)
        if (lane == 0) { bp.ctl->status = status | ST_ERROR; if (!bp.ctl->err) bp.ctl->err = SZ_ERR_ZERO_VISITS; }
        return;
    }
    int end_kind = SZ_END_NONE, end_result = 0;
    if constexpr (ENDING) {                                              // on the counted visits, before any pruning
        const EndOpts& eo = opt_of<EndOpts>(fo...);
        int code = PR_UNKNOWN;
        if constexpr (SOLVE) code = rm.pad & PR_MASK;
        const int colour = uni((int)szm_turn(bp.npos[0].meta));
        EndState st = eo.state[b];
        double m; bool marked;
        end_kind = wave_ending(bp.es + first, n, code, colour, root_ply, st, eo.o, uni((int)eo.holdout[b]) != 0, &m, &marked);
        end_result = ending_result(end_kind, code, colour);
        if (lane == 0) {
            eo.state[b] = st; eo.kind[b] = (uint8_t)end_kind; eo.mval[b] = m;
            if (end_kind != SZ_END_NONE) eo.stat[(size_t)b * 4 + end_kind - 1] += 1;
            if (marked) eo.stat[(size_t)b * 4 + 3] += 1;
        }
    }
    if constexpr (FORCED) {
        if (status & ST_FORCED) {                                        // the zero-visit check above stays on the counted visits
            int cut;
            if constexpr (PUCT) {                                        // sz_set_cpuct: the root triple's rate at the root's counted N
                const int rootN = uni(bp.es[0].N);
                cut = wave_prune(bp.es + first, n, rootN, puct_c(opt_of<PuctOpts>(fo...).o, rootN, true), opt_of<ForcedOpts>(fo...).k, vis_lds, nullptr);
            } else
                cut = wave_prune(bp.es + first, n, uni(bp.es[0].N), v.c_puct, opt_of<ForcedOpts>(fo...).k, vis_lds, nullptr);
            __syncthreads();
            total -= cut;
            if (v.rec_action) for (int c = lane; c < n; c += 64) v.rec_visits[(size_t)b * SZ_MAX_CHILDREN + c] = vis_lds[c];
            if (lane == 0) opt_of<ForcedOpts>(fo...).stat[(size_t)b * 2 + 1] += (unsigned long long)cut;
        }
    }
    if constexpr (ENDING) {
        if (end_kind != SZ_END_NONE) {                                   // the game ends instead of a move: ring, game_ply and the root stay, no subtree is kept,
            if (lane == 0) {                                             // the board's uniform is not read
                Ctl* c = bp.ctl;
                c->status = (status & ST_ACTIVE) | ST_GAMEOVER;
                c->game_result = end_result;
                if (v.rec_nchild) { v.rec_nchild[b] = n; v.rec_chosen[b] = -1; v.rec_over[b] = 1; v.rec_result[b] = (int8_t)end_result; v.rec_active[b] = 1; }
            }
            return;
        }
    }
    // np.random.choice: cdf = cumsum(p); cdf /= cdf[-1]; idx = searchsorted(cdf, u, 'right')   (sequential f64, like numpy)
    int chosen = 0;
    int temp_kind = TEMP_SAMPLED;                                        // sz_set_lcb reads how wave_temperature came to its move
    if constexpr (GUMBEL) {
        const GumbelOpts& go = opt_of<GumbelOpts>(fo...);
        chosen = wave_gumbel_play(bp.es + first, go.g ? go.g + (size_t)b * SZ_MAX_MOVES : nullptr, n, go.o, go.vhat[b], go.work + (size_t)b * SZ_MAX_MOVES,
                                  go.policy + (size_t)b * SZ_MAX_MOVES, go.vmix + b);
    } else if constexpr (TEMP) {
        const TempOpts& to = opt_of<TempOpts>(fo...);
        int pmove = -1;
        if constexpr (SOLVE) {
            if (uni((int)rm.pad & PR_MASK) == PR_WIN) {                  // the proving move, whatever T is: the first child proven LOSS
                int fi = 0x7fffffff;
                for (int c = lane; c < n && fi == 0x7fffffff; c += 64) if ((bp.em[first + c].pad & PR_MASK) == PR_LOSS) fi = c;
                for (int off = 32; off >= 1; off >>= 1) { const int oi = __shfl_xor(fi, off); if (oi < fi) fi = oi; }
                fi = uni(fi);
                if (fi != 0x7fffffff) pmove = fi;
            }
        }
        int kind, ne, ex; double p;
        chosen = wave_temperature(bp.es + first, vis_lds, n, to.o, uni_f64(to.temps[b]), uni_f64(uniforms[b]), pmove, to.work + (size_t)b * SZ_MAX_MOVES,
                                  &kind, &ne, &p, &ex);
        temp_kind = kind;
        if (lane == 0) {
            to.nelig[b] = ne; to.pch[b] = p;
            to.stat[(size_t)b * 3 + (kind == TEMP_SAMPLED ? 0 : 1)] += 1;
            to.stat[(size_t)b * 3 + 2] += (unsigned long long)ex;
        }
    } else
    if (lane == 0) {
        const double u = uniforms[b];
        double acc = 0.0;
        for (int c = 0; c < n; c++) acc += (double)vis_lds[c] / (double)total;
        const double last = acc;
        acc = 0.0;
        int idx = 0;
        for (int c = 0; c < n; c++) { acc += (double)vis_lds[c] / (double)total; if (acc / last <= u) idx = c + 1; }
        if (idx >= n) idx = n - 1;
        if (u < 0.0) {                                                  // greedy: max(action_probs, key=...) of eval.py:92-94 — first maximum
            idx = 0;
            for (int c = 1; c < n; c++) if (vis_lds[c] > vis_lds[idx]) idx = c;
        }
        if constexpr (SOLVE) {
            if ((rm.pad & PR_MASK) == PR_WIN)
                for (int c = 0; c < n; c++) if ((bp.em[first + c].pad & PR_MASK) == PR_LOSS) { idx = c; break; }
        }
        chosen = idx;
    }
    chosen = uni(chosen);
    if constexpr (LCB) {
        // sz_set_lcb: where the move above is "the most visited one" (the negative uniform without the temperature option, wave_temperature's
        // greedy kind with it; never the proving move of a root proven WIN) the rule's move takes its place, unless the option only observes
        const LcbOpts& lo = opt_of<LcbOpts>(fo...);
        int cs, ncand, nbad; double lcb_move, lcb_star;
        const int mv = wave_lcb(bp.es + first, lo.Q + (size_t)b * v.e_cap + first, vis_lds, n, lo.o, nullptr, &cs, &lcb_move, &lcb_star, &ncand, &nbad);
        bool greedy;
        if constexpr (TEMP) greedy = temp_kind == TEMP_GREEDY;
        else {
            greedy = uni_f64(uniforms[b]) < 0.0;
            if constexpr (SOLVE) { if (uni((int)rm.pad & PR_MASK) == PR_WIN) greedy = false; }
        }
        const bool decided = greedy && lo.o.select != 0;
        if (decided) chosen = mv;
        if (lane == 0) {
            lo.move[b] = mv; lo.cstar[b] = cs; lo.lcb2[(size_t)b * 2] = lcb_move; lo.lcb2[(size_t)b * 2 + 1] = lcb_star; lo.ncand[b] = ncand; lo.decided[b] = decided ? 1 : 0;
            lo.stat[(size_t)b * 3] += decided ? 1 : 0;
            lo.stat[(size_t)b * 3 + 1] += mv != cs ? 1 : 0;
            lo.stat[(size_t)b * 3 + 2] += (unsigned long long)nbad;
        }
    }
    const int action = uni((int)bp.em[first + chosen].action);
    SzPos R = load_pos(bp.npos);
    path[0] = 0;
    SzPos X = wave_create_position(bp, R, action, v.chess960, path, 1, root_ply, mask);
    const int over = szm_term(X.meta);
    int result = 0;
    if (over && szm_loss(X.meta)) result = szm_turn(X.meta) ? -1 : 1;      // side to move is mated
    if (lane == 0) {
        bp.ring[(root_ply + 1) & (SZ_RING - 1)] = X;
        Ctl* c = bp.ctl;
        c->game_ply = root_ply + 1;
        c->status = (status & ST_ACTIVE) | (over ? ST_GAMEOVER : 0);
        c->game_result = result;
        if (v.rec_nchild) { v.rec_nchild[b] = n; v.rec_chosen[b] = action; v.rec_over[b] = (uint8_t)over; v.rec_result[b] = (int8_t)result; v.rec_active[b] = 1; }
    }
    if (!v.reuse || over) return;
    // ---- NON-REFERENCE option: keep the subtree of the move just played (the reference builds a fresh tree per ply, sim.py:53) ------------
    __syncthreads();
    wave_keep_subtree(v, bp, b, first + chosen);
}

// ------------------------------------------------------------------------------------------------
// kernel: play a GIVEN move (sz_play_moves): an opponent engine's, a book's, a person's.  One wave per board, no option state read.
// ------------------------------------------------------------------------------------------------
// The root position is the ring entry of the game's ply (as k_search_begin takes it; npos[0] is the root only right after a search).  Legality
// is the action's bit in wave_movegen's mask, never a look-up among the root's children: expansion drops legal moves whose renormalised prior
// is exactly 0.  The move itself is what k_play does after its choice; the record says the board played no search move (rec_active = 0) and
// still reports the game's end.  With reuse_subtree the board's tree (a finished search's, or the one an earlier sz_play / sz_play_moves kept)
// is re-rooted at the given move by wave_keep_subtree, so sz_play followed by sz_play_moves keeps the grandchild's subtree.
__global__ __launch_bounds__(64) void k_play_moves(View v, const int* actions) {
    extern __shared__ u64 lds64[];
    u64* mask = lds64 + LDS_HIST_WORDS; int* path = (int*)(lds64 + LDS_HIST_WORDS + LDS_MASK_WORDS);
    const int b = blockIdx.x, lane = lane_id();
    const int action = uni(actions[b]);
    if (action < 0) return;                                              // -1: the board is left alone, its record and kept subtree included
    BoardPtrs bp = board_ptrs(v, b);
    const int status = uni(bp.ctl->status);
    if (status & (ST_ERROR | ST_GAMEOVER)) return;
    if ((status & ST_SEARCHING) && !(status & ST_DONE)) {                // inside an unfinished search: refused loudly, like a board without a row
        if (lane == 0) { bp.ctl->status = status | ST_ERROR; if (!bp.ctl->err) bp.ctl->err = SZ_ERR_STATE; }
        return;
    }
    const int root_ply = uni(bp.ctl->game_ply);
    const SzPos R = load_pos(bp.ring + (root_ply & (SZ_RING - 1)));
    int legal = 0;
    if (action < SZ_ACTIONS) {
        int n_legal, ep_legal; u64 checkers;
        wave_movegen(R, v.chess960, mask, n_legal, ep_legal, checkers);
        __syncthreads();
        legal = (int)((mask[action >> 6] >> (action & 63)) & 1);
        __syncthreads();                                                 // wave_create_position fills the same mask words
    }
    if (!uni(legal)) {                                                   // ValueError("Invalid move"), chess_tensor.py:91-92
        if (lane == 0) { bp.ctl->status = status | ST_ERROR; if (!bp.ctl->err) bp.ctl->err = SZ_ERR_INVALID; }
        return;
    }
    // the new position at depth 0 of a tree rooted one ply on: every ancestor is a ring entry, the root's included, so no tree is read
    path[0] = 0;
    SzPos X = wave_create_position(bp, R, action, v.chess960, path, 0, root_ply + 1, mask);
    const int over = szm_term(X.meta);
    int result = 0;
    if (over && szm_loss(X.meta)) result = szm_turn(X.meta) ? -1 : 1;      // side to move is mated
    const bool tree = ((status & ST_SEARCHING) && (status & ST_DONE)) || uni(bp.ctl->reuse_ready) != 0;
    if (lane == 0) {
        bp.ring[(root_ply + 1) & (SZ_RING - 1)] = X;
        Ctl* c = bp.ctl;
        c->game_ply = root_ply + 1;
        c->status = (status & ST_ACTIVE) | (over ? ST_GAMEOVER : 0);
        c->game_result = result;
        c->reuse_ready = 0;
        if (v.rec_nchild) { v.rec_chosen[b] = action; v.rec_over[b] = (uint8_t)over; v.rec_result[b] = (int8_t)result; v.rec_active[b] = 0; }
    }
    if (!v.reuse || over || !tree) return;
    __syncthreads();
    const EdgeMeta rm = bp.em[0];
    const int n = uni((int)rm.n), first = uni(rm.first);
    u64 hit = 0;
    int at = -1;
    for (int base = 0; base < n && at < 0; base += 64) {                 // the root child with this action; none: a move expansion dropped
        const int c = base + lane;
        hit = __ballot(c < n && (int)bp.em[first + c].action == action);
        if (hit) at = base + __builtin_ctzll(hit);
    }
    if (at < 0) return;
    wave_keep_subtree(v, bp, b, first + at);
}

// ------------------------------------------------------------------------------------------------
// test hook (sz_debug_select): the device's Node.select / get_ucb on caller-supplied children, one wave per case
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_debug_select(const int* offsets, const int* vc, const double* wsum, const float* prior,
                                                     const int* parent_visits, const float* c_puct, float* ucb_out, int* argmax_out) {
    extern __shared__ u64 lds64[];
    EdgeStat* ch = (EdgeStat*)lds64;                       // the case's children staged as the SoA records the search reads
    const int cs = blockIdx.x, lo = offsets[cs], n = offsets[cs + 1] - lo;
    if (n <= 0 || n > SZ_MAX_CHILDREN) { if (lane_id() == 0) argmax_out[cs] = -1; return; }
    for (int c = lane_id(); c < n; c += 64) { EdgeStat s; s.W = wsum[lo + c]; s.N = vc[lo + c]; s.P = prior[lo + c]; ch[c] = s; }
    __syncthreads();
    const int bi = wave_select_child<false, false, false>(ch, nullptr, nullptr, n, parent_visits[cs], c_puct[cs], 0.f, SZ_FPU_REFERENCE, 0.f, 0, 0.0, ucb_out + lo);
    if (lane_id() == 0) argmax_out[cs] = bi;
}

// the children [lo, lo + n) of a hook's case staged as the records the search reads, for the hooks whose cases carry in-flight counts and proven
// codes (proven == NULL: none): ch, cm and kk hold SZ_MAX_CHILDREN entries each, in this order, from the start of the LDS
__device__ __forceinline__ void stage_case(int lo, int n, const int* vc, const int* inflight, const double* wsum, const float* prior, const int8_t* proven,
                                           EdgeStat* ch, EdgeMeta* cm, int* kk) {
    for (int c = lane_id(); c < n; c += 64) {
        EdgeStat s; s.W = wsum[lo + c]; s.N = vc[lo + c]; s.P = prior[lo + c]; ch[c] = s;
        EdgeMeta m; m.first = -1; m.node = -1; m.n = 0; m.action = 0; m.term = 0; m.tval = 0; m.pad = (unsigned short)(proven ? (proven[lo + c] & PR_MASK) : 0); cm[c] = m;
        kk[c] = inflight[lo + c];
    }
}

// test hook (sz_debug_forced): wave_select_root_forced and wave_prune, the functions k_search_step<.., ForcedOpts> and k_play<.., ForcedOpts> call, on
// caller-supplied children, one wave per case.  proven == NULL: the instantiations without the solver
__global__ __launch_bounds__(64) void k_debug_forced(const int* offsets, const int* vc, const int* inflight, const double* wsum, const float* prior,
                                                     const int8_t* proven, const int* parent_visits, const float* c_puct, const float* fk, float lam,
                                                     int* selected_out, int* forced_out, int* pruned_out, int* cstar_out) {
    extern __shared__ u64 lds64[];
    EdgeStat* ch = (EdgeStat*)lds64;
    EdgeMeta* cm = (EdgeMeta*)(ch + SZ_MAX_CHILDREN);
    int* kk = (int*)(cm + SZ_MAX_CHILDREN);
    int* vis = kk + SZ_MAX_CHILDREN;
    const int cs = blockIdx.x, lo = offsets[cs], n = offsets[cs + 1] - lo, lane = lane_id();
    if (n <= 0 || n > SZ_MAX_CHILDREN) { if (lane == 0) { selected_out[cs] = -1; forced_out[cs] = 0; cstar_out[cs] = -1; } return; }
    stage_case(lo, n, vc, inflight, wsum, prior, proven, ch, cm, kk);
    for (int c = lane; c < n; c += 64) vis[c] = vc[lo + c];
    __syncthreads();
    const int pv = parent_visits[cs];
    bool forced;
    const int bi = proven ? wave_select_root_forced<true, true>(ch, cm, kk, n, pv, c_puct[cs], lam, fk[cs], &forced)
                          : wave_select_root_forced<true, false>(ch, cm, kk, n, pv, c_puct[cs], lam, fk[cs], &forced);
    if (lane == 0) { selected_out[cs] = bi; forced_out[cs] = forced ? 1 : 0; }
    wave_prune(ch, n, pv, c_puct[cs], fk[cs], vis, cstar_out + cs);       // the case read as a finished search: the parent count is the root's N
    __syncthreads();
    for (int c = lane; c < n; c += 64) pruned_out[lo + c] = vis[c];
}

// test hook (sz_debug_select_fpu): wave_select_child<.., true>, the function k_search_step<.., FpuOpts> calls, on caller-supplied children, one wave per
// case.  proven == NULL: the instantiations without the solver
__global__ __launch_bounds__(64) void k_debug_select_fpu(const int* offsets, const int* vc, const int* inflight, const double* wsum, const float* prior,
                                                         const int8_t* proven, const int* parent_visits, const int* parent_n, const double* parent_w,
                                                         const float* c_puct, const int* is_root, const sz_fpu_options* opts, float lam, float* ucb_out, int* selected_out) {
    extern __shared__ u64 lds64[];
    EdgeStat* ch = (EdgeStat*)lds64;
    EdgeMeta* cm = (EdgeMeta*)(ch + SZ_MAX_CHILDREN);
    int* kk = (int*)(cm + SZ_MAX_CHILDREN);
    const int cs = blockIdx.x, lo = offsets[cs], n = offsets[cs + 1] - lo, lane = lane_id();
    if (n <= 0 || n > SZ_MAX_CHILDREN) { if (lane == 0) selected_out[cs] = -1; return; }
    stage_case(lo, n, vc, inflight, wsum, prior, proven, ch, cm, kk);
    __syncthreads();
    const sz_fpu_options o = opts[cs];
    const int root = uni(is_root[cs]);
    const int mode = uni(root ? o.root_mode : o.tree_mode);
    const float value = root ? o.root_value : o.tree_value;
    const int bi = proven ? wave_select_child<true, true, true>(ch, cm, kk, n, parent_visits[cs], c_puct[cs], lam, mode, value, uni(parent_n[cs]), uni_f64(parent_w[cs]), ucb_out + lo)
                          : wave_select_child<true, false, true>(ch, cm, kk, n, parent_visits[cs], c_puct[cs], lam, mode, value, uni(parent_n[cs]), uni_f64(parent_w[cs]), ucb_out + lo);
    if (lane == 0) selected_out[cs] = bi;
}

// test hook (sz_debug_gumbel): the device functions of sz_set_gumbel on caller-supplied cases, one wave per case.  Three parts, each skipped
// when its first array is NULL: sz_slog / sz_sexp of x[cs]; sz_gumbel_level of tnm[cs] = (t, n, m_eff); wave_select_root_gumbel and
// wave_gumbel_play, the functions k_search_step<.., GumbelOpts> and k_play<.., GumbelOpts> call, on the case's children
__global__ __launch_bounds__(64) void k_debug_gumbel(const double* x, double* slog_out, double* sexp_out, const int* tnm, int* level_out,
                                                     const int* offsets, const int* vc, const double* wsum, const float* prior, const double* g,
                                                     const int* visit, const int* goal, const float* vhat, const sz_gumbel_options* opts,
                                                     int* selected_out, int* fallback_out, int* final_out, float* policy_out, double* vmix_out) {
    extern __shared__ u64 lds64[];
    EdgeStat* ch = (EdgeStat*)lds64;
    double* work = (double*)(ch + SZ_MAX_CHILDREN);
    float* pol = (float*)(work + SZ_MAX_CHILDREN);
    const int cs = blockIdx.x, lane = lane_id();
    if (x && lane == 0) { slog_out[cs] = sz_slog(x[cs]); sexp_out[cs] = sz_sexp(x[cs]); }
    if (tnm && lane == 0) {
        const int t = tnm[cs * 3], n = tnm[cs * 3 + 1], m = tnm[cs * 3 + 2];
        level_out[cs] = (t >= 0 && t < n && m >= 1) ? sz_gumbel_level(t, n, m) : -1;           // the rule knows visits 0..n-1 only
    }
    if (!offsets) return;
    const int lo = offsets[cs], n = offsets[cs + 1] - lo;
    const int t = uni(visit[cs]), gl = uni(goal[cs]);
    const sz_gumbel_options o = opts[cs];
    if (n <= 0 || n > SZ_MAX_CHILDREN || t < 0 || t >= gl - 1 || o.max_considered < 1) { if (lane == 0) { selected_out[cs] = -1; fallback_out[cs] = 0; final_out[cs] = -1; } return; }
    for (int c = lane; c < n; c += 64) { EdgeStat s; s.W = wsum[lo + c]; s.N = vc[lo + c]; s.P = prior[lo + c]; ch[c] = s; }
    __syncthreads();
    bool fallback;
    const int bi = wave_select_root_gumbel(ch, g ? g + lo : nullptr, n, t, gl, o, &fallback);
    double vmix;
    const int mv = wave_gumbel_play(ch, g ? g + lo : nullptr, n, o, vhat[cs], work, pol, &vmix);
    __syncthreads();
    for (int c = lane; c < n; c += 64) policy_out[lo + c] = pol[c];
    if (lane == 0) { selected_out[cs] = bi; fallback_out[cs] = fallback ? 1 : 0; final_out[cs] = mv; vmix_out[cs] = vmix; }
}

// test hook (sz_debug_gumbel_tree): wave_select_tree_gumbel, the function k_search_step<.., GumbelTreeOpts> calls, on caller-supplied cases, one
// wave per case
__global__ __launch_bounds__(64) void k_debug_gumbel_tree(const int* offsets, const int* vc, const double* wsum, const float* prior, const float* vhat,
                                                          const sz_gumbel_options* opts, double* score_out, int* selected_out, double* vmix_out) {
    extern __shared__ u64 lds64[];
    EdgeStat* ch = (EdgeStat*)lds64;
    const int cs = blockIdx.x, lo = offsets[cs], n = offsets[cs + 1] - lo, lane = lane_id();
    if (n <= 0 || n > SZ_MAX_CHILDREN) { if (lane == 0) selected_out[cs] = -1; return; }
    for (int c = lane; c < n; c += 64) { EdgeStat s; s.W = wsum[lo + c]; s.N = vc[lo + c]; s.P = prior[lo + c]; ch[c] = s; }
    __syncthreads();
    const sz_gumbel_options o = opts[cs];
    const int bi = wave_select_tree_gumbel(ch, n, o, vhat[cs], score_out + lo, vmix_out + cs);
    if (lane == 0) selected_out[cs] = bi;
}

// test hook (sz_debug_endings): wave_ending, the function k_play<.., EndOpts> calls, on caller-supplied cases, one wave per case
__global__ __launch_bounds__(64) void k_debug_endings(const int* offsets, const int* vc, const double* wsum, const int8_t* root_proven, const uint8_t* colour,
                                                      const int* ply, const uint8_t* holdout, const int* state_in, const sz_ending_options* opts,
                                                      int* kind_out, double* m_out, int* state_out) {
    extern __shared__ u64 lds64[];
    EdgeStat* ch = (EdgeStat*)lds64;
    const int cs = blockIdx.x, lo = offsets[cs], n = offsets[cs + 1] - lo, lane = lane_id();
    if (n <= 0 || n > SZ_MAX_CHILDREN) { if (lane == 0) kind_out[cs] = -1; return; }
    for (int c = lane; c < n; c += 64) { EdgeStat s; s.W = wsum[lo + c]; s.N = vc[lo + c]; s.P = 0.0f; ch[c] = s; }
    __syncthreads();
    const int* si = state_in + (size_t)cs * 6;
    EndState st; st.rs[0] = si[0]; st.rs[1] = si[1]; st.ds = si[2]; st.would_ply = si[3]; st.would_kind = si[4]; st.would_colour = si[5];
    double m; bool marked;
    const int kind = wave_ending(ch, n, root_proven[cs] & PR_MASK, colour[cs], ply[cs], st, opts[cs], holdout[cs] != 0, &m, &marked);
    if (lane == 0) {
        int* so = state_out + (size_t)cs * 6;
        kind_out[cs] = kind; m_out[cs] = m;
        so[0] = st.rs[0]; so[1] = st.rs[1]; so[2] = st.ds; so[3] = st.would_ply; so[4] = st.would_kind; so[5] = st.would_colour;
    }
}

// test hook (sz_debug_temperature): wave_temperature, the function k_play<.., TempOpts> calls, on caller-supplied cases, one wave per case.
// The weights go straight to weights_out (the case's span is the function's work array); a greedy or proven-win case writes none.
__global__ __launch_bounds__(64) void k_debug_temperature(const int* offsets, const int* vc, const int* tree_vc, const double* wsum, const double* temps,
                                                          const double* uniforms, const int* proven_move, const sz_temperature_options* opts, int* chosen_out,
                                                          int* kind_out, int* nelig_out, double* pch_out, int* excl_out, double* weights_out) {
    extern __shared__ u64 lds64[];
    EdgeStat* ch = (EdgeStat*)lds64;
    int* vis = (int*)(ch + SZ_MAX_CHILDREN);
    const int cs = blockIdx.x, lo = offsets[cs], n = offsets[cs + 1] - lo, lane = lane_id();
    if (n <= 0 || n > SZ_MAX_CHILDREN) { if (lane == 0) chosen_out[cs] = -1; return; }
    for (int c = lane; c < n; c += 64) { EdgeStat s; s.W = wsum[lo + c]; s.N = tree_vc ? tree_vc[lo + c] : vc[lo + c]; s.P = 0.0f; ch[c] = s; vis[c] = vc[lo + c]; }
    __syncthreads();
    int pmove = proven_move ? uni(proven_move[cs]) : -1;
    if (pmove >= n) pmove = -1;
    int kind, ne, ex; double p;
    const int mv = wave_temperature(ch, vis, n, opts[cs], uni_f64(temps[cs]), uni_f64(uniforms[cs]), pmove, weights_out + lo, &kind, &ne, &p, &ex);
    if (lane == 0) { chosen_out[cs] = mv; kind_out[cs] = kind; nelig_out[cs] = ne; pch_out[cs] = p; excl_out[cs] = ex; }
}

// test hook (sz_debug_cpuct): puct_c, the function the option's k_search_step and k_play call, on caller-supplied cases, one lane per case
__global__ __launch_bounds__(64) void k_debug_cpuct(const int* n_p, const uint8_t* is_root, const sz_cpuct_options* opts, float* c_out, int n_cases) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n_cases) c_out[i] = puct_c(opts[i], n_p[i], is_root[i] != 0);
}

// ------------------------------------------------------------------------------------------------
// NON-REFERENCE option (sz_set_kld_stop; include/sigmazero.h is the rule, sz_kldgain.h the term): a board's search stops when the
// Kullback-Leibler gain per new root-child visit falls below a threshold.  The rule lives in the kernels below, which the host launches beside
// k_search_begin and at check points; k_search_begin, k_search_step and k_play have no variant: they read the board's goal where they read a
// budget, and a stop lowers it.
// ------------------------------------------------------------------------------------------------
struct KldStop {
    sz_kld_stop_options o;
    int* goal;                  // [B] the goals in force: View::budget (and BeginOpts::goal under visit targets) point here while the option is on
    int* goal0;                 // [B] the goal k_search_begin left, what sz_search_goals reports
    int* prev;                  // [B][SZ_MAX_MOVES] the root children's N at the last snapshot
    int* prev_total;            // [B] their sum; 0 at search begin
    int* has_prev;              // [B] a snapshot was taken in this search
    int* stopped_at;            // [B] the goal the board was stopped at, -1 = not stopped
    int* checks;                // [B] checks evaluated in this search (a gain was formed)
    double* last_gain;          // [B] the last of them, per new visit; NaN before the first
    unsigned long long* stat;   // [B][3] boards stopped early, checks evaluated, simulations not made
};

// the goals of a search without visit targets, before k_search_begin reads them: the board's budget (sz_set_search_budgets), else num_searches
__global__ void k_kld_goals(int* goal, const int* budget, int S, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) goal[b] = budget ? budget[b] : S;
}

// after k_search_begin: every board that starts a search, fresh or continued, starts with clean stop state, and its goal is kept
__global__ void k_kld_begin(View v, KldStop ks) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= v.B || !(v.ctl[b].status & ST_SEARCHING)) return;
    ks.goal0[b] = ks.goal[b];
    ks.prev_total[b] = 0; ks.has_prev[b] = 0; ks.stopped_at[b] = -1; ks.checks[b] = 0;
    ks.last_gain[b] = __longlong_as_double(0x7ff8000000000000LL);
}

// gain = sum over the K children of sz_kld_term in the project's fixed order: lane l adds term_l, term_{l+64}, ... ascending, then the xor
// butterfly.  now(c): child c's count now.  The same sum in every lane (f64 addition commutes).
template <typename NowF>
__device__ __forceinline__ double wave_kld_gain(const int* prev, NowF now, int K, int prev_total, int new_total) {
    double acc = 0.0;
    for (int c = lane_id(); c < K; c += 64) acc = acc + sz_kld_term(prev[c], prev_total, now(c), new_total);
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    return uni_f64(acc);
}
__device__ __forceinline__ int wave_sum_int(int x) {
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return uni(x);
}

// the check (sz_search_check_stop): one wavefront per board.  vl: leaf batching is on, the board's leaves in flight are n_pend
__global__ __launch_bounds__(64) void k_kld_check(View v, KldStop ks, int vl) {
    const int b = blockIdx.x, lane = lane_id();
    BoardPtrs bp = board_ptrs(v, b);
    const int status = uni(bp.ctl->status);
    if (!(status & ST_SEARCHING) || (status & (ST_DONE | ST_ERROR)) || uni(ks.stopped_at[b]) >= 0) return;
    const EdgeMeta rm = bp.em[0];
    int K = uni((int)rm.n);
    const int first = uni(rm.first);
    if (K <= 0 || first < 0) return;                                  // the root is not expanded yet
    if (K > SZ_MAX_MOVES) K = SZ_MAX_MOVES;
    const EdgeStat* ch = bp.es + first;
    int* prev = ks.prev + (size_t)b * SZ_MAX_MOVES;
    int part = 0;
    for (int c = lane; c < K; c += 64) part += ch[c].N;               // counted visits only: no in-flight count
    const int new_total = wave_sum_int(part), prev_total = uni(ks.prev_total[b]);
    if (new_total < prev_total + ks.o.interval) return;
    const int sims = uni(bp.ctl->sims_done);
    bool stop = false;
    if (uni(ks.has_prev[b]) && prev_total > 0) {
        const double gain = wave_kld_gain(prev, [&](int c) { return ch[c].N; }, K, prev_total, new_total);
        const double g = gain / (double)(new_total - prev_total);
        stop = g < ks.o.min_gain && sims >= ks.o.min_simulations;
        if (lane == 0) { ks.last_gain[b] = g; ks.checks[b] += 1; ks.stat[(size_t)b * 3 + 1] += 1; }
    }
    if (stop) {
        // the goal becomes what is made and in flight: the next sz_search_step consumes the leaves in flight, starts no descent and sets ST_DONE
        if (lane == 0) {
            const int pending = vl ? bp.ctl->n_pend : ((status & ST_PENDING) ? 1 : 0);
            const int s = sims + pending;
            ks.stopped_at[b] = s; ks.goal[b] = s;
            ks.stat[(size_t)b * 3] += 1; ks.stat[(size_t)b * 3 + 2] += (unsigned long long)(ks.goal0[b] - s);
            if (!pending) bp.ctl->status = status | ST_DONE;
        }
        return;
    }
    for (int c = lane; c < K; c += 64) prev[c] = ch[c].N;
    if (lane == 0) { ks.prev_total[b] = new_total; ks.has_prev[b] = 1; }
}

// test hook (sz_debug_kld_gain): wave_kld_gain, the function k_kld_check calls, on caller-supplied cases, one wavefront per case
__global__ __launch_bounds__(64) void k_debug_kld_gain(const int* prev, const int* now, const int* n_child, double* gain_out) {
    const int cs = blockIdx.x;
    const int* p = prev + (size_t)cs * SZ_MAX_MOVES;
    const int* q = now + (size_t)cs * SZ_MAX_MOVES;
    int K = uni(n_child[cs]);
    if (K < 0) K = 0;
    if (K > SZ_MAX_MOVES) K = SZ_MAX_MOVES;
    int pp = 0, pq = 0;
    for (int c = lane_id(); c < K; c += 64) { pp += p[c]; pq += q[c]; }
    const int prev_total = wave_sum_int(pp), new_total = wave_sum_int(pq);
    const double gain = wave_kld_gain(p, [&](int c) { return q[c]; }, K, prev_total, new_total);
    if (lane_id() == 0) gain_out[cs] = gain;
}

// ------------------------------------------------------------------------------------------------
// NON-REFERENCE option (sz_set_search_summary; include/sigmazero.h is the rule, sz_summary.h the scalar arithmetic, the child order and the
// logarithm's precondition): what a finished search hands to the trainer beside the visit counts.  Two kernels of their own around k_play, one
// wavefront per board; k_play, k_search_begin, k_search_step and k_play_moves have no variant and no new argument.
// ------------------------------------------------------------------------------------------------
struct SummaryOpts {
    double* root_q;             // [B] the mover's expected outcome over the whole search; NaN on a board that did not play
    double* best_q;             // [B] ... over the most visited child's visits: sz_set_endings' m
    double* surprise;           // [B] KL(record's visit fractions || stored priors); NaN on a board that did not play or whose record holds no visit
    uint8_t* valid;             // [B] the board played in the last sz_play and the three values above are its summary
    float* prior;               // [B][SZ_MAX_MOVES] the root children's stored priors, copied by k_summary_pre for k_summary_post
    unsigned long long* stat;   // [B][2] summaries made, terms dropped by the precondition rule
};

// root_q and best_q of the K children with counts N(c) and value sums W(c), lanes = children.  false (nothing written): no child or no visit,
// k_play's SZ_ERR_ZERO_VISITS.  Every lane returns the same.
template <typename NF, typename WF>
__device__ __forceinline__ bool wave_summary_values(NF N, WF W, int K, double* root_q, double* best_q) {
    const int lane = lane_id();
    int part = 0, bn = -1, bi = 0x7fffffff;
    double acc = 0.0;
    for (int c = lane; c < K; c += 64) {
        const int nc = N(c);
        part += nc;
        if (nc > bn) { bn = nc; bi = c; }
        acc = acc + sz_summary_value_term(nc, W(c));
    }
    for (int off = 32; off >= 1; off >>= 1) {                              // the first maximum of N_c, wave_ending's butterfly
        const int on = __shfl_xor(bn, off), oi = __shfl_xor(bi, off);
        if (on > bn || (on == bn && oi < bi)) { bn = on; bi = oi; }
    }
    const int total = wave_sum_int(part);
    if (K <= 0 || total == 0) return false;
    *root_q = sz_summary_root_q(wave_sum_f64(acc), total);
    bi = uni(bi);
    *best_q = sz_summary_best_q(uni_f64(W(bi)), uni(N(bi)));
    return true;
}

// the surprise of the K children with record counts n(c) against the priors P(c); NaN when the record holds no visit.  *dropped: the terms
// the precondition rule left out.  Every lane returns the same.
template <typename RF, typename PF>
__device__ __forceinline__ double wave_summary_surprise(RF n, PF P, int K, int* dropped) {
    const int lane = lane_id();
    int part = 0;
    for (int c = lane; c < K; c += 64) part += n(c);
    const int rtotal = wave_sum_int(part);
    *dropped = 0;
    if (rtotal == 0) return sz_summary_nan();
    double acc = 0.0;
    int drop = 0;
    for (int c = lane; c < K; c += 64) acc = acc + sz_summary_term(n(c), rtotal, P(c), &drop);
    *dropped = wave_sum_int(drop);
    return wave_sum_f64(acc);
}

// before k_play, while the tree is intact: the two values and the priors of every board that will play.  The conditions are k_play's early
// return and its zero-visit check, restated.
__global__ __launch_bounds__(64) void k_summary_pre(View v, SummaryOpts so) {
    const int b = blockIdx.x, lane = lane_id();
    BoardPtrs bp = board_ptrs(v, b);
    const int status = uni(bp.ctl->status);
    double rq = sz_summary_nan(), bq = sz_summary_nan();
    bool ok = (status & ST_SEARCHING) && (status & ST_DONE) && !(status & (ST_ERROR | ST_GAMEOVER));
    if (ok) {
        const EdgeMeta rm = bp.em[0];
        int K = uni((int)rm.n);
        const int first = uni(rm.first);
        if (K > SZ_MAX_MOVES) K = SZ_MAX_MOVES;
        ok = K > 0 && first >= 0;
        if (ok) {
            const EdgeStat* ch = bp.es + first;
            ok = wave_summary_values([&](int c) { return ch[c].N; }, [&](int c) { return ch[c].W; }, K, &rq, &bq);
            if (ok) for (int c = lane; c < K; c += 64) so.prior[(size_t)b * SZ_MAX_MOVES + c] = ch[c].P;
        }
    }
    if (lane == 0) { so.valid[b] = ok ? 1 : 0; so.root_q[b] = rq; so.best_q[b] = bq; so.surprise[b] = sz_summary_nan(); }
}

// after k_play: the surprise of every board k_summary_pre marked, on the record k_play just wrote (the pruned counts on a forced board)
__global__ __launch_bounds__(64) void k_summary_post(View v, SummaryOpts so) {
    const int b = blockIdx.x;
    if (!uni((int)so.valid[b])) return;
    int K = uni(v.rec_nchild[b]);
    if (K < 0) K = 0;
    if (K > SZ_MAX_MOVES) K = SZ_MAX_MOVES;
    const int* rv = v.rec_visits + (size_t)b * SZ_MAX_CHILDREN;
    const float* pr = so.prior + (size_t)b * SZ_MAX_MOVES;
    int dropped;
    const double s = wave_summary_surprise([&](int c) { return rv[c]; }, [&](int c) { return pr[c]; }, K, &dropped);
    if (lane_id() == 0) { so.surprise[b] = s; so.stat[(size_t)b * 2] += 1; so.stat[(size_t)b * 2 + 1] += (unsigned long long)dropped; }
}

// test hook (sz_debug_search_summary): wave_summary_values and wave_summary_surprise, the functions the two kernels call, on caller-supplied
// cases, one wavefront per case.  out3[cs] = root_q, best_q (NaN both without a child or a visit), surprise.
__global__ __launch_bounds__(64) void k_debug_search_summary(const int* n_child, const int* tree_vc, const double* value_sum, const float* prior, const int* record_vc,
                                                             double* out3) {
    const int cs = blockIdx.x;
    const int* tn = tree_vc + (size_t)cs * SZ_MAX_MOVES;
    const double* tw = value_sum + (size_t)cs * SZ_MAX_MOVES;
    const float* pr = prior + (size_t)cs * SZ_MAX_MOVES;
    const int* rv = record_vc + (size_t)cs * SZ_MAX_MOVES;
    int K = uni(n_child[cs]);
    if (K < 0) K = 0;
    if (K > SZ_MAX_MOVES) K = SZ_MAX_MOVES;
    double rq = sz_summary_nan(), bq = sz_summary_nan();
    wave_summary_values([&](int c) { return tn[c]; }, [&](int c) { return tw[c]; }, K, &rq, &bq);
    int dropped;
    const double s = wave_summary_surprise([&](int c) { return rv[c]; }, [&](int c) { return pr[c]; }, K, &dropped);
    if (lane_id() == 0) { out3[(size_t)cs * 3] = rq; out3[(size_t)cs * 3 + 1] = bq; out3[(size_t)cs * 3 + 2] = s; }
}

// ------------------------------------------------------------------------------------------------
// NON-REFERENCE option (sz_set_lcb): readout and test hooks.  The rule itself is wave_lcb, called by k_play<.., LcbOpts>.
// ------------------------------------------------------------------------------------------------
// the root children's square sums in sz_root_children's order (sz_root_value_spread); 0.0 beyond the children and on a board without a search
__global__ __launch_bounds__(64) void k_root_spread(View v, const double* Q, double* out) {
    const int b = blockIdx.x, lane = lane_id();
    BoardPtrs bp = board_ptrs(v, b);
    int n = 0, first = 0;
    if (bp.ctl->status & ST_SEARCHING) { EdgeMeta m = bp.em[0]; n = m.n; first = m.first; }
    for (int c = lane; c < SZ_MAX_CHILDREN; c += 64) out[(size_t)b * SZ_MAX_CHILDREN + c] = c < n ? Q[(size_t)b * v.e_cap + first + c] : 0.0;
}

// test hook (sz_debug_lcb): wave_lcb, the function k_play<.., LcbOpts> calls, on caller-supplied cases, one wave per case: the counts the move
// choice reads, the tree's N, W and Q, the options.  lcb_out receives every child's bound.
__global__ __launch_bounds__(64) void k_debug_lcb(const int* offsets, const int* vc, const int* tree_vc, const double* wsum, const double* qsum, const sz_lcb_options* opts,
                                                  int* move_out, int* cstar_out, int* ncand_out, int* bad_out, double* lcb_out) {
    extern __shared__ u64 lds64[];
    EdgeStat* ch = (EdgeStat*)lds64;
    int* vis = (int*)(ch + SZ_MAX_CHILDREN);
    const int cs = blockIdx.x, lo = offsets[cs], n = offsets[cs + 1] - lo, lane = lane_id();
    if (n <= 0 || n > SZ_MAX_CHILDREN) { if (lane == 0) { move_out[cs] = -1; cstar_out[cs] = -1; ncand_out[cs] = 0; bad_out[cs] = 0; } return; }
    for (int c = lane; c < n; c += 64) { EdgeStat s; s.W = wsum[lo + c]; s.N = tree_vc[lo + c]; s.P = 0.0f; ch[c] = s; vis[c] = vc[lo + c]; }
    __syncthreads();
    int cstar, ncand, bad; double lm, ls;
    const int mv = wave_lcb(ch, qsum + lo, vis, n, opts[cs], lcb_out + lo, &cstar, &lm, &ls, &ncand, &bad);
    if (lane == 0) { move_out[cs] = mv; cstar_out[cs] = cstar; ncand_out[cs] = ncand; bad_out[cs] = bad; }
}
// ... and sz_ssqrt on an array of arguments, one lane per argument
__global__ __launch_bounds__(64) void k_debug_ssqrt(const double* x, double* out, int* bad_out, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int bad = 0;
    out[i] = sz_ssqrt(x[i], &bad);
    if (bad_out) bad_out[i] = bad;
}

// ------------------------------------------------------------------------------------------------
// host side: the C ABI
// ------------------------------------------------------------------------------------------------
// what sz_set_forced_playouts, sz_set_fpu, sz_set_gumbel and sz_set_cpuct set for the next sz_search_begin, which takes it up whole: a search, its descent-only
// launch, its steps and its sz_play run with what its sz_search_begin saw, whatever the setters are told in between
struct Latched {
    float forced_k;                 // the forced constant, 0 = off; > 0 selects the FORCED instantiations
    sz_fpu_options fpu;             // all zero = off; a mode other than SZ_FPU_REFERENCE selects the FPU instantiations
    int gumbel_on;                  // != 0 selects the GUMBEL instantiations ...
    sz_gumbel_options gumbel; const double* gumbel_g;      // ... which run with these
    int gumbel_tree;                // sz_set_gumbel_tree: != 0 (only beside gumbel_on) selects k_search_step<false, false, GumbelTreeOpts>
    int cpuct_on;                   // sz_set_cpuct: != 0 (never beside gumbel_on) selects the instantiations that take PuctOpts ...
    sz_cpuct_options cpuct;         // ... which run with these
    int lcb_on;                     // sz_set_lcb: != 0 (never beside gumbel_on) selects the instantiations that take SpreadOpts / LcbOpts ...
    sz_lcb_options lcb;             // ... and k_play's run with these
};

struct sz_engine {
    sz_config cfg;
    View v;
    size_t lds_bytes;
    std::vector<void*> allocs;
    int* d_scharnagl; uint8_t* d_active;
    int* d_slot; int* d_nlive;
    int* d_slot_next;               // sz_compact_searching: the mapping being built (swapped with d_slot when the call succeeds)
    int* d_budget;                  // sz_set_search_budgets: [n_boards], View::budget points here while budgets are set
    int* d_target; int* d_goal;     // sz_set_visit_targets: [n_boards] each; bo.target / bo.goal and View::budget point here while targets are set
    uint8_t* d_quiet;               // sz_set_search_root_noise: [n_boards], bo.quiet points here while a quiet array is set
    BeginOpts bo;                   // k_search_begin's view of the two options; all NULL = off
    void* stage; size_t stage_bytes;    // sz_compact_searching: staging buffer of the row move, allocated on first use
    Batch vb;                       // sz_set_leaf_batching; vb.L == 1: the reference's search, nothing allocated
    int vb_cap;                     // L the batching buffers were allocated for
    std::vector<void*> vb_allocs;
    int solver;                     // sz_set_solver: the SOLVE instantiations of begin / step / play run
    unsigned long long* d_sstat;    // its counters [n_boards][2], allocated by the first enabling call
    Latched next, cur;              // sz_set_forced_playouts, sz_set_fpu, sz_set_gumbel, sz_set_cpuct: what the next sz_search_begin takes up, and what it took up last
    ForcedOpts fo;                  // sz_set_forced_playouts: fo.boards [n_boards] and fo.stat [n_boards][2], allocated by the first enabling call
    GumbelOpts go;                  // sz_set_gumbel: its arrays, allocated by the first enabling call (go.stat != NULL from then on)
    float* gt_nval;                 // sz_set_gumbel_tree: the node values [n_boards][n_cap] and the counter [n_boards], allocated by the first
    unsigned long long* gt_stat;    //     enabling call (gt_stat != NULL from then on)
    int end_on;                     // sz_set_endings: sz_play runs the ENDING instantiations of k_play
    EndOpts eo;                     // ... with these; its arrays are allocated by the first enabling call (eo.state != NULL from then on)
    int temp_on;                    // sz_set_move_temperature: sz_play runs the TEMPERATURE instantiations of k_play
    TempOpts to;                    // ... with these; its arrays are allocated by the first enabling call (to.stat != NULL from then on)
    int budgets_set, targets_set;   // sz_set_search_budgets / sz_set_visit_targets hold an array: what goal_view points View::budget and bo at
    int kld_on;                     // sz_set_kld_stop: View::budget points at d_goal, sz_search_begin fills it, sz_search_check_stop lowers it
    KldStop ks;                     // ... with these; its arrays are allocated by the first enabling call (ks.stat != NULL from then on)
    int search_open;                // a sz_search_begin was made and neither sz_play, sz_play_moves nor a sz_compact_searching that found no board followed
    int sum_on;                     // sz_set_search_summary: sz_play launches k_summary_pre before k_play and k_summary_post after it
    SummaryOpts so;                 // ... with these; its arrays are allocated by the first enabling call (so.stat != NULL from then on)
    LcbOpts lo;                     // sz_set_lcb: Q, the last play's outputs and the counters, allocated by the first enabling call (lo.stat != NULL from then on)
    double* lcb_q;                  // ... lo.Q without the const: SpreadOpts::Q
};

#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { fprintf(stderr, "[sigmazero] HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); return SZ_ERR_HIP; } } while (0)

// every entry point runs with the engine's device current and restores the caller's afterwards (one engine per GPU per process;
// a rank whose torch current device is not the engine's must not see it changed under its feet)
struct DeviceGuard {
    int prev = -1; bool changed = false;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess); }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};
#define ENGINE_GUARD(e) DeviceGuard _guard((e)->cfg.device)

template <typename T> static int dalloc(sz_engine* e, T** p, size_t count) {
    void* q = nullptr;
    hipError_t err = hipMalloc(&q, count * sizeof(T));
    if (err != hipSuccess) { fprintf(stderr, "[sigmazero] hipMalloc(%zu bytes) failed: %s\n", count * sizeof(T), hipGetErrorString(err)); return SZ_ERR_HIP; }
    e->allocs.push_back(q);
    *p = (T*)q;
    return SZ_OK;
}

// The one place that maps the options in force to a kernel instantiation, for sz_search_begin, sz_search_step and sz_play alike.  f(vl, solve, o...)
// is called with two std::bool_constants, VL = leaf batching on (vb.L > 1; instantiations without it take an empty Batch) and SOLVE = the solver
// on, and with the option structs in force, in the order the kernels take them: ForcedOpts or else GumbelOpts (the search begun last, e->cur;
// under Gumbel VL = SOLVE = false, which the setters' refusals see to; GumbelTreeOpts in its place and no FpuOpts under sz_set_gumbel_tree),
// FpuOpts (e->cur), PuctOpts (e->cur; never beside GumbelOpts), TempOpts (sz_set_move_temperature; never beside GumbelOpts), EndOpts (sz_set_endings; `proven` cleared while the
// solver is off; never beside GumbelOpts), SpreadOpts and LcbOpts (sz_set_lcb, e->cur; never beside GumbelOpts).  Each kernel takes the members of the pack that concern it: pick below.
template <typename F> static void with_search_options(const sz_engine* e, F&& f) {
    const Latched& c = e->cur;
    auto spread = [&](auto vl, auto solve, auto... o) {                     // sz_set_lcb, latched: the last two members, never beside GumbelOpts
        if (c.lcb_on) { LcbOpts lo = e->lo; lo.o = c.lcb; f(vl, solve, o..., SpreadOpts{e->lcb_q}, lo); }
        else f(vl, solve, o...);
    };
    auto endings = [&](auto vl, auto solve, auto... o) {
        if constexpr (has_opt<GumbelOpts, decltype(o)...> || has_opt<GumbelTreeOpts, decltype(o)...>) f(vl, solve, o...);
        else if (e->end_on) { EndOpts eo = e->eo; if (!decltype(solve)::value) eo.o.proven = 0; spread(vl, solve, o..., eo); }
        else spread(vl, solve, o...);
    };
    auto temperature = [&](auto vl, auto solve, auto... o) {
        if constexpr (has_opt<GumbelOpts, decltype(o)...>) endings(vl, solve, o...);
        else if (e->temp_on) endings(vl, solve, o..., e->to);
        else endings(vl, solve, o...);
    };
    auto puct = [&](auto vl, auto solve, auto... o) {
        if constexpr (has_opt<GumbelOpts, decltype(o)...>) temperature(vl, solve, o...);
        else if (c.cpuct_on) temperature(vl, solve, o..., PuctOpts{c.cpuct});
        else temperature(vl, solve, o...);
    };
    auto fpu = [&](auto vl, auto solve, auto... o) {
        if (c.fpu.tree_mode != SZ_FPU_REFERENCE || c.fpu.root_mode != SZ_FPU_REFERENCE) puct(vl, solve, o..., FpuOpts{c.fpu}); else puct(vl, solve, o...);
    };
    auto forced = [&](auto vl, auto solve) {
        if (c.forced_k > 0.0f) { ForcedOpts fo = e->fo; fo.k = c.forced_k; fpu(vl, solve, fo); } else fpu(vl, solve);
    };
    if (c.gumbel_on) {
        GumbelOpts go = e->go; go.o = c.gumbel; go.g = c.gumbel_g;
        if (c.gumbel_tree) {                                                // sz_set_gumbel_tree: in GumbelOpts' place, and FpuOpts is left out: neither site is consulted
            GumbelTreeOpts gt; static_cast<GumbelOpts&>(gt) = go; gt.nval = e->gt_nval; gt.tstat = e->gt_stat;
            endings(std::false_type{}, std::false_type{}, gt);
        } else fpu(std::false_type{}, std::false_type{}, go);
    }
    else if (e->vb.L > 1) { if (e->solver) forced(std::true_type{}, std::true_type{}); else forced(std::true_type{}, std::false_type{}); }
    else                  { if (e->solver) forced(std::false_type{}, std::true_type{}); else forced(std::false_type{}, std::false_type{}); }
}
// the members of an option pack whose type is one of Keep..., as a tuple to std::apply a launch to
template <typename... Keep, typename O> static auto pick1(const O& o) {
    if constexpr (has_opt<O, Keep...>) return std::tuple<O>(o); else return std::tuple<>();
}
template <typename... Keep, typename... O> static auto pick(const O&... o) { return std::tuple_cat(pick1<Keep...>(o)...); }
// sz_play's view of a member of the pack: the tree rule (sz_set_gumbel_tree) acts in the descent alone, k_play takes its GumbelOpts part
template <typename O> static const O& play_opt(const O& o) { return o; }
static GumbelOpts play_opt(const GumbelTreeOpts& o) { return o; }

extern "C" {

const char* sz_error_string(int code) {
    switch (code) {
        case SZ_OK: return "ok";
        case SZ_ERR_INVALID: return "invalid argument or illegal move";
        case SZ_ERR_HIP: return "HIP runtime error";
        case SZ_ERR_CAPACITY: return "node/edge capacity exhausted on a board";
        case SZ_ERR_NO_DEVICE: return "no HIP device: the engine has no CPU fallback";
        case SZ_ERR_STATE: return "call sequence violated";
        case SZ_ERR_ZERO_VISITS: return "root children have no visits (num_searches == 1 divides by zero in the reference)";
        default: return "unknown error";
    }
}

int sz_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sz_create(const sz_config* cfg, sz_engine** out) {
    if (!cfg || !out || cfg->n_boards <= 0 || cfg->num_searches < 0) return SZ_ERR_INVALID;
    if (sz_device_count() <= 0) return SZ_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= sz_device_count()) return SZ_ERR_INVALID;
    DeviceGuard _guard(cfg->device);
    sz_engine* e = new sz_engine();
    e->cfg = *cfg;
    View& v = e->v;
    memset(&v, 0, sizeof v);
    v.B = cfg->n_boards; v.S = cfg->num_searches;
    v.reuse = cfg->reuse_subtree ? 1 : 0;
    v.n_cap = (v.reuse ? 2 : 1) * cfg->num_searches + 2;     // reuse: up to num_searches kept nodes + num_searches new ones
    if (cfg->edges_per_board > 0) {
        v.e_cap = cfg->edges_per_board;
    } else {
        // default: the worst case (every expansion creates the maximum of 218 children) when it fits in half of the free HBM, so that no
        // position can overflow a search (4096 boards x 800 searches: 22.9 GB of the 288 GB); otherwise what fits, at least 64 per search
        const long long worst = (long long)(v.reuse ? 2 : 1) * cfg->num_searches * SZ_MAX_MOVES + 2, floor_cap = (long long)cfg->num_searches * 64 + 256;
        size_t free_b = 0, total_b = 0;
        long long fit = floor_cap;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            fit = (long long)(free_b / 2 / ((size_t)cfg->n_boards * (sizeof(EdgeStat) + sizeof(EdgeMeta))));
        long long cap = worst < fit ? worst : fit;
        if (cap < floor_cap) cap = floor_cap;
        v.e_cap = (int)cap;
    }
    if (v.e_cap < SZ_MAX_CHILDREN + 2) v.e_cap = SZ_MAX_CHILDREN + 2;
    v.p_cap = v.n_cap;
    v.learning = cfg->learning; v.chess960 = cfg->chess960; v.planes_dtype = cfg->planes_dtype;
    v.c_puct = cfg->c_puct; v.noise = cfg->noise_value; v.root_gamma = nullptr; v.dbg = nullptr;
    e->vb.L = 1; e->vb.lam = 1.0f;
    e->lds_bytes = (LDS_HIST_WORDS + LDS_MASK_WORDS) * 8 + (size_t)(v.p_cap > 256 ? v.p_cap : 256) * 4 + 220 * 4 + 220 * 2;   // + expand stash
    if (e->lds_bytes > 64 * 1024) { delete e; return SZ_ERR_INVALID; }
    const size_t B = v.B;
    int rc = SZ_OK;
    if ((rc = dalloc(e, &v.npos, B * v.n_cap)) || (rc = dalloc(e, &v.ring, B * SZ_RING)) || (rc = dalloc(e, &v.es, B * v.e_cap)) ||
        (rc = dalloc(e, &v.em, B * v.e_cap)) || (rc = dalloc(e, &v.gpath, B * v.p_cap)) || (rc = dalloc(e, &v.pmask, B * PMASK_STRIDE)) ||
        (rc = dalloc(e, &v.ctl, B)) || (rc = dalloc(e, &v.rec_planes, B * SZ_NUM_PLANES * 8)) ||
        (rc = dalloc(e, &v.rec_action, B * SZ_MAX_CHILDREN)) || (rc = dalloc(e, &v.rec_visits, B * SZ_MAX_CHILDREN)) ||
        (rc = dalloc(e, &v.rec_nchild, B)) || (rc = dalloc(e, &v.rec_colour, B)) || (rc = dalloc(e, &v.rec_chosen, B)) ||
        (rc = dalloc(e, &v.rec_over, B)) || (rc = dalloc(e, &v.rec_result, B)) || (rc = dalloc(e, &v.rec_active, B)) ||
        (v.reuse && (rc = dalloc(e, &v.nmap, B * v.n_cap))) ||
        (rc = dalloc(e, &e->d_scharnagl, B)) || (rc = dalloc(e, &e->d_active, B)) || (rc = dalloc(e, &e->d_slot, B)) || (rc = dalloc(e, &e->d_nlive, 1)) ||
        (rc = dalloc(e, &e->d_slot_next, B)) || (rc = dalloc(e, &e->d_budget, B)) ||
        (rc = dalloc(e, &e->d_target, B)) || (rc = dalloc(e, &e->d_goal, B)) || (rc = dalloc(e, &e->d_quiet, B))) {
        sz_destroy(e);
        return rc;
    }
    HIPCHK(hipMemset(v.ctl, 0, B * sizeof(Ctl)));
    HIPCHK(hipMemset(v.ring, 0, B * SZ_RING * sizeof(SzPos)));
    HIPCHK(hipMemset(v.rec_active, 0, B));
    HIPCHK(hipMemset(e->d_goal, 0, B * sizeof(int)));
    HIPCHK(hipDeviceSynchronize());
    *out = e;
    return SZ_OK;
}

int sz_destroy(sz_engine* e) {
    if (!e) return SZ_OK;
    ENGINE_GUARD(e);
    for (void* p : e->allocs) (void)hipFree(p);
    for (void* p : e->vb_allocs) (void)hipFree(p);
    if (e->stage) (void)hipFree(e->stage);
    delete e;
    return SZ_OK;
}

int sz_new_games(sz_engine* e, const int32_t* scharnagl, const uint8_t* active, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    std::vector<int> sch(B, -1);
    if (scharnagl) for (size_t i = 0; i < B; i++) sch[i] = scharnagl[i];
    HIPCHK(hipMemcpyAsync(e->d_scharnagl, sch.data(), B * sizeof(int), hipMemcpyHostToDevice, s));
    if (active) HIPCHK(hipMemcpyAsync(e->d_active, active, B, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                    // host staging buffers go out of scope
    hipLaunchKernelGGL(k_new_games, dim3(e->v.B), dim3(64), e->lds_bytes, s, e->v, e->d_scharnagl, active ? e->d_active : nullptr);
    if (e->eo.state)                                    // sz_set_endings: streaks and marks start again with the game
        hipLaunchKernelGGL(k_reset_endings, dim3((e->v.B + 255) / 256), dim3(256), 0, s, e->eo.state, active ? e->d_active : nullptr, e->v.B, -1);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_step_stamps(sz_engine* e, void* dev_buffer) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    e->v.dbg = (unsigned long long*)dev_buffer;
    return SZ_OK;
}

int sz_compact(sz_engine* e, int32_t enable, int32_t* n_live_out, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    if (!enable) { e->v.slot = nullptr; if (n_live_out) *n_live_out = e->v.B; return SZ_OK; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_compact<false>, dim3(1), dim3(1024), 0, s, e->v, e->d_slot, e->d_nlive);
    HIPCHK(hipGetLastError());
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, e->d_nlive, sizeof n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    e->v.slot = e->d_slot;
    if (n_live_out) *n_live_out = n;
    return SZ_OK;
}

// "only between searches": SZ_ERR_STATE while some board is between sz_search_begin and the end of its search (synchronises the stream)
static int between_searches(sz_engine* e, hipStream_t s) {
    std::vector<Ctl> h(e->v.B);
    HIPCHK(hipMemcpyAsync(h.data(), e->v.ctl, h.size() * sizeof(Ctl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (const Ctl& c : h)
        if ((c.status & ST_SEARCHING) && !(c.status & (ST_DONE | ST_ERROR))) return SZ_ERR_STATE;
    return SZ_OK;
}

// sums of a per-board counter array [n_boards][width] (NULL: the option was never on, all zero) into out[0..width)
static int sum_board_counters(sz_engine* e, const unsigned long long* counters, int width, uint64_t* out, void* stream) {
    if (!e || !out) return SZ_ERR_INVALID;
    for (int k = 0; k < width; k++) out[k] = 0;
    if (!counters) return SZ_OK;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    std::vector<unsigned long long> h((size_t)e->v.B * width);
    HIPCHK(hipMemcpyAsync(h.data(), counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < h.size(); i++) out[i % width] += h[i];
    return SZ_OK;
}

// The combinations of options an engine runs, in one place.  OptionState is what they depend on; a setter takes option_state(e), applies its own
// change and asks option_refusal before it touches the engine, so the state in force is always an allowed one and switching an option off never
// leads out of it.  SZ_ERR_INVALID comes before the question whether the engine searches, SZ_ERR_STATE is the root noise's code.
struct OptionState {
    int L, solver;                  // sz_set_leaf_batching / sz_set_solver / sz_set_search_options
    bool forced, gumbel;            // sz_set_forced_playouts, sz_set_gumbel: what the next sz_search_begin takes up
    bool endings, noise;            // sz_set_endings; sz_set_root_noise / sz_set_search_root_noise with a gamma
    bool temperature;               // sz_set_move_temperature
    bool cpuct;                     // sz_set_cpuct: what the next sz_search_begin takes up
    bool kld;                       // sz_set_kld_stop
    bool summary;                   // sz_set_search_summary
    bool lcb;                       // sz_set_lcb: what the next sz_search_begin takes up
};
enum OptionSetter { BY_ANY, BY_LEAF_BATCHING, BY_SOLVER, BY_ROOT_NOISE };     // the setters whose own entry point accepts less than the engine runs
static OptionState option_state(const sz_engine* e) {
    return {e->vb.L, e->solver, e->next.forced_k > 0.0f, e->next.gumbel_on != 0, e->end_on != 0, e->v.root_gamma != nullptr, e->temp_on != 0, e->next.cpuct_on != 0, e->kld_on != 0, e->sum_on != 0, e->next.lcb_on != 0};
}
static int option_refusal(const sz_engine* e, const OptionState& p, OptionSetter by = BY_ANY) {
    const bool reuse = e->v.reuse != 0;
    if (p.forced && !e->v.learning) return SZ_ERR_INVALID;                  // an exploration option of self-play, like root noise
    // Gumbel, each combination a follow-up: a kept subtree's root was not expanded by this search, leaf batching has visits in flight, the
    // solver and forced playouts select at the root themselves, the ending rules read the most visited move
    if (p.gumbel && (reuse || p.L > 1 || p.solver || p.forced || p.endings)) return SZ_ERR_INVALID;
    // leaf batching, the solver and subtree reuse combine through sz_set_search_options alone
    if (by == BY_LEAF_BATCHING && p.L > 1 && (reuse || p.solver)) return SZ_ERR_INVALID;
    if (by == BY_SOLVER && p.solver && (reuse || p.L > 1)) return SZ_ERR_INVALID;
    if (p.gumbel && p.noise) return SZ_ERR_STATE;                           // Gumbel is the root's exploration
    if (p.gumbel && p.temperature) return SZ_ERR_STATE;                     // ... and chooses its own move
    if (p.gumbel && p.cpuct) return SZ_ERR_STATE;                           // Gumbel's rule is a chain of its own: the combination is a follow-up
    if (p.gumbel && p.kld) return SZ_ERR_STATE;                             // sequential halving plans on the goal: it cannot be lowered under it
    if (p.gumbel && p.summary) return SZ_ERR_STATE;                         // Gumbel's record is pi' and it exports v_mix itself: the combination is a follow-up
    if (p.gumbel && p.lcb) return SZ_ERR_STATE;                             // Gumbel chooses its own move and backs up through its own rule: a follow-up
    if (p.lcb && reuse) return SZ_ERR_STATE;                                // wave_keep_subtree and k_play_moves would have to compact Q too: a follow-up
    // sz_set_root_noise: a reused root was expanded as an inner node, on un-noised priors, and is never expanded again, so the noise would silently
    // apply to the first ply of a game only; and a reuse engine under sz_set_search_root_noise leaves that mode through that setter, which drops
    // the kept subtrees
    if (by == BY_ROOT_NOISE && reuse && (p.noise || e->v.root_gamma)) return SZ_ERR_STATE;
    return SZ_OK;
}

// Where the kernels read a board's simulations from.  Visit targets: k_search_begin turns d_target into d_goal and everything reads d_goal.
// Budgets: d_budget.  Neither: num_searches (NULL).  sz_set_kld_stop: d_goal in every case, which sz_search_begin fills from the budgets or
// num_searches where k_search_begin does not, so that a stop has a goal to lower.
static void goal_view(sz_engine* e) {
    e->bo.target = e->targets_set ? e->d_target : nullptr;
    e->bo.goal = e->targets_set ? e->d_goal : nullptr;
    e->v.budget = (e->targets_set || e->kld_on) ? e->d_goal : (e->budgets_set ? e->d_budget : nullptr);
}

int sz_set_search_budgets(sz_engine* e, const int32_t* budgets, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (budgets && e->v.reuse) return SZ_ERR_INVALID;                      // a kept subtree already holds simulations: not combined with budgets
    if (budgets)
        for (int b = 0; b < e->v.B; b++)
            if (budgets[b] < 0 || budgets[b] > e->v.S) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    int rc = between_searches(e, s);
    if (rc) return rc;
    if (budgets) {
        HIPCHK(hipMemcpyAsync(e->d_budget, budgets, (size_t)e->v.B * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                                    // the caller's array may go out of scope
    }
    e->budgets_set = budgets != nullptr;
    e->targets_set = 0;                                                       // budgets and visit targets exclude each other: the later setter wins
    goal_view(e);
    return SZ_OK;
}

int sz_set_visit_targets(sz_engine* e, const int32_t* targets, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (targets)
        for (int b = 0; b < e->v.B; b++)
            if (targets[b] < 0 || targets[b] > e->v.S) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    int rc = between_searches(e, s);
    if (rc) return rc;
    if (targets) {
        HIPCHK(hipMemcpyAsync(e->d_target, targets, (size_t)e->v.B * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                                    // the caller's array may go out of scope
    }
    // k_search_begin writes each board's goal into d_goal; everything that reads a budget reads it from there
    e->targets_set = targets != nullptr;
    e->budgets_set = 0;
    goal_view(e);
    return SZ_OK;
}

int sz_search_goals(sz_engine* e, int32_t* goals, void* stream) {
    if (!e || !goals) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    std::vector<Ctl> h(B);
    std::vector<int> bud(e->v.budget ? B : 0);                              // the goals (targets set), the budgets, or nothing: num_searches
    const int* src = e->kld_on ? e->ks.goal0 : e->v.budget;                 // sz_set_kld_stop: the goals at begin, whatever a stop made of them
    HIPCHK(hipMemcpyAsync(h.data(), e->v.ctl, B * sizeof(Ctl), hipMemcpyDeviceToHost, s));
    if (src) HIPCHK(hipMemcpyAsync(bud.data(), src, B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t b = 0; b < B; b++)
        goals[b] = (h[b].status & ST_SEARCHING) ? (e->v.budget ? bud[b] : e->v.S) : 0;
    return SZ_OK;
}

int sz_compact_searching(sz_engine* e, void* planes_dev, int32_t* n_live_out, void* stream) {
    if (!e || !planes_dev) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const View& v = e->v;
    const int rows = e->vb.L;
    const size_t row_bytes = v.planes_dtype == SZ_PLANES_F32 ? (size_t)SZ_NUM_PLANES * 64 * 4 : (v.planes_dtype == SZ_PLANES_BF16 ? (size_t)SZ_NUM_PLANES * 64 * 2 :
                             (v.planes_dtype == SZ_PLANES_NHWC128_BITS ? (size_t)1024 : (size_t)64 * 128 * 2));      // = planes_board_bytes, all multiples of 16
    const size_t need = (size_t)v.B * rows * row_bytes;
    if (need > e->stage_bytes) {
        HIPCHK(hipStreamSynchronize(s));
        if (e->stage) (void)hipFree(e->stage);
        e->stage = nullptr; e->stage_bytes = 0;
        hipError_t err = hipMalloc(&e->stage, need);
        if (err != hipSuccess) { fprintf(stderr, "[sigmazero] hipMalloc(%zu bytes) failed: %s\n", need, hipGetErrorString(err)); e->stage = nullptr; return SZ_ERR_HIP; }
        e->stage_bytes = need;
    }
    // new mapping into d_slot_next, rows out to the staging buffer and back; the mapping in use is replaced only when the call succeeds.
    // With no board searching (before sz_search_begin, after the search ended) every new row is -1 and the two moves touch nothing.
    hipLaunchKernelGGL(k_compact<true>, dim3(1), dim3(1024), 0, s, v, e->d_slot_next, e->d_nlive);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_move_rows, dim3(v.B), dim3(256), 0, s, (const uint4*)planes_dev, (uint4*)e->stage, v.slot, e->d_slot_next, rows, (int)(row_bytes / 16), 1);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_move_rows, dim3(v.B), dim3(256), 0, s, (const uint4*)e->stage, (uint4*)planes_dev, v.slot, e->d_slot_next, rows, (int)(row_bytes / 16), 0);
    HIPCHK(hipGetLastError());
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, e->d_nlive, sizeof n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n <= 0) { e->search_open = 0; return SZ_ERR_STATE; }
    int* t = e->d_slot; e->d_slot = e->d_slot_next; e->d_slot_next = t;
    e->v.slot = e->d_slot;
    if (n_live_out) *n_live_out = n;
    return SZ_OK;
}

int sz_set_root_noise(sz_engine* e, const float* gamma_dev) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    OptionState p = option_state(e);
    p.noise = gamma_dev != nullptr;
    if (int rc = option_refusal(e, p, BY_ROOT_NOISE)) return rc;
    e->v.root_gamma = gamma_dev;
    e->bo.quiet = nullptr;
    return SZ_OK;
}

int sz_set_search_root_noise(sz_engine* e, const float* gamma_dev, const uint8_t* quiet, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    OptionState p = option_state(e);
    p.noise = gamma_dev != nullptr;
    int rc = option_refusal(e, p);
    if (rc) return rc;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = between_searches(e, s))) return rc;
    if (quiet) {
        HIPCHK(hipMemcpyAsync(e->d_quiet, quiet, (size_t)e->v.B, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                                    // the caller's array may go out of scope
    }
    // a tree built under the reference's noise carries the constant in every node's priors, one built under root-only noise carries it nowhere
    const bool drop = e->v.reuse && ((gamma_dev != nullptr) != (e->v.root_gamma != nullptr));
    e->v.root_gamma = gamma_dev;
    e->bo.quiet = quiet ? e->d_quiet : nullptr;
    if (drop) {
        hipLaunchKernelGGL(k_drop_subtrees, dim3((e->v.B + 255) / 256), dim3(256), 0, s, e->v);
        HIPCHK(hipGetLastError());
    }
    return SZ_OK;
}

int sz_set_active(sz_engine* e, const uint8_t* active, void* stream) {
    if (!e || !active) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(e->d_active, active, e->v.B, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    hipLaunchKernelGGL(k_set_active, dim3((e->v.B + 255) / 256), dim3(256), 0, s, e->v, e->d_active);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_upload_game(sz_engine* e, int32_t board, const void* ring, int32_t ply, void* stream) {
    if (!e || !ring || board < 0 || board >= e->v.B || ply < 0) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(e->v.ring + (size_t)board * SZ_RING, ring, SZ_RING * sizeof(SzPos), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    hipLaunchKernelGGL(k_after_upload, dim3(1), dim3(1), 0, s, e->v, board, ply);
    if (e->eo.state)                                    // sz_set_endings: streaks and marks start again with the game
        hipLaunchKernelGGL(k_reset_endings, dim3((e->v.B + 255) / 256), dim3(256), 0, s, e->eo.state, (const uint8_t*)nullptr, e->v.B, board);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

// the k_search_step instantiation of the options in force; policy == NULL: the descent-only launch of sz_search_begin
static void launch_step(sz_engine* e, const float* policy, const float* value, void* planes, hipStream_t s) {
    with_search_options(e, [&](auto vl, auto solve, auto... o) {
        constexpr bool VL = decltype(vl)::value, SOLVE = decltype(solve)::value;
        std::apply([&](auto... k) {
            hipLaunchKernelGGL((k_search_step<VL, SOLVE, decltype(k)...>), dim3(e->v.B), dim3(64), e->lds_bytes, s, e->v, policy, value, planes, VL ? e->vb : Batch{}, k...);
        }, pick<ForcedOpts, GumbelOpts, GumbelTreeOpts, FpuOpts, PuctOpts, SpreadOpts>(o...));      // the ending rules live in sz_play alone
    });
}

int sz_search_begin(sz_engine* e, void* planes_dev, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    e->cur = e->next;                                                       // sz_set_forced_playouts, sz_set_fpu, sz_set_gumbel, sz_set_cpuct and sz_set_lcb take effect here
    if (e->kld_on && !e->targets_set)                                       // sz_set_kld_stop: the goals k_search_begin reads as budgets (under targets it writes them itself)
        hipLaunchKernelGGL(k_kld_goals, dim3((e->v.B + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->d_goal, e->budgets_set ? e->d_budget : nullptr, e->v.S, e->v.B);
    with_search_options(e, [&](auto vl, auto solve, auto... o) {
        constexpr bool VL = decltype(vl)::value, SOLVE = decltype(solve)::value;
        std::apply([&](auto... k) {
            hipLaunchKernelGGL((k_search_begin<VL, SOLVE, decltype(k)...>), dim3(e->v.B), dim3(64), e->lds_bytes, (hipStream_t)stream, e->v, planes_dev, VL ? e->vb : Batch{}, e->bo, k...);
        }, pick<ForcedOpts, SpreadOpts>(o...));                             // the options that act where a root is made: the board's bit, the root edge's Q
    });
    HIPCHK(hipGetLastError());
    if (e->kld_on) {                                                        // sz_set_kld_stop: clean stop state for the boards that search
        hipLaunchKernelGGL(k_kld_begin, dim3((e->v.B + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->v, e->ks);
        HIPCHK(hipGetLastError());
    }
    e->search_open = 1;
    if (e->v.reuse && planes_dev) {
        // boards that continue on a kept subtree have no root to evaluate: one descent-only launch selects their first leaf (boards whose fresh
        // root waits for the network sit it out), so that every board enters the first network call with a real position.  Batched
        // (sz_set_search_options): it gathers up to L leaves; with the solver a board whose kept root is proven counts all its simulations out here
        launch_step(e, nullptr, nullptr, planes_dev, (hipStream_t)stream);
        HIPCHK(hipGetLastError());
    }
    return SZ_OK;
}

int sz_search_step(sz_engine* e, const float* policy_dev, const float* value_dev, void* planes_dev, void* stream) {
    if (!e || !policy_dev || !value_dev || !planes_dev) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    launch_step(e, policy_dev, value_dev, planes_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

// the leaf-batching buffers (in-flight counts, L paths and legal masks per board), grown on the first call that needs more than there is
static int batch_buffers(sz_engine* e, int leaves_per_step) {
    if (leaves_per_step > 1 && leaves_per_step > e->vb_cap) {
        for (void* p : e->vb_allocs) (void)hipFree(p);
        e->vb_allocs.clear(); e->vb_cap = 0;
        const size_t B = e->v.B, L = leaves_per_step;
        void* q[4] = {nullptr, nullptr, nullptr, nullptr};
        const size_t bytes[4] = {B * e->v.e_cap * sizeof(int), B * L * e->v.p_cap * sizeof(int), B * L * PMASK_STRIDE * sizeof(u64), B * L * sizeof(int)};
        for (int k = 0; k < 4; k++) {
            hipError_t err = hipMalloc(&q[k], bytes[k]);
            if (err != hipSuccess) {
                fprintf(stderr, "[sigmazero] hipMalloc(%zu bytes) failed: %s\n", bytes[k], hipGetErrorString(err));
                for (void* p : e->vb_allocs) (void)hipFree(p);
                e->vb_allocs.clear(); e->vb.L = 1;
                return SZ_ERR_HIP;
            }
            e->vb_allocs.push_back(q[k]);
        }
        e->vb.vk = (int*)q[0]; e->vb.path = (int*)q[1]; e->vb.mask = (u64*)q[2]; e->vb.depth = (int*)q[3];
        e->vb_cap = leaves_per_step;
    }
    return SZ_OK;
}

// the solver's counters, allocated by the first enabling call
static int solver_counters(sz_engine* e, hipStream_t s) {
    if (e->d_sstat) return SZ_OK;
    int rc = dalloc(e, &e->d_sstat, (size_t)e->v.B * 2);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(e->d_sstat, 0, (size_t)e->v.B * 2 * sizeof(unsigned long long), s));
    HIPCHK(hipStreamSynchronize(s));
    return SZ_OK;
}

// what the three option setters share, after their own argument checks: the combination rules as the setter `by` applies them, then only
// between searches; buffers and counters before the assignment, so a call that fails changes no option (a failed allocation of the batch
// buffers leaves leaves_per_step = 1)
static int set_options(sz_engine* e, int leaves_per_step, float virtual_loss, int solver, OptionSetter by, hipStream_t s) {
    OptionState p = option_state(e);
    p.L = leaves_per_step; p.solver = solver;
    int rc = option_refusal(e, p, by);
    if (rc || (rc = between_searches(e, s))) return rc;
    if ((rc = batch_buffers(e, leaves_per_step))) return rc;
    if (solver && (rc = solver_counters(e, s))) return rc;
    e->vb.L = leaves_per_step;
    e->vb.lam = virtual_loss;
    e->solver = solver;
    e->v.sstat = solver ? e->d_sstat : nullptr;
    return SZ_OK;
}

static bool batching_args_ok(int leaves_per_step, float virtual_loss) {
    return leaves_per_step >= 1 && leaves_per_step <= SZ_MAX_LEAVES_PER_STEP && virtual_loss >= 0.0f && std::isfinite(virtual_loss);
}

int sz_set_leaf_batching(sz_engine* e, int32_t leaves_per_step, float virtual_loss, void* stream) {
    if (!e || !batching_args_ok(leaves_per_step, virtual_loss)) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    return set_options(e, leaves_per_step, virtual_loss, e->solver, BY_LEAF_BATCHING, (hipStream_t)stream);
}

int sz_set_solver(sz_engine* e, int32_t enable, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    return set_options(e, e->vb.L, e->vb.lam, enable ? 1 : 0, BY_SOLVER, (hipStream_t)stream);
}

int sz_set_search_options(sz_engine* e, const sz_search_options* opt, void* stream) {
    if (!e || !opt || !batching_args_ok(opt->leaves_per_step, opt->virtual_loss)) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    const int solver = opt->solver ? 1 : 0;
    // a kept subtree built under other settings has no `complete` bits, or its in-flight counts were never written: start fresh
    const bool drop = e->v.reuse && (opt->leaves_per_step != e->vb.L || solver != e->solver);
    int rc = set_options(e, opt->leaves_per_step, opt->virtual_loss, solver, BY_ANY, (hipStream_t)stream);
    if (rc) return rc;
    if (drop) {
        hipLaunchKernelGGL(k_drop_subtrees, dim3((e->v.B + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->v);
        HIPCHK(hipGetLastError());
    }
    return SZ_OK;
}

int sz_root_proven(sz_engine* e, int8_t* root_dev, int8_t* child_dev, void* stream) {
    if (!e || !root_dev || !child_dev) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipLaunchKernelGGL(k_root_proven, dim3(e->v.B), dim3(64), 0, (hipStream_t)stream, e->v, root_dev, child_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_solver_stats(sz_engine* e, uint64_t out[2], void* stream) { return sum_board_counters(e, e ? e->d_sstat : nullptr, 2, out, stream); }

int sz_set_forced_playouts(sz_engine* e, float k, const uint8_t* boards, void* stream) {
    if (!e || !(k >= 0.0f) || !std::isfinite(k)) return SZ_ERR_INVALID;
    OptionState p = option_state(e);
    p.forced = k > 0.0f;
    int rc = option_refusal(e, p);
    if (rc) return rc;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = between_searches(e, s))) return rc;
    if (k > 0.0f) {
        const size_t B = e->v.B;
        if (!e->fo.stat) {                                                  // the first enabling call: the boards' bits and the counters
            uint8_t* fb = nullptr; unsigned long long* st = nullptr;
            if ((rc = dalloc(e, &fb, B)) || (rc = dalloc(e, &st, B * 2))) return rc;
            HIPCHK(hipMemsetAsync(st, 0, B * 2 * sizeof(unsigned long long), s));
            e->fo.boards = fb; e->fo.stat = st;
        }
        std::vector<uint8_t> h(B, 1);
        if (boards) for (size_t b = 0; b < B; b++) h[b] = boards[b] ? 1 : 0;
        HIPCHK(hipMemcpyAsync((void*)e->fo.boards, h.data(), B, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                                    // the staging array goes out of scope
    }
    e->next.forced_k = k;
    return SZ_OK;
}

static bool fpu_site_ok(int mode, float value) {
    if (mode == SZ_FPU_REFERENCE) return true;                              // its value is ignored
    if (!std::isfinite(value)) return false;
    if (mode == SZ_FPU_ABSOLUTE) return value >= -1.0f && value <= 1.0f;
    if (mode == SZ_FPU_REDUCTION) return value >= 0.0f && value <= 2.0f;
    return false;
}

int sz_set_fpu(sz_engine* e, const sz_fpu_options* opt, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (opt && (!fpu_site_ok(opt->tree_mode, opt->tree_value) || !fpu_site_ok(opt->root_mode, opt->root_value))) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    int rc = between_searches(e, (hipStream_t)stream);
    if (rc) return rc;
    sz_fpu_options o = {SZ_FPU_REFERENCE, 0.0f, SZ_FPU_REFERENCE, 0.0f};
    if (opt) o = *opt;
    if (o.tree_mode == SZ_FPU_REFERENCE) o.tree_value = 0.0f;
    if (o.root_mode == SZ_FPU_REFERENCE) o.root_value = 0.0f;
    e->next.fpu = o;
    return SZ_OK;
}

static bool cpuct_site_ok(float init, float base, float factor) {
    if (!std::isfinite(init) || !std::isfinite(base) || !std::isfinite(factor)) return false;
    return init >= 0.0f && init <= 100.0f && factor >= 0.0f && factor <= 100.0f && base >= 1.0f && base <= 1e9f;
}

int sz_set_cpuct(sz_engine* e, const sz_cpuct_options* opt, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (opt && (!cpuct_site_ok(opt->tree_init, opt->tree_base, opt->tree_factor) || !cpuct_site_ok(opt->root_init, opt->root_base, opt->root_factor))) return SZ_ERR_INVALID;
    OptionState p = option_state(e);
    p.cpuct = opt != nullptr;
    const int refused = option_refusal(e, p);
    if (refused == SZ_ERR_INVALID) return refused;
    ENGINE_GUARD(e);
    int rc = between_searches(e, (hipStream_t)stream);
    if (rc) return rc;
    if (!opt) { e->next.cpuct_on = 0; e->next.cpuct = sz_cpuct_options{}; return SZ_OK; }
    if (refused) return refused;                                            // Gumbel is on: SZ_ERR_STATE, after the question whether the engine searches
    e->next.cpuct = *opt; e->next.cpuct_on = 1;
    return SZ_OK;
}

int sz_set_kld_stop(sz_engine* e, const sz_kld_stop_options* opt, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (opt && (!std::isfinite(opt->min_gain) || !(opt->min_gain > 0.0) || opt->min_gain > 1.0 || opt->interval < 1 || opt->interval > e->v.S ||
                opt->min_simulations < 0 || opt->min_simulations > e->v.S)) return SZ_ERR_INVALID;
    OptionState p = option_state(e);
    p.kld = opt != nullptr;
    const int refused = option_refusal(e, p);
    if (refused == SZ_ERR_INVALID) return refused;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    int rc = between_searches(e, s);
    if (rc) return rc;
    if (!opt) { e->kld_on = 0; goal_view(e); return SZ_OK; }
    if (refused) return refused;                                            // Gumbel is on: SZ_ERR_STATE, after the question whether the engine searches
    if (!e->ks.stat) {                                                      // the first enabling call: the per-board state and the counters
        const size_t B = e->v.B;
        KldStop k = e->ks;
        if ((rc = dalloc(e, &k.goal0, B)) || (rc = dalloc(e, &k.prev, B * SZ_MAX_MOVES)) || (rc = dalloc(e, &k.prev_total, B)) || (rc = dalloc(e, &k.has_prev, B)) ||
            (rc = dalloc(e, &k.stopped_at, B)) || (rc = dalloc(e, &k.checks, B)) || (rc = dalloc(e, &k.last_gain, B)) || (rc = dalloc(e, &k.stat, B * 3))) return rc;
        HIPCHK(hipMemsetAsync(k.goal0, 0, B * sizeof(int), s));
        HIPCHK(hipMemsetAsync(k.prev, 0, B * SZ_MAX_MOVES * sizeof(int), s));
        HIPCHK(hipMemsetAsync(k.prev_total, 0, B * sizeof(int), s));
        HIPCHK(hipMemsetAsync(k.has_prev, 0, B * sizeof(int), s));
        HIPCHK(hipMemsetAsync(k.stopped_at, 0xff, B * sizeof(int), s));      // -1: no board was stopped
        HIPCHK(hipMemsetAsync(k.checks, 0, B * sizeof(int), s));
        HIPCHK(hipMemsetAsync(k.last_gain, 0xff, B * sizeof(double), s));    // a NaN: no check was evaluated
        HIPCHK(hipMemsetAsync(k.stat, 0, B * 3 * sizeof(unsigned long long), s));
        HIPCHK(hipStreamSynchronize(s));
        k.goal = e->d_goal;
        e->ks = k;
    }
    e->ks.o = *opt; e->kld_on = 1;
    goal_view(e);
    return SZ_OK;
}

int sz_search_check_stop(sz_engine* e, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (!e->kld_on) return SZ_OK;                                           // off: a driver may call it unconditionally
    if (!e->search_open) return SZ_ERR_STATE;
    ENGINE_GUARD(e);
    hipLaunchKernelGGL(k_kld_check, dim3(e->v.B), dim3(64), 0, (hipStream_t)stream, e->v, e->ks, e->vb.L > 1 ? 1 : 0);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_fetch_kld_stop(sz_engine* e, int32_t* stopped_at, int32_t* checks, double* last_gain, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (!e->ks.stat) return SZ_ERR_STATE;                                   // the option was never on
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    if (stopped_at) HIPCHK(hipMemcpyAsync(stopped_at, e->ks.stopped_at, B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (checks) HIPCHK(hipMemcpyAsync(checks, e->ks.checks, B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (last_gain) HIPCHK(hipMemcpyAsync(last_gain, e->ks.last_gain, B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SZ_OK;
}

int sz_kld_stop_stats(sz_engine* e, uint64_t out[3], void* stream) { return sum_board_counters(e, e ? e->ks.stat : nullptr, 3, out, stream); }

int sz_set_search_summary(sz_engine* e, int32_t enable, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    OptionState p = option_state(e);
    p.summary = enable != 0;
    const int refused = option_refusal(e, p);
    if (refused == SZ_ERR_INVALID) return refused;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    int rc = between_searches(e, s);
    if (rc) return rc;
    if (!enable) { e->sum_on = 0; return SZ_OK; }
    if (refused) return refused;                                            // Gumbel is on: SZ_ERR_STATE, after the question whether the engine searches
    if (!e->so.stat) {                                                      // the first enabling call: the per-board outputs, the prior copy and the counters
        const size_t B = e->v.B;
        SummaryOpts o = e->so;
        if ((rc = dalloc(e, &o.root_q, B)) || (rc = dalloc(e, &o.best_q, B)) || (rc = dalloc(e, &o.surprise, B)) || (rc = dalloc(e, &o.valid, B)) ||
            (rc = dalloc(e, &o.prior, B * SZ_MAX_MOVES)) || (rc = dalloc(e, &o.stat, B * 2))) return rc;
        HIPCHK(hipMemsetAsync(o.root_q, 0xff, B * sizeof(double), s));       // NaNs: no summary was made
        HIPCHK(hipMemsetAsync(o.best_q, 0xff, B * sizeof(double), s));
        HIPCHK(hipMemsetAsync(o.surprise, 0xff, B * sizeof(double), s));
        HIPCHK(hipMemsetAsync(o.valid, 0, B, s));
        HIPCHK(hipMemsetAsync(o.prior, 0, B * SZ_MAX_MOVES * sizeof(float), s));
        HIPCHK(hipMemsetAsync(o.stat, 0, B * 2 * sizeof(unsigned long long), s));
        HIPCHK(hipStreamSynchronize(s));
        e->so = o;
    }
    e->sum_on = 1;
    return SZ_OK;
}

int sz_fetch_search_summary(sz_engine* e, double* root_q, double* best_q, double* surprise, uint8_t* valid, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (!e->so.stat) return SZ_ERR_STATE;                                   // the option was never on
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    if (root_q) HIPCHK(hipMemcpyAsync(root_q, e->so.root_q, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (best_q) HIPCHK(hipMemcpyAsync(best_q, e->so.best_q, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (surprise) HIPCHK(hipMemcpyAsync(surprise, e->so.surprise, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (valid) HIPCHK(hipMemcpyAsync(valid, e->so.valid, B, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SZ_OK;
}

int sz_search_summary_stats(sz_engine* e, uint64_t out[2], void* stream) { return sum_board_counters(e, e ? e->so.stat : nullptr, 2, out, stream); }

int sz_set_lcb(sz_engine* e, const sz_lcb_options* opt, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (opt) {
        if (!std::isfinite(opt->stdevs) || opt->stdevs < 0.0f) return SZ_ERR_INVALID;
        if (!(opt->min_visit_prop >= 0.0f && opt->min_visit_prop <= 1.0f)) return SZ_ERR_INVALID;      // a NaN fails the comparison
    }
    OptionState p = option_state(e);
    p.lcb = opt != nullptr;
    const int refused = option_refusal(e, p);
    if (refused == SZ_ERR_INVALID) return refused;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    int rc = between_searches(e, s);
    if (rc) return rc;
    if (!opt) { e->next.lcb_on = 0; return SZ_OK; }
    if (refused) return refused;                                            // a reuse_subtree engine, or Gumbel is on: SZ_ERR_STATE, after the question whether the engine searches
    const size_t B = e->v.B;
    if (!e->lo.stat) {                                                      // the first enabling call: Q, the last play's outputs and the counters
        LcbOpts o = e->lo;
        double* q = nullptr;
        if ((rc = dalloc(e, &q, B * (size_t)e->v.e_cap)) || (rc = dalloc(e, &o.move, B)) || (rc = dalloc(e, &o.cstar, B)) || (rc = dalloc(e, &o.lcb2, B * 2)) ||
            (rc = dalloc(e, &o.ncand, B)) || (rc = dalloc(e, &o.decided, B)) || (rc = dalloc(e, &o.stat, B * 3))) return rc;
        HIPCHK(hipMemsetAsync(q, 0, B * (size_t)e->v.e_cap * sizeof(double), s));
        HIPCHK(hipMemsetAsync(o.stat, 0, B * 3 * sizeof(unsigned long long), s));
        o.Q = q;
        e->lo = o; e->lcb_q = q;
    }
    if (!e->next.lcb_on) {                                                  // off -> on: no sz_play of the option to describe yet
        HIPCHK(hipMemsetAsync(e->lo.move, 0xff, B * sizeof(int), s));       // -1
        HIPCHK(hipMemsetAsync(e->lo.cstar, 0xff, B * sizeof(int), s));
        HIPCHK(hipMemsetAsync(e->lo.lcb2, 0xff, B * 2 * sizeof(double), s));    // all ones: a NaN
        HIPCHK(hipMemsetAsync(e->lo.ncand, 0, B * sizeof(int), s));
        HIPCHK(hipMemsetAsync(e->lo.decided, 0, B, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    e->next.lcb = *opt;
    e->next.lcb.select = opt->select ? 1 : 0;
    e->next.lcb_on = 1;
    return SZ_OK;
}

int sz_fetch_lcb(sz_engine* e, int32_t* move, int32_t* cstar, double* lcb_move, double* lcb_cstar, int32_t* n_candidates, uint8_t* decided, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (!e->lo.stat) return SZ_ERR_STATE;                                   // the option was never on
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    std::vector<double> two(B * 2);
    if (move) HIPCHK(hipMemcpyAsync(move, e->lo.move, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (cstar) HIPCHK(hipMemcpyAsync(cstar, e->lo.cstar, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(two.data(), e->lo.lcb2, B * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (n_candidates) HIPCHK(hipMemcpyAsync(n_candidates, e->lo.ncand, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (decided) HIPCHK(hipMemcpyAsync(decided, e->lo.decided, B, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t b = 0; b < B; b++) { if (lcb_move) lcb_move[b] = two[b * 2]; if (lcb_cstar) lcb_cstar[b] = two[b * 2 + 1]; }
    return SZ_OK;
}

int sz_lcb_stats(sz_engine* e, uint64_t out[3], void* stream) { return sum_board_counters(e, e ? e->lo.stat : nullptr, 3, out, stream); }

int sz_root_value_spread(sz_engine* e, double* sq_sum_dev, void* stream) {
    if (!e || !sq_sum_dev) return SZ_ERR_INVALID;
    if (!e->lo.stat || !e->cur.lcb_on) return SZ_ERR_STATE;                 // the search begun last kept no second moment
    ENGINE_GUARD(e);
    hipLaunchKernelGGL(k_root_spread, dim3(e->v.B), dim3(64), 0, (hipStream_t)stream, e->v, e->lo.Q, sq_sum_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_tree_spread(sz_engine* e, int32_t board, int32_t max_nodes, double* sq_sum, int32_t* n_out, void* stream) {
    if (!e || board < 0 || board >= e->v.B || !n_out) return SZ_ERR_INVALID;
    if (!e->lo.stat || !e->cur.lcb_on) return SZ_ERR_STATE;                 // the search begun last kept no second moment
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    Ctl c;
    HIPCHK(hipMemcpyAsync(&c, e->v.ctl + board, sizeof c, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_out = 0;
    if (!(c.status & ST_SEARCHING) || c.n_edges <= 0) return SZ_OK;
    std::vector<EdgeMeta> em(c.n_edges);
    std::vector<double> q(c.n_edges);
    HIPCHK(hipMemcpyAsync(em.data(), e->v.em + (size_t)board * e->v.e_cap, em.size() * sizeof(EdgeMeta), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(q.data(), e->lo.Q + (size_t)board * e->v.e_cap, q.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<int> stack;                                 // the walk of sz_debug_tree
    int n = 0;
    stack.push_back(0);
    while (!stack.empty()) {
        const int ed = stack.back(); stack.pop_back();
        if (n < max_nodes && sq_sum) sq_sum[n] = q[ed];
        n++;
        if (em[ed].first >= 0) for (int k = (int)em[ed].n - 1; k >= 0; k--) stack.push_back(em[ed].first + k);
    }
    *n_out = n;
    return SZ_OK;
}

int sz_set_gumbel(sz_engine* e, const sz_gumbel_options* opt, const double* g_dev, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (opt) {
        if (opt->max_considered < 1 || opt->max_considered > SZ_MAX_MOVES) return SZ_ERR_INVALID;
        if (!std::isfinite(opt->c_visit) || opt->c_visit < 0.0f || !std::isfinite(opt->c_scale) || opt->c_scale < 0.0f) return SZ_ERR_INVALID;
    }
    OptionState p = option_state(e);
    p.gumbel = opt != nullptr;
    const int refused = option_refusal(e, p);
    if (refused == SZ_ERR_INVALID) return refused;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    int rc = between_searches(e, s);
    if (rc) return rc;
    if (!opt) { e->next.gumbel_on = 0; e->next.gumbel_g = nullptr; e->next.gumbel_tree = 0; return SZ_OK; }      // ... and sz_set_gumbel_tree's flag goes with it
    if (refused) return refused;                                            // root noise is on: SZ_ERR_STATE, after the question whether the engine searches
    if (!e->go.stat) {                                                      // the first enabling call: the per-board outputs and the counters
        const size_t B = e->v.B;
        float* vh = nullptr; float* po = nullptr; double* vm = nullptr; double* wk = nullptr; unsigned long long* st = nullptr;
        if ((rc = dalloc(e, &vh, B)) || (rc = dalloc(e, &po, B * SZ_MAX_MOVES)) || (rc = dalloc(e, &vm, B)) || (rc = dalloc(e, &wk, B * SZ_MAX_MOVES)) ||
            (rc = dalloc(e, &st, B * 2))) return rc;
        HIPCHK(hipMemsetAsync(vh, 0, B * sizeof(float), s));
        HIPCHK(hipMemsetAsync(po, 0, B * SZ_MAX_MOVES * sizeof(float), s));
        HIPCHK(hipMemsetAsync(vm, 0, B * sizeof(double), s));
        HIPCHK(hipMemsetAsync(st, 0, B * 2 * sizeof(unsigned long long), s));
        HIPCHK(hipStreamSynchronize(s));
        e->go.vhat = vh; e->go.policy = po; e->go.vmix = vm; e->go.work = wk; e->go.stat = st;
    }
    e->next.gumbel = *opt; e->next.gumbel_g = g_dev; e->next.gumbel_on = 1;
    return SZ_OK;
}

int sz_fetch_gumbel(sz_engine* e, float* policy_target, double* v_mix, float* root_value, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (!e->go.stat) return SZ_ERR_STATE;                                   // the option was never on
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    if (policy_target) HIPCHK(hipMemcpyAsync(policy_target, e->go.policy, B * SZ_MAX_MOVES * sizeof(float), hipMemcpyDeviceToHost, s));
    if (v_mix) HIPCHK(hipMemcpyAsync(v_mix, e->go.vmix, B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (root_value) HIPCHK(hipMemcpyAsync(root_value, e->go.vhat, B * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SZ_OK;
}

int sz_gumbel_stats(sz_engine* e, uint64_t out[2], void* stream) { return sum_board_counters(e, e ? e->go.stat : nullptr, 2, out, stream); }

int sz_set_gumbel_tree(sz_engine* e, int32_t enable, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    int rc = between_searches(e, s);
    if (rc) return rc;
    if (!enable) { e->next.gumbel_tree = 0; return SZ_OK; }
    if (!e->next.gumbel_on) return SZ_ERR_STATE;                            // the rule is a part of the Gumbel search
    if (!e->gt_stat) {                                                      // the first enabling call: the node values and the counter
        const size_t B = e->v.B;
        float* nv = nullptr; unsigned long long* st = nullptr;
        if ((rc = dalloc(e, &nv, B * e->v.n_cap)) || (rc = dalloc(e, &st, B))) return rc;
        HIPCHK(hipMemsetAsync(nv, 0, B * e->v.n_cap * sizeof(float), s));
        HIPCHK(hipMemsetAsync(st, 0, B * sizeof(unsigned long long), s));
        HIPCHK(hipStreamSynchronize(s));
        e->gt_nval = nv; e->gt_stat = st;
    }
    e->next.gumbel_tree = 1;
    return SZ_OK;
}

int sz_gumbel_tree_stats(sz_engine* e, uint64_t out[1], void* stream) { return sum_board_counters(e, e ? e->gt_stat : nullptr, 1, out, stream); }

int sz_forced_stats(sz_engine* e, uint64_t out[2], void* stream) { return sum_board_counters(e, e ? e->fo.stat : nullptr, 2, out, stream); }

int sz_set_endings(sz_engine* e, const sz_ending_options* opt, const uint8_t* holdout, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (opt) {
        if (!std::isfinite(opt->resign_value) || opt->resign_value < -1.0f || opt->resign_value > 1.0f) return SZ_ERR_INVALID;
        if (!std::isfinite(opt->draw_value) || opt->draw_value < 0.0f || opt->draw_value > 1.0f) return SZ_ERR_INVALID;
        if (opt->resign_patience < 0 || opt->resign_patience > END_STREAK_MAX || opt->draw_patience < 0 || opt->draw_patience > END_STREAK_MAX) return SZ_ERR_INVALID;
        if (opt->resign_min_ply < 0 || opt->draw_min_ply < 0) return SZ_ERR_INVALID;
    }
    OptionState p = option_state(e);
    p.endings = opt != nullptr;
    int rc = option_refusal(e, p);
    if (rc) return rc;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = between_searches(e, s))) return rc;
    if (!opt) { e->end_on = 0; return SZ_OK; }
    const size_t B = e->v.B;
    if (!e->eo.state) {                                                     // the first enabling call: state, flags, last-play readouts, counters
        EndState* st = nullptr; uint8_t* ho = nullptr; uint8_t* kd = nullptr; double* mv = nullptr; unsigned long long* ct = nullptr;
        if ((rc = dalloc(e, &st, B)) || (rc = dalloc(e, &ho, B)) || (rc = dalloc(e, &kd, B)) || (rc = dalloc(e, &mv, B)) || (rc = dalloc(e, &ct, B * 4))) return rc;
        HIPCHK(hipMemsetAsync(ct, 0, B * 4 * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_reset_endings, dim3((e->v.B + 255) / 256), dim3(256), 0, s, st, (const uint8_t*)nullptr, e->v.B, -1);
        HIPCHK(hipGetLastError());
        e->eo.holdout = ho; e->eo.kind = kd; e->eo.mval = mv; e->eo.stat = ct; e->eo.state = st;
    }
    if (!e->end_on) {                                                       // off -> on: no sz_play of the option to describe yet
        HIPCHK(hipMemsetAsync(e->eo.kind, 0, B, s));
        HIPCHK(hipMemsetAsync(e->eo.mval, 0xff, B * sizeof(double), s));    // all ones: a NaN
    }
    std::vector<uint8_t> h(B, 0);
    if (holdout) for (size_t b = 0; b < B; b++) h[b] = holdout[b] ? 1 : 0;
    HIPCHK(hipMemcpyAsync((void*)e->eo.holdout, h.data(), B, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                                        // the staging array goes out of scope
    e->eo.o = *opt;
    e->end_on = 1;
    return SZ_OK;
}

int sz_fetch_endings(sz_engine* e, uint8_t* kind, double* mover_value, int32_t* would_ply, uint8_t* would_kind, uint8_t* would_colour, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    std::vector<EndState> st;
    if (e->eo.state) {
        st.resize(B);
        HIPCHK(hipMemcpyAsync(st.data(), e->eo.state, B * sizeof(EndState), hipMemcpyDeviceToHost, s));
    }
    if (e->end_on) {
        if (kind) HIPCHK(hipMemcpyAsync(kind, e->eo.kind, B, hipMemcpyDeviceToHost, s));
        if (mover_value) HIPCHK(hipMemcpyAsync(mover_value, e->eo.mval, B * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    for (size_t b = 0; b < B; b++) {
        if (!e->end_on) { if (kind) kind[b] = SZ_END_NONE; if (mover_value) mover_value[b] = std::nan(""); }
        if (would_ply) would_ply[b] = st.empty() ? -1 : st[b].would_ply;
        if (would_kind) would_kind[b] = (uint8_t)(st.empty() ? 0 : st[b].would_kind);
        if (would_colour) would_colour[b] = (uint8_t)(st.empty() ? 0 : st[b].would_colour);
    }
    return SZ_OK;
}

int sz_ending_stats(sz_engine* e, uint64_t out[4], void* stream) { return sum_board_counters(e, e ? e->eo.stat : nullptr, 4, out, stream); }

int sz_set_move_temperature(sz_engine* e, const sz_temperature_options* opt, const double* temps_dev, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    if (opt) {
        if (!temps_dev) return SZ_ERR_INVALID;
        if (!std::isfinite(opt->visit_offset)) return SZ_ERR_INVALID;
        if (opt->use_cutoff && (!std::isfinite(opt->value_cutoff) || opt->value_cutoff < 0.0f)) return SZ_ERR_INVALID;
    }
    OptionState p = option_state(e);
    p.temperature = opt != nullptr;
    int rc = option_refusal(e, p);
    if (rc) return rc;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = between_searches(e, s))) return rc;
    if (!opt) { e->temp_on = 0; return SZ_OK; }
    const size_t B = e->v.B;
    if (!e->to.stat) {                                                      // the first enabling call: the weights, last-play readouts, counters
        double* wk = nullptr; int* ne = nullptr; double* pc = nullptr; unsigned long long* ct = nullptr;
        if ((rc = dalloc(e, &wk, B * SZ_MAX_MOVES)) || (rc = dalloc(e, &ne, B)) || (rc = dalloc(e, &pc, B)) || (rc = dalloc(e, &ct, B * 3))) return rc;
        HIPCHK(hipMemsetAsync(ct, 0, B * 3 * sizeof(unsigned long long), s));
        e->to.work = wk; e->to.nelig = ne; e->to.pch = pc; e->to.stat = ct;
    }
    if (!e->temp_on) {                                                      // off -> on: no sz_play of the option to describe yet
        HIPCHK(hipMemsetAsync(e->to.nelig, 0, B * sizeof(int), s));
        HIPCHK(hipMemsetAsync(e->to.pch, 0xff, B * sizeof(double), s));     // all ones: a NaN
    }
    e->to.o = *opt;
    e->to.o.use_cutoff = opt->use_cutoff ? 1 : 0;
    if (!e->to.o.use_cutoff) e->to.o.value_cutoff = 0.0f;
    e->to.temps = temps_dev;
    e->temp_on = 1;
    return SZ_OK;
}

int sz_fetch_temperature(sz_engine* e, int32_t* n_eligible, double* p_chosen, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    if (e->temp_on) {
        if (n_eligible) HIPCHK(hipMemcpyAsync(n_eligible, e->to.nelig, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (p_chosen) HIPCHK(hipMemcpyAsync(p_chosen, e->to.pch, B * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (!e->temp_on)
        for (size_t b = 0; b < B; b++) { if (n_eligible) n_eligible[b] = 0; if (p_chosen) p_chosen[b] = std::nan(""); }
    return SZ_OK;
}

int sz_temperature_stats(sz_engine* e, uint64_t out[3], void* stream) { return sum_board_counters(e, e ? e->to.stat : nullptr, 3, out, stream); }

int sz_pending_boards(sz_engine* e, int32_t* n_out, void* stream) {
    if (!e || !n_out) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_count_pending, dim3(1), dim3(1024), 0, s, e->v, e->d_nlive);
    HIPCHK(hipGetLastError());
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, e->d_nlive, sizeof n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_out = n;
    return SZ_OK;
}

int sz_get_stats(sz_engine* e, sz_stats* out, void* stream) {
    if (!e || !out) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    std::vector<Ctl> h(e->v.B);
    HIPCHK(hipMemcpyAsync(h.data(), e->v.ctl, h.size() * sizeof(Ctl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    for (const Ctl& c : h) {
        out->expansions += c.n_expand; out->terminal_hits += c.n_term; out->sum_depth += c.sum_depth; out->sum_children += c.sum_k;
        if ((uint64_t)c.max_edges > out->max_edges_used) out->max_edges_used = c.max_edges;
        if (c.status & ST_PENDING) out->boards_pending++;
        if (c.status & ST_DONE) out->boards_done++;
        if (c.status & ST_ERROR) { out->boards_error++; if (!out->first_error) out->first_error = c.err; }
    }
    out->simulations = out->expansions + out->terminal_hits;
    return SZ_OK;
}

int sz_root_children(sz_engine* e, int32_t* action_dev, int32_t* visits_dev, int32_t* n_child_dev, float* prior_dev, double* value_sum_dev, void* stream) {
    if (!e || !action_dev || !visits_dev || !n_child_dev) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipLaunchKernelGGL(k_root_children, dim3(e->v.B), dim3(64), 0, (hipStream_t)stream, e->v, action_dev, visits_dev, n_child_dev, prior_dev, value_sum_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_play(sz_engine* e, const double* uniforms_dev, void* stream) {
    if (!e || !uniforms_dev) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    e->search_open = 0;
    if (e->sum_on)                                                          // sz_set_search_summary: while the tree is intact
        hipLaunchKernelGGL(k_summary_pre, dim3(e->v.B), dim3(64), 0, (hipStream_t)stream, e->v, e->so);
    with_search_options(e, [&](auto, auto solve, auto... o) {
        auto launch = [&](auto... k) {
            hipLaunchKernelGGL((k_play<decltype(solve)::value, decltype(k)...>), dim3(e->v.B), dim3(64), e->lds_bytes, (hipStream_t)stream, e->v, uniforms_dev, k...);
        };
        // first-play urgency acts in the descent alone; the exploration rate reaches k_play for pruning alone, so only beside ForcedOpts
        if constexpr (has_opt<ForcedOpts, decltype(o)...>) std::apply(launch, pick<ForcedOpts, GumbelOpts, PuctOpts, TempOpts, EndOpts, LcbOpts>(play_opt(o)...));
        else std::apply(launch, pick<ForcedOpts, GumbelOpts, TempOpts, EndOpts, LcbOpts>(play_opt(o)...));
    });
    if (e->sum_on)                                                          // ... and when the ply's record exists
        hipLaunchKernelGGL(k_summary_post, dim3(e->v.B), dim3(64), 0, (hipStream_t)stream, e->v, e->so);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_play_moves(sz_engine* e, const int32_t* actions_dev, void* stream) {
    if (!e || !actions_dev) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    e->search_open = 0;
    hipLaunchKernelGGL(k_play_moves, dim3(e->v.B), dim3(64), e->lds_bytes, (hipStream_t)stream, e->v, actions_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_fetch_ply(sz_engine* e, uint8_t* packed_planes, int32_t* action, int32_t* visits, int32_t* n_child, uint8_t* colour, int32_t* chosen,
                 uint8_t* game_over, int8_t* result, uint8_t* active, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    const View& v = e->v;
    if (packed_planes) HIPCHK(hipMemcpyAsync(packed_planes, v.rec_planes, B * SZ_NUM_PLANES * 8, hipMemcpyDeviceToHost, s));
    if (action) HIPCHK(hipMemcpyAsync(action, v.rec_action, B * SZ_MAX_CHILDREN * 4, hipMemcpyDeviceToHost, s));
    if (visits) HIPCHK(hipMemcpyAsync(visits, v.rec_visits, B * SZ_MAX_CHILDREN * 4, hipMemcpyDeviceToHost, s));
    if (n_child) HIPCHK(hipMemcpyAsync(n_child, v.rec_nchild, B * 4, hipMemcpyDeviceToHost, s));
    if (colour) HIPCHK(hipMemcpyAsync(colour, v.rec_colour, B, hipMemcpyDeviceToHost, s));
    if (chosen) HIPCHK(hipMemcpyAsync(chosen, v.rec_chosen, B * 4, hipMemcpyDeviceToHost, s));
    if (game_over) HIPCHK(hipMemcpyAsync(game_over, v.rec_over, B, hipMemcpyDeviceToHost, s));
    if (result) HIPCHK(hipMemcpyAsync(result, v.rec_result, B, hipMemcpyDeviceToHost, s));
    if (active) HIPCHK(hipMemcpyAsync(active, v.rec_active, B, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SZ_OK;
}

int sz_debug_pending(sz_engine* e, uint64_t* mask, int32_t* depth, int32_t* n_nodes, int32_t* n_edges, int32_t* status, void* stream) {
    if (!e) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = e->v.B;
    std::vector<Ctl> h(B);
    std::vector<u64> pm(mask ? B * PMASK_STRIDE : 0);
    HIPCHK(hipMemcpyAsync(h.data(), e->v.ctl, B * sizeof(Ctl), hipMemcpyDeviceToHost, s));
    if (mask) HIPCHK(hipMemcpyAsync(pm.data(), e->v.pmask, pm.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t b = 0; b < B; b++) {
        if (depth) depth[b] = h[b].pend_depth;
        if (n_nodes) n_nodes[b] = h[b].n_nodes;
        if (n_edges) n_edges[b] = h[b].n_edges;
        if (status) status[b] = h[b].status;
        if (mask) memcpy(mask + b * SZ_MASK_WORDS, pm.data() + b * PMASK_STRIDE, SZ_MASK_WORDS * 8);
    }
    return SZ_OK;
}

int sz_debug_position(sz_engine* e, int32_t board, void* pos_out, int32_t* ply, void* stream) {
    if (!e || board < 0 || board >= e->v.B || !pos_out) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    Ctl c;
    HIPCHK(hipMemcpyAsync(&c, e->v.ctl + board, sizeof c, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpyAsync(pos_out, e->v.ring + (size_t)board * SZ_RING + (c.game_ply & (SZ_RING - 1)), sizeof(SzPos), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ply) *ply = c.game_ply;
    return SZ_OK;
}

int sz_debug_tree(sz_engine* e, int32_t board, int32_t max_nodes, int32_t* depth, int32_t* action, int32_t* visits, double* value_sum,
                  float* prior, int32_t* n_out, void* stream) {
    if (!e || board < 0 || board >= e->v.B || !n_out) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    Ctl c;
    HIPCHK(hipMemcpyAsync(&c, e->v.ctl + board, sizeof c, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_out = 0;
    if (!(c.status & ST_SEARCHING) || c.n_edges <= 0) return SZ_OK;
    std::vector<EdgeStat> es(c.n_edges);
    std::vector<EdgeMeta> em(c.n_edges);
    HIPCHK(hipMemcpyAsync(es.data(), e->v.es + (size_t)board * e->v.e_cap, es.size() * sizeof(EdgeStat), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(em.data(), e->v.em + (size_t)board * e->v.e_cap, em.size() * sizeof(EdgeMeta), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // depth-first in child order = the order a recursive walk over Node.children visits the reference's tree; edge 0 is the root itself
    std::vector<std::pair<int, int>> stack;                // (edge, depth)
    int n = 0;
    if (max_nodes > 0 && depth) { depth[0] = -1; action[0] = -1; visits[0] = es[0].N; value_sum[0] = es[0].W; prior[0] = es[0].P; }
    n = 1;
    for (int k = (int)em[0].n - 1; k >= 0 && em[0].first >= 0; k--) stack.push_back({em[0].first + k, 0});
    while (!stack.empty()) {
        auto [ed, d] = stack.back(); stack.pop_back();
        if (n < max_nodes && depth) { depth[n] = d; action[n] = em[ed].action; visits[n] = es[ed].N; value_sum[n] = es[ed].W; prior[n] = es[ed].P; }
        n++;
        if (em[ed].first >= 0) for (int k = (int)em[ed].n - 1; k >= 0; k--) stack.push_back({em[ed].first + k, d + 1});
    }
    *n_out = n;
    return SZ_OK;
}

int sz_debug_tree_proven(sz_engine* e, int32_t board, int32_t max_nodes, int8_t* proven, uint8_t* complete, int32_t* n_out, void* stream) {
    if (!e || board < 0 || board >= e->v.B || !n_out) return SZ_ERR_INVALID;
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    Ctl c;
    HIPCHK(hipMemcpyAsync(&c, e->v.ctl + board, sizeof c, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_out = 0;
    if (!(c.status & ST_SEARCHING) || c.n_edges <= 0) return SZ_OK;
    std::vector<EdgeMeta> em(c.n_edges);
    HIPCHK(hipMemcpyAsync(em.data(), e->v.em + (size_t)board * e->v.e_cap, em.size() * sizeof(EdgeMeta), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<int> stack;                                 // the walk of sz_debug_tree
    int n = 0;
    stack.push_back(0);
    while (!stack.empty()) {
        const int ed = stack.back(); stack.pop_back();
        if (n < max_nodes && proven) proven[n] = (int8_t)(em[ed].pad & PR_MASK);
        if (n < max_nodes && complete) complete[n] = (uint8_t)((em[ed].pad & PR_COMPLETE) ? 1 : 0);
        n++;
        if (em[ed].first >= 0) for (int k = (int)em[ed].n - 1; k >= 0; k--) stack.push_back(em[ed].first + k);
    }
    *n_out = n;
    return SZ_OK;
}

int sz_debug_tree_values(sz_engine* e, int32_t board, int32_t max_nodes, float* node_value, int32_t* n_out, void* stream) {
    if (!e || board < 0 || board >= e->v.B || !n_out) return SZ_ERR_INVALID;
    if (!e->gt_nval || !e->cur.gumbel_tree) return SZ_ERR_STATE;            // the search begun last kept no node values
    ENGINE_GUARD(e);
    hipStream_t s = (hipStream_t)stream;
    Ctl c;
    HIPCHK(hipMemcpyAsync(&c, e->v.ctl + board, sizeof c, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_out = 0;
    if (!(c.status & ST_SEARCHING) || c.n_edges <= 0) return SZ_OK;
    std::vector<EdgeMeta> em(c.n_edges);
    std::vector<float> nv(e->v.n_cap);
    HIPCHK(hipMemcpyAsync(em.data(), e->v.em + (size_t)board * e->v.e_cap, em.size() * sizeof(EdgeMeta), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(nv.data(), e->gt_nval + (size_t)board * e->v.n_cap, nv.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<int> stack;                                 // the walk of sz_debug_tree
    int n = 0;
    stack.push_back(0);
    while (!stack.empty()) {
        const int ed = stack.back(); stack.pop_back();
        // a node is expanded exactly when its edge has a child span; its value was stored then.  Unvisited, terminal and pending nodes: NaN
        const bool expanded = em[ed].first >= 0 && em[ed].node >= 0 && em[ed].node < e->v.n_cap;
        if (n < max_nodes && node_value) node_value[n] = expanded ? nv[em[ed].node] : std::numeric_limits<float>::quiet_NaN();
        n++;
        if (em[ed].first >= 0) for (int k = (int)em[ed].n - 1; k >= 0; k--) stack.push_back(em[ed].first + k);
    }
    *n_out = n;
    return SZ_OK;
}

int sz_debug_select(const int32_t* offsets_dev, const int32_t* vc_dev, const double* value_sum_dev, const float* prior_dev, const int32_t* parent_visits_dev,
                    const float* c_dev, float* ucb_out_dev, int32_t* argmax_out_dev, int32_t n_cases, void* stream) {
    if (!offsets_dev || !vc_dev || !value_sum_dev || !prior_dev || !parent_visits_dev || !c_dev || !ucb_out_dev || !argmax_out_dev || n_cases <= 0) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_select, dim3(n_cases), dim3(64), SZ_MAX_CHILDREN * sizeof(EdgeStat), (hipStream_t)stream, offsets_dev, vc_dev, value_sum_dev,
                       prior_dev, parent_visits_dev, c_dev, ucb_out_dev, argmax_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_forced(const int32_t* offsets_dev, const int32_t* vc_dev, const int32_t* inflight_dev, const double* value_sum_dev, const float* prior_dev,
                    const int8_t* proven_dev, const int32_t* parent_visits_dev, const float* c_dev, const float* forced_k_dev, float virtual_loss,
                    int32_t* selected_out_dev, int32_t* forced_out_dev, int32_t* pruned_out_dev, int32_t* cstar_out_dev, int32_t n_cases, void* stream) {
    if (!offsets_dev || !vc_dev || !inflight_dev || !value_sum_dev || !prior_dev || !parent_visits_dev || !c_dev || !forced_k_dev || !selected_out_dev ||
        !forced_out_dev || !pruned_out_dev || !cstar_out_dev || n_cases <= 0) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_forced, dim3(n_cases), dim3(64), SZ_MAX_CHILDREN * (sizeof(EdgeStat) + sizeof(EdgeMeta) + 2 * sizeof(int)), (hipStream_t)stream,
                       offsets_dev, vc_dev, inflight_dev, value_sum_dev, prior_dev, proven_dev, parent_visits_dev, c_dev, forced_k_dev, virtual_loss,
                       selected_out_dev, forced_out_dev, pruned_out_dev, cstar_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_select_fpu(const int32_t* offsets_dev, const int32_t* vc_dev, const int32_t* inflight_dev, const double* value_sum_dev, const float* prior_dev,
                        const int8_t* proven_dev, const int32_t* parent_visits_dev, const int32_t* parent_n_dev, const double* parent_w_dev, const float* c_dev,
                        const int32_t* is_root_dev, const sz_fpu_options* opts_dev, float virtual_loss, float* ucb_out_dev, int32_t* selected_out_dev,
                        int32_t n_cases, void* stream) {
    if (!offsets_dev || !vc_dev || !inflight_dev || !value_sum_dev || !prior_dev || !parent_visits_dev || !parent_n_dev || !parent_w_dev || !c_dev || !is_root_dev ||
        !opts_dev || !ucb_out_dev || !selected_out_dev || n_cases <= 0) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_select_fpu, dim3(n_cases), dim3(64), SZ_MAX_CHILDREN * (sizeof(EdgeStat) + sizeof(EdgeMeta) + sizeof(int)), (hipStream_t)stream,
                       offsets_dev, vc_dev, inflight_dev, value_sum_dev, prior_dev, proven_dev, parent_visits_dev, parent_n_dev, parent_w_dev, c_dev, is_root_dev,
                       opts_dev, virtual_loss, ucb_out_dev, selected_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_gumbel(const double* x_dev, double* slog_out_dev, double* sexp_out_dev, const int32_t* tnm_dev, int32_t* level_out_dev,
                    const int32_t* offsets_dev, const int32_t* vc_dev, const double* value_sum_dev, const float* prior_dev, const double* g_dev,
                    const int32_t* visit_dev, const int32_t* goal_dev, const float* root_value_dev, const sz_gumbel_options* opts_dev,
                    int32_t* selected_out_dev, int32_t* fallback_out_dev, int32_t* final_out_dev, float* policy_out_dev, double* v_mix_out_dev,
                    int32_t n_cases, void* stream) {
    if (n_cases <= 0 || (!x_dev && !tnm_dev && !offsets_dev)) return SZ_ERR_INVALID;
    if (x_dev && (!slog_out_dev || !sexp_out_dev)) return SZ_ERR_INVALID;
    if (tnm_dev && !level_out_dev) return SZ_ERR_INVALID;
    if (offsets_dev && (!vc_dev || !value_sum_dev || !prior_dev || !visit_dev || !goal_dev || !root_value_dev || !opts_dev || !selected_out_dev || !fallback_out_dev ||
                        !final_out_dev || !policy_out_dev || !v_mix_out_dev)) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_gumbel, dim3(n_cases), dim3(64), SZ_MAX_CHILDREN * (sizeof(EdgeStat) + sizeof(double) + sizeof(float)), (hipStream_t)stream,
                       x_dev, slog_out_dev, sexp_out_dev, tnm_dev, level_out_dev, offsets_dev, vc_dev, value_sum_dev, prior_dev, g_dev, visit_dev, goal_dev,
                       root_value_dev, opts_dev, selected_out_dev, fallback_out_dev, final_out_dev, policy_out_dev, v_mix_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_lcb(const double* x_dev, double* ssqrt_out_dev, int32_t* x_bad_out_dev, int32_t n_x, const int32_t* offsets_dev, const int32_t* vc_dev,
                 const int32_t* tree_vc_dev, const double* value_sum_dev, const double* sq_sum_dev, const sz_lcb_options* opts_dev, int32_t* move_out_dev,
                 int32_t* cstar_out_dev, int32_t* n_candidates_out_dev, int32_t* bad_out_dev, double* lcb_out_dev, int32_t n_cases, void* stream) {
    if (!x_dev && !offsets_dev) return SZ_ERR_INVALID;
    if (x_dev && (!ssqrt_out_dev || n_x <= 0)) return SZ_ERR_INVALID;
    if (offsets_dev && (n_cases <= 0 || !vc_dev || !tree_vc_dev || !value_sum_dev || !sq_sum_dev || !opts_dev || !move_out_dev || !cstar_out_dev ||
                        !n_candidates_out_dev || !bad_out_dev || !lcb_out_dev)) return SZ_ERR_INVALID;
    if (x_dev) hipLaunchKernelGGL(k_debug_ssqrt, dim3((n_x + 63) / 64), dim3(64), 0, (hipStream_t)stream, x_dev, ssqrt_out_dev, x_bad_out_dev, n_x);
    if (offsets_dev)
        hipLaunchKernelGGL(k_debug_lcb, dim3(n_cases), dim3(64), SZ_MAX_CHILDREN * (sizeof(EdgeStat) + sizeof(int)), (hipStream_t)stream, offsets_dev, vc_dev, tree_vc_dev,
                           value_sum_dev, sq_sum_dev, opts_dev, move_out_dev, cstar_out_dev, n_candidates_out_dev, bad_out_dev, lcb_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_cpuct(const int32_t* n_p_dev, const uint8_t* is_root_dev, const sz_cpuct_options* opts_dev, float* c_out_dev, int32_t n_cases, void* stream) {
    if (!n_p_dev || !is_root_dev || !opts_dev || !c_out_dev || n_cases <= 0) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_cpuct, dim3((n_cases + 63) / 64), dim3(64), 0, (hipStream_t)stream, n_p_dev, is_root_dev, opts_dev, c_out_dev, n_cases);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_kld_gain(const int32_t* prev_dev, const int32_t* now_dev, const int32_t* n_child_dev, double* gain_out_dev, int32_t n_cases, void* stream) {
    if (!prev_dev || !now_dev || !n_child_dev || !gain_out_dev || n_cases <= 0) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_kld_gain, dim3(n_cases), dim3(64), 0, (hipStream_t)stream, prev_dev, now_dev, n_child_dev, gain_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_search_summary(const int32_t* n_child_dev, const int32_t* tree_vc_dev, const double* value_sum_dev, const float* prior_dev, const int32_t* record_vc_dev,
                            double* out3_dev, int32_t n_cases, void* stream) {
    if (!n_child_dev || !tree_vc_dev || !value_sum_dev || !prior_dev || !record_vc_dev || !out3_dev || n_cases <= 0) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_search_summary, dim3(n_cases), dim3(64), 0, (hipStream_t)stream, n_child_dev, tree_vc_dev, value_sum_dev, prior_dev, record_vc_dev, out3_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_gumbel_tree(const int32_t* offsets_dev, const int32_t* vc_dev, const double* value_sum_dev, const float* prior_dev, const float* node_value_dev,
                         const sz_gumbel_options* opts_dev, double* score_out_dev, int32_t* selected_out_dev, double* v_mix_out_dev, int32_t n_cases, void* stream) {
    if (n_cases <= 0 || !offsets_dev || !vc_dev || !value_sum_dev || !prior_dev || !node_value_dev || !opts_dev || !score_out_dev || !selected_out_dev ||
        !v_mix_out_dev) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_gumbel_tree, dim3(n_cases), dim3(64), SZ_MAX_CHILDREN * sizeof(EdgeStat), (hipStream_t)stream,
                       offsets_dev, vc_dev, value_sum_dev, prior_dev, node_value_dev, opts_dev, score_out_dev, selected_out_dev, v_mix_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_endings(const int32_t* offsets_dev, const int32_t* vc_dev, const double* value_sum_dev, const int8_t* root_proven_dev, const uint8_t* colour_dev,
                     const int32_t* ply_dev, const uint8_t* holdout_dev, const int32_t* state_in_dev, const sz_ending_options* opts_dev,
                     int32_t* kind_out_dev, double* m_out_dev, int32_t* state_out_dev, int32_t n_cases, void* stream) {
    if (!offsets_dev || !vc_dev || !value_sum_dev || !root_proven_dev || !colour_dev || !ply_dev || !holdout_dev || !state_in_dev || !opts_dev ||
        !kind_out_dev || !m_out_dev || !state_out_dev || n_cases <= 0) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_endings, dim3(n_cases), dim3(64), SZ_MAX_CHILDREN * sizeof(EdgeStat), (hipStream_t)stream,
                       offsets_dev, vc_dev, value_sum_dev, root_proven_dev, colour_dev, ply_dev, holdout_dev, state_in_dev, opts_dev,
                       kind_out_dev, m_out_dev, state_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

int sz_debug_temperature(const int32_t* offsets_dev, const int32_t* vc_dev, const int32_t* tree_vc_dev, const double* value_sum_dev, const double* temps_dev,
                         const double* uniforms_dev, const int32_t* proven_move_dev, const sz_temperature_options* opts_dev, int32_t* chosen_out_dev,
                         int32_t* kind_out_dev, int32_t* n_eligible_out_dev, double* p_chosen_out_dev, int32_t* excluded_out_dev, double* weights_out_dev,
                         int32_t n_cases, void* stream) {
    if (!offsets_dev || !vc_dev || !value_sum_dev || !temps_dev || !uniforms_dev || !opts_dev || !chosen_out_dev || !kind_out_dev || !n_eligible_out_dev ||
        !p_chosen_out_dev || !excluded_out_dev || !weights_out_dev || n_cases <= 0) return SZ_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_temperature, dim3(n_cases), dim3(64), SZ_MAX_CHILDREN * (sizeof(EdgeStat) + sizeof(int)), (hipStream_t)stream,
                       offsets_dev, vc_dev, tree_vc_dev, value_sum_dev, temps_dev, uniforms_dev, proven_move_dev, opts_dev, chosen_out_dev, kind_out_dev,
                       n_eligible_out_dev, p_chosen_out_dev, excluded_out_dev, weights_out_dev);
    HIPCHK(hipGetLastError());
    return SZ_OK;
}

}  // extern "C"
