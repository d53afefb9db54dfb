/* sigmazero.h — C ABI of the MI355X-native batched MCTS self-play engine.
 *
 * The reference (DidItWork/Sigma-Zero) has NO native/FFI layer: its boundary for this path is the
 * Python call surface.  This header is therefore the boundary a maintainer binds
 * from Python with ctypes (INTEGRATION.md shows the stub); every entry point names the reference
 * code it replaces.  Plain pointers and sizes only — no torch types.
 *
 * Conventions: every function returns SZ_OK (0) or a negative SZ_ERR_*; the engine owns all of its
 * device memory; tensors handed in by pointer stay owned by the caller; all device work is enqueued
 * on the caller's stream (pass torch.cuda.current_stream().cuda_stream), which must belong to the
 * engine's device (sz_config.device); every call makes that device current for its duration and
 * restores the caller's current device; not thread-safe.  "All device work" means launches, copies,
 * fills and the waits in front of host reads alike.  tests/test_gpu_stream_contract.py holds every
 * entry point to that on a non-default stream, bit for bit.  One engine per GPU per process is the usual
 * arrangement (self-play fills the card with one), a usage note and not a constraint: engines share
 * nothing, and several may live side by side on one device (arena.play_options_match
 * holds two).  Give each an explicit edges_per_board then: the default sizes the first one to half of the
 * free HBM.  The network launches (sz_nn_*) do keep state per device and process: the persistent tower's
 * pacing counters, the function-attribute flags and the stamp pointers of the diagnostic builds.  It is
 * safe in program order on one stream at a time; two streams with network launches in flight at once are
 * not supported.
 */
#ifndef SIGMAZERO_H
#define SIGMAZERO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SZ_RING 256              /* per-game position history kept for repetition / history planes */
#define SZ_PLANES 119            /* chess_tensor.py:31-35  M*T+L = 14*8+7 */
#define SZ_ACTIONS 4672          /* 73*8*8, chess_tensor.py:197 */
#define SZ_MAX_MOVES 218
#define SZ_POS_BYTES 80

enum {
    SZ_OK = 0,
    SZ_ERR_INVALID = -1,         /* bad argument / illegal move (ValueError("Invalid move"), chess_tensor.py:91-92) */
    SZ_ERR_HIP = -2,             /* a HIP runtime call failed */
    SZ_ERR_CAPACITY = -3,        /* a board ran out of child slots (edges_per_board too small) */
    SZ_ERR_NO_DEVICE = -4,       /* no MI355X visible: the product path never falls back to the CPU */
    SZ_ERR_STATE = -5,           /* call sequence violated (e.g. step before begin) */
    SZ_ERR_ZERO_VISITS = -6      /* num_searches == 1: the reference raises ZeroDivisionError (mcts.py:118-120) */
};

/* network-input layouts written by the engine:
 *   F32 / BF16     : [n_boards,119,8,8] NCHW, the reference's get_representation() layout
 *   NHWC128_BF16   : [n_boards,64,128] position-major, channels 119..127 zero — input of sz_nn_conv_bf16 (stem)
 *   NHWC128_BITS   : the same image bit-packed, 1 KiB per board (16x fewer bytes than bf16): [n_boards][64 lanes] uint4,
 *                    lane l = psub*16 + cq; byte q (little-endian) of its 16 bytes holds channels cq*8..cq*8+7 (bit k =
 *                    channel cq*8+k) of position q*4 + psub.  Consumed by the stem with SZ_NN_IN_BITS. */
enum { SZ_PLANES_F32 = 0, SZ_PLANES_BF16 = 1, SZ_PLANES_NHWC128_BF16 = 2, SZ_PLANES_NHWC128_BITS = 3 };

/* ------------------------------------------------------------------ engine (HIP, gfx950) */

typedef struct sz_engine sz_engine;

typedef struct sz_config {
    int32_t n_boards;            /* concurrent self-play boards on this GPU */
    int32_t num_searches;        /* args['num_searches'], mcts.py:49 */
    float   c_puct;              /* args['C'], mctsnode.py:37 */
    int32_t learning;            /* search(..., learning=...), mcts.py:91 */
    float   noise_value;         /* value of the degenerate Dirichlet draw of mcts.py:93 (1-2^-24 under torch 2.10) */
    int32_t chess960;            /* boards spell castling king-takes-rook (chess.Board(chess960=True)) */
    int32_t edges_per_board;     /* child slots per board per search; 0 = worst case num_searches*218+2 when that fits in half of the free
                                  * HBM (no position can overflow), else what fits, at least num_searches*64+256 */
    int32_t planes_dtype;        /* SZ_PLANES_F32 / SZ_PLANES_BF16: element type of the network input */
    int32_t device;              /* HIP device ordinal */
    int32_t reuse_subtree;       /* NON-REFERENCE option, 0 = off (default, the reference builds a fresh tree per ply: sim.py:53).  != 0: sz_play keeps the
                                  * subtree below the move it plays (compacted in place) and the next sz_search_begin continues on it — the new root starts
                                  * with that child's visit count, value sum and children — whenever the kept part is at most num_searches nodes and half
                                  * of the child slots; otherwise, and after sz_new_games / sz_upload_game, the search starts fresh.  Doubles the stores.
                                  * The search starts from a fresh root (visit count 1, no children) exactly when
                                  *  (1) the chosen child was never visited, or was visited and has no children (then it is a terminal position);
                                  *  (2) the kept subtree has more than num_searches visited nodes, the new root included;
                                  *  (3) twice its edge count, the new root's own edge included, exceeds the child slots per board
                                  *      (edges_per_board, at least 220).
                                  * A continued search makes num_searches new simulations: it descends first (nothing waits for the network at
                                  * sz_search_begin's return but the first new leaf), the root keeps the kept visit count and is not expanded again.
                                  * Held to a re-rooted host search by tests/test_gpu_subtree_reuse.py (tests/reuseref.py). */
} sz_config;

typedef struct sz_stats {
    uint64_t simulations;        /* executions of the mcts.py:49 loop body, all boards */
    uint64_t expansions;         /* non-terminal leaves evaluated by the network (mcts.py:66-102) */
    uint64_t terminal_hits;      /* simulations that ended in a terminal leaf (mcts.py:104-106) */
    uint64_t sum_depth;          /* sum of leaf depths (edges from the root) */
    uint64_t sum_children;       /* sum of K over expansions */
    uint64_t max_edges_used;     /* high-water mark of child slots on any board */
    int32_t  boards_pending;     /* boards waiting for a network evaluation */
    int32_t  boards_done;        /* boards whose search finished */
    int32_t  boards_error;       /* boards with a sticky error flag */
    int32_t  first_error;        /* SZ_ERR_* of the first failing board, or 0 */
} sz_stats;

/* MCTS0.__init__ (mcts.py:30-37): allocate the SoA node store for n_boards trees. */
int sz_create(const sz_config* cfg, sz_engine** out);
int sz_destroy(sz_engine* e);

/* ChessTensor.__init__/start_board (chess_tensor.py:31-35,65-86) for every board with active[b] != 0
 * (NULL = all): scharnagl[b] >= 0 -> Board.from_chess960_pos(n), < 0 -> chess.Board().
 * Host arrays. */
int sz_new_games(sz_engine* e, const int32_t* scharnagl, const uint8_t* active, void* stream);

/* Put an arbitrary live game on one board: `ring` is the SZ_RING*SZ_POS_BYTES history exported by
 * szh_export (the root game object of mcts.py:43, which search() uses un-copied). */
int sz_upload_game(sz_engine* e, int32_t board, const void* ring, int32_t ply, void* stream);
/* mark boards (in)active for the next searches; host array of n_boards bytes */
int sz_set_active(sz_engine* e, const uint8_t* active, void* stream);

/* Batch compaction for ragged self-play (games of one call end at different plies, sim.py:46): with enable != 0 the boards that will
 * search next (active, game not over, no error) are numbered 0..n_live-1 in board order, and from then on board b reads its policy / value
 * from ROW slot(b) of policy_dev / value_dev and writes its network input to ROW slot(b) of planes_dev — so the network runs on n_live
 * rows instead of n_boards.  Call between searches, after sz_play / sz_new_games / sz_set_active changed the live set (synchronises the
 * stream to return n_live).  enable == 0 restores the identity mapping (row = board), the default.  Results per board do not depend on
 * the mapping.  Per-board outputs (sz_root_children, sz_fetch_ply, sz_play's uniforms) stay indexed by board.  A board that becomes live
 * without a new sz_compact has no row: sz_search_begin flags it SZ_ERR_STATE (sticky, sz_get_stats().first_error). */
int sz_compact(sz_engine* e, int32_t enable, int32_t* n_live_out, void* stream);

/* First half of MCTS0.search (mcts.py:43-75): create the roots (visit_count = 1), test them for
 * termination, and write the network input of every root into planes_dev [n_boards,119,8,8]. */
int sz_search_begin(sz_engine* e, void* planes_dev, void* stream);

/* One lock-step iteration over all boards: consume model(x, inference=True) for the pending leaves
 * (policy_dev [n_boards,4672] f32 probabilities, value_dev [n_boards] f32) = masked renormalise,
 * noise mix, Node.expand, Node.backpropagate (mcts.py:77-109, mctsnode.py:39-63); then run
 * Node.select (mctsnode.py:23-37) down to the next leaf of each board, play the move
 * (mcts.py:57-59), test termination (terminal leaves are backed up on the spot and selection
 * repeats), and encode the next network input into planes_dev. */
int sz_search_step(sz_engine* e, const float* policy_dev, const float* value_dev, void* planes_dev, void* stream);

/* Counters (synchronises the stream). */
int sz_get_stats(sz_engine* e, sz_stats* out, void* stream);

/* mcts.py:113-122 readout: for each board the root children in ascending action-index order.
 * Device pointers: action [n_boards,218] int32, visits [n_boards,218] int32, n_child [n_boards] int32;
 * optional (may be NULL) prior [n_boards,218] f32 and value_sum [n_boards,218] f64. */
int sz_root_children(sz_engine* e, int32_t* action_dev, int32_t* visits_dev, int32_t* n_child_dev,
                     float* prior_dev, double* value_sum_dev, void* stream);

/* sim.py:68-76: sample a move per board from the visit distribution exactly like
 * np.random.choice(keys, p=visits/sum) given the uniform it draws (uniforms_dev [n_boards] f64),
 * record the training sample of this ply, play the move into the board's game and test
 * board.is_game_over() (sim.py:46).  A negative uniform selects the most visited child instead
 * (max(action_probs, key=...) of eval.py:92-94 / play.py:40-41: first maximum in action-index order). */
int sz_play(sz_engine* e, const double* uniforms_dev, void* stream);

/* Play GIVEN moves, one per board: an opponent engine's, a book's, a person's (the role of the reference's play.py, which pushes the
 * human's move into the game: ChessTensor.move, chess_tensor.py:88-95).  actions_dev: device array [n_boards] int32; -1 leaves the board
 * alone, any other value is an action index 0..SZ_ACTIONS-1 to play on that board.  One launch, one wavefront per board, no
 * synchronisation.  SZ_ERR_INVALID: e or actions_dev NULL.  Per board, in this order:
 *   actions[b] < 0     nothing is touched: the record's `active` flag and a kept subtree stay as they are;
 *   game over, or a sticky error: nothing is touched;
 *   inside an unfinished search (between sz_search_begin and the search's last step): the board is flagged SZ_ERR_STATE, sticky, the
 *                      way sz_search_begin flags a board without a row.  Whether the board is active (sz_set_active) is NOT consulted and
 *                      is preserved: a caller may park the boards an engine does not search as inactive and still move on them;
 *   legality           the root position is the ring entry of the game's ply (what sz_search_begin takes).  The action must be a bit of the
 *                      legal-move mask move generation makes for it; it is not looked up among the root's children, because expansion drops
 *                      legal moves whose renormalised prior is exactly 0.  An illegal action, or one >= SZ_ACTIONS, flags the board
 *                      SZ_ERR_INVALID, sticky (ValueError("Invalid move"), chess_tensor.py:91-92); nothing else on the board changes;
 *   the move           is played as sz_play plays the one it chose: the new position goes to the ring slot of ply + 1, the game's ply
 *                      advances, the game-over test runs and sets the game's result.  The 80-byte position record and the ring are
 *                      byte-identical to what sz_play writes when it plays the same action.  The board's status keeps its active bit
 *                      alone (plus game over): a finished search is consumed, as by sz_play;
 *   the record         a given move is not a training sample: active[b] = 0.  chosen[b], game_over[b] and result[b] are written, so
 *                      sz_fetch_ply reports the game's end; visits, actions, n_child, colour and planes are left as they are;
 *   not touched        sz_play's uniforms, the ending streaks and marks of sz_set_endings, the counters of sz_forced_stats,
 *                      sz_solver_stats, sz_ending_stats and sz_get_stats: a given move is not a search of the mover;
 *   reuse_subtree      the board has a tree when a search has finished on it and was not yet consumed, or when an earlier sz_play /
 *                      sz_play_moves kept a subtree that no search has continued yet.  If the root child with this action exists, was
 *                      visited and has children, its subtree is kept with sz_play's own in-place compaction (solver labels and `complete`
 *                      bits travel with their edges) and the next sz_search_begin continues on it, under the three fresh-start conditions
 *                      of sz_config.reuse_subtree evaluated on what is kept now.  Otherwise nothing is kept and the next search starts
 *                      fresh: no tree, no such child (a move expansion dropped), an unvisited child, a leaf, a game that has ended.  So
 *                      sz_play followed by one sz_play_moves is a two-ply re-rooting: the next search continues on the grandchild's
 *                      subtree, which holds the engine's thinking about the reply.
 * Held to a host restatement by tests/test_gpu_play_moves.py (tests/playmovesref.py). */
int sz_play_moves(sz_engine* e, const int32_t* actions_dev, void* stream);

/* Copy this ply's training records to host arrays (synchronises; any pointer may be NULL):
 *  packed_planes [n_boards,119,8] uint8   root get_representation(), bit j of byte = column j
 *                                         (the (119,8) format of generate_training_supervised.py:91)
 *  action/visits [n_boards,218] int32, n_child [n_boards] int32        sim.py:72 'actions'
 *  colour [n_boards] uint8 (board.turn at the root, sim.py:73), chosen [n_boards] int32 (action index),
 *  game_over [n_boards] uint8, result [n_boards] int8 (+1 = '1-0', -1 = '0-1', 0 draw; sim.py:86-92),
 *  active [n_boards] uint8 (whether the record is valid for this ply). */
int sz_fetch_ply(sz_engine* e, uint8_t* packed_planes, int32_t* action, int32_t* visits, int32_t* n_child,
                 uint8_t* colour, int32_t* chosen, uint8_t* game_over, int8_t* result, uint8_t* active, void* stream);

/* NON-REFERENCE option, off by default: true AlphaZero root noise.  gamma_dev: device array [n_boards][SZ_MAX_MOVES]
 * f32 of Gamma(alpha,1) draws, read when a search's ROOT is expanded (the step after sz_search_begin): root prior k becomes
 * 0.75*p_k + 0.25*g_k/sum_{j<K} g_j (one Dirichlet(alpha) sample over the K legal moves); inner nodes get no noise.  NULL restores
 * the reference behaviour (mcts.py:91-98: the constant noise_value at every expansion).  Needs learning = 1.  Refused (SZ_ERR_STATE) on an engine created
 * with reuse_subtree: a reused root is never expanded again, the noise would silently reach the first ply of a game only; sz_set_search_root_noise
 * below noises kept roots as well and is the setter for such an engine. */
int sz_set_root_noise(sz_engine* e, const float* gamma_dev);

/* NON-REFERENCE option (default L = 1, lambda ignored): gather up to `leaves_per_step` leaves per board per
 * sz_search_step with virtual loss `virtual_loss`; network rows become n_rows * leaves_per_step, board b's
 * leaf i at row slot(b)*leaves_per_step + i.  Only between searches (SZ_ERR_STATE otherwise).
 * Per board and step: every leaf pending from the previous step is expanded and backed up in gather order; then descents
 * are made one after another until L leaves are pending or simulations done + pending == num_searches.  Every edge carries
 * an in-flight count k (kept apart from W / N); selection scores a child with visit count N + k and value sum W + lambda*k
 * (f64) under the parent term sqrt(N_parent + k_parent), otherwise exactly Node.get_ucb / Node.select.  A terminal leaf is
 * backed up on the spot; a new non-terminal leaf becomes pending (k + 1 along its path, network input at its row); a descent
 * that ends on a leaf already pending in this step (a collision) ends the gather.  A search takes at most num_searches steps
 * and counts the same simulations as at L = 1.  L = 1 is the reference's search, bit for bit (the same kernel).  L > 1 is NOT
 * the reference's search and is not held to its visit counts; its effect on playing strength is unmeasured.
 * SZ_ERR_INVALID: L < 1, L > SZ_MAX_LEAVES_PER_STEP, lambda negative or not finite, or L > 1 on an engine with reuse_subtree or while the
 * solver is on (sz_set_solver); those combinations are asked for through sz_set_search_options.
 * The buffers (in-flight counts, L paths and legal masks per board) are allocated by the first call with L > 1. */
#define SZ_MAX_LEAVES_PER_STEP 256
int sz_set_leaf_batching(sz_engine* e, int32_t leaves_per_step, float virtual_loss, void* stream);
/* number of boards still waiting for a network evaluation (synchronises the stream).  With leaf batching a search takes a
 * data-dependent number of steps (collisions end a gather early): step until this is 0. */
int sz_pending_boards(sz_engine* e, int32_t* n_out, void* stream);

/* NON-REFERENCE option (default: every board runs num_searches simulations, as the reference's one args['num_searches'] does): a search
 * budget per board.  budgets: HOST array [n_boards], each entry in 0..num_searches; NULL = every board num_searches again.  num_searches
 * stays the capacity the stores were sized for.  Takes effect at the next sz_search_begin and holds until changed.  A board with budget s
 * searches exactly like a board of an engine created with num_searches = s, bit for bit — s = 0 and a terminal root (N = 1 + s, W = tv*s),
 * SZ_ERR_ZERO_VISITS from sz_play at s = 1 and the counters of sz_get_stats included — with leaf batching as well (simulations done +
 * pending == s ends a gather).  This is playout-cap randomisation's engine half (KataGo: most plies searched cheaply, a random few
 * fully); the reference has nothing like it.
 * SZ_ERR_INVALID: an entry outside 0..num_searches, or budgets != NULL on an engine created with reuse_subtree (a kept subtree already
 * holds simulations; the combination is not supported).  SZ_ERR_STATE: a search is in progress (the rule of sz_set_leaf_batching). */
int sz_set_search_budgets(sz_engine* e, const int32_t* budgets, void* stream);
/* IN-SEARCH batch compaction, the other half: valid only between sz_search_begin and the end of that search (SZ_ERR_STATE before a
 * search and once no board searches any more; nothing is changed then).  The boards that still search (not done, no error) are renumbered
 * 0..n_live-1 in board order, the others get no row, and the pending network inputs of the live boards — leaves_per_step rows each — are
 * moved to their new rows of planes_dev (the buffer sz_search_begin / sz_search_step wrote; staged through an engine-owned buffer that
 * is allocated on first use, since a board's new row can be another live board's old row).  When the call returns the next evaluation runs
 * on rows 0..n_live*leaves_per_step-1 and the next sz_search_step reads policy / value from the new rows.  Works from the identity
 * mapping and after sz_compact (rows only ever move down); the next sz_compact between searches replaces the mapping as before — call it
 * (enable 1 or 0) before the next sz_search_begin, a board without a row is flagged SZ_ERR_STATE there.  Results per board do not depend
 * on the mapping.  Synchronises the stream to return n_live. */
int sz_compact_searching(sz_engine* e, void* planes_dev, int32_t* n_live_out, void* stream);

/* NON-REFERENCE option, off by default: a ROOT VISIT TARGET per board, the form of a search budget that works with reuse_subtree (lc0 / KataGo:
 * the budget names the root's visit count at the END of the search, visits a kept subtree already holds count towards it).
 * targets: HOST array [n_boards], each entry in 0..num_searches; NULL = off (every board makes num_searches new simulations again).  Accepted on
 * engines with and without reuse_subtree.  Only between searches (SZ_ERR_STATE during a search, the rule of sz_set_search_budgets; nothing is
 * changed then); SZ_ERR_INVALID: an entry outside 0..num_searches.  Takes effect at the next sz_search_begin and holds until changed.
 * With targets set, board b's search makes `goal` NEW simulations, computed by sz_search_begin where the root is known:
 *   fresh root       goal = t_b: a new game, an upload, any of the three fresh-start conditions of sz_config.reuse_subtree, dropped subtrees,
 *                    and every search of an engine without reuse_subtree.  This is exactly a budget of t_b: on an engine without reuse_subtree
 *                    the call equals sz_set_search_budgets(targets) bit for bit.
 *   continued search on a kept root with visit count N_kept: goal = max(0, t_b + 1 - N_kept).  The search ends with root visit count
 *                    max(N_kept, 1 + t_b): what a fresh search with budget t_b ends with, or what was kept if that was more.
 * With goal == 0 the board is done when sz_search_begin returns: it takes no network row after the next sz_compact_searching, and sz_play samples
 * from the kept visit counts.  num_searches stays the capacity; the fresh-start conditions are unchanged.  Everything that reads a budget reads
 * the goal: the gather end (simulations done + pending == goal), the done test, the solver counting a proven root out, the terminal-root shortcut
 * (N = 1 + t_b).  sz_stats.simulations counts new simulations only; the per-ply record (sz_fetch_ply visits) is the root's children as they stand,
 * kept visits included.  Targets and budgets exclude each other, the later setter wins (sz_set_search_budgets, NULL included, switches targets
 * off); on a reuse_subtree engine sz_set_search_budgets(non-NULL) stays refused.  Works with sz_set_search_options (any L, solver on or off),
 * sz_compact and sz_compact_searching.  With targets always on a kept subtree never exceeds num_searches nodes, so the doubled stores of
 * reuse_subtree could be halved; that is not done.  Held bit for bit to the host restatement tests/targetref.py by
 * tests/test_gpu_visit_targets.py.  Its effect on playing strength is unmeasured. */
int sz_set_visit_targets(sz_engine* e, const int32_t* targets, void* stream);
/* Valid after sz_search_begin: the NEW simulations each board's search makes (HOST array [n_boards]): the goal above with targets set, else the
 * board's budget, else num_searches; 0 for a board that does not search.  Synchronises the stream.  It is what the host plans its segments of
 * steps and shrinks from (search_segments). */
int sz_search_goals(sz_engine* e, int32_t* goals, void* stream);
/* NON-REFERENCE option, off by default: the root noise of sz_set_root_noise applied at the root of EVERY search, continued ones included, so
 * that it works with reuse_subtree.  gamma_dev: device array [n_boards][SZ_MAX_MOVES] f32 of Gamma(alpha,1) draws, read by sz_search_begin
 * (continued search) and by the step after it (fresh root); NULL = the reference behaviour.  Needs learning = 1.
 *   continued search the kept root's K children get P_c = (0.75f*P_c) + (0.25f*(g_c / gs)), in place, in sz_search_begin before its descent-only
 *                    launch.  The kept root was expanded as an inner node under this mode, inner nodes get no noise, so its children's priors
 *                    are the clean renormalised policy.
 *   fresh root       noised at expansion exactly as sz_set_root_noise does.
 *   arithmetic       one device function for both sites: gs from lane-strided partial sums (lane l adds g[l], g[l+64], ... ascending) and an
 *                    xor butterfly, every operator one IEEE rounding (-ffp-contract=off).
 *   quiet            HOST array [n_boards] or NULL (no board is quiet).  quiet[b] != 0: board b's root gets no noise in the searches that
 *                    follow, fresh or continued; its priors stay clean (KataGo: no noise on fast plies).
 * On a reuse_subtree engine a call that switches between gamma_dev == NULL and non-NULL drops every kept subtree (a tree built under the
 * reference's noise carries the constant in every node's priors, one built under root-only noise carries it nowhere); a call that only changes
 * the pointer or `quiet` keeps them.  While this mode is on, a reuse_subtree engine refuses sz_set_root_noise (SZ_ERR_STATE): leave the mode
 * through this setter.  Only between searches (SZ_ERR_STATE during a search; nothing is changed then).  On an engine without reuse_subtree and
 * with quiet == NULL the call equals sz_set_root_noise.  Orthogonal to sz_set_search_options, sz_set_visit_targets, sz_compact and
 * sz_compact_searching.  Held bit for bit to tests/targetref.py by tests/test_gpu_visit_targets.py.  Its effect on playing strength is unmeasured. */
int sz_set_search_root_noise(sz_engine* e, const float* gamma_dev, const uint8_t* quiet, void* stream);

/* NON-REFERENCE option, off by default: proven-result propagation (MCTS-Solver; lc0's "certainty propagation").  The reference backs a
 * checkmate leaf up as one more sample of -1; with enable != 0 the search also carries what is PROVEN up the tree.  Off, every kernel that
 * runs today runs unchanged (the solver is a template instantiation of its own, like leaf batching).
 * State: every node e has R(e) in {unknown, WIN, DRAW, LOSS}, from the view of the side to move in e's position (the convention of the
 * terminal value), and one bit complete(e), set at expansion when the number of children created equals the number of legal moves
 * (expansion drops moves whose renormalised prior is exactly 0; a node that lost a move that way is never proven LOSS or DRAW).  Both live
 * in 16 spare bits of the edge record: no new memory per edge.  Rules, per board:
 *   terminal leaf  when a leaf's position is created and found terminal: R = LOSS if the side to move is mated, DRAW otherwise.
 *   update         after every backup, walk the backed-up path from its last node towards the root.  The parent p of a node whose R has
 *                  just become proven is recomputed from p's children alone (one wavefront, lanes = children): WIN if any child is LOSS;
 *                  otherwise, if complete(p) and every child is proven, DRAW if any child is DRAW, else LOSS; otherwise unknown.  The walk
 *                  stops at the first node whose R does not change.  R never goes back to unknown.
 *   descent        a descent stops at the first node on its way whose R is proven, the root included.  The simulation ends there: it is
 *                  backed up along the path to that node with -1 / 0 / +1 for LOSS / DRAW / WIN (the usual sign alternation), and counted
 *                  as a simulation and as a terminal_hit at that node's depth (sz_stats); selection repeats within the same step, as it
 *                  does for terminal leaves.  With a proven root all remaining simulations of the board end at the root in one step.
 *   selection      at an unknown node the arg-max runs over the children with R != WIN (a child whose side to move wins is a refuted
 *                  move); Node.get_ucb, its operation order and the first-maximum tie-break are unchanged.  If every child is WIN (possible
 *                  only when complete is 0) it runs over all children.
 *   sz_play        on a board whose root is WIN the move played and recorded as `chosen` is the first root child in action order with
 *                  R == LOSS, whatever the uniform; the recorded action / visits stay what the search counted.  A root that is LOSS,
 *                  DRAW or unknown is played as without the solver.
 * NO mate distance is kept: a won position is won by the first proving move in action order, which may not be the shortest mate.
 * Only between searches (SZ_ERR_STATE otherwise, the rule of sz_set_leaf_batching).  SZ_ERR_INVALID when enabling on an engine created
 * with reuse_subtree or while leaves_per_step > 1; sz_set_leaf_batching with leaves_per_step > 1 is refused (SZ_ERR_INVALID) while the
 * solver is on.  Both combinations are follow-ups, not supported by this entry point: sz_set_search_options below sets them.  Works with sz_set_search_budgets (a board whose root is proven early
 * keeps searching until its budget is counted out), sz_compact, sz_compact_searching and sz_set_root_noise.  Held bit for bit to the host
 * restatement tests/solverref.py by tests/test_gpu_solver.py.  Its effect on playing strength is unmeasured. */
int sz_set_solver(sz_engine* e, int32_t enable, void* stream);
/* NON-REFERENCE option: leaf batching, the solver and subtree reuse in ONE search.  Sets leaves_per_step / virtual_loss (sz_set_leaf_batching)
 * and the solver (sz_set_solver) in one call and accepts every combination of L >= 1 and solver on or off, on engines with and without
 * reuse_subtree.  Only between searches (SZ_ERR_STATE otherwise; nothing is changed then).  SZ_ERR_INVALID: opt NULL, L < 1,
 * L > SZ_MAX_LEAVES_PER_STEP, virtual_loss negative or not finite.  {1, x, 0} leaves the engine exactly as if no setter had been called;
 * {L, lam, 0} on an engine without reuse_subtree equals sz_set_leaf_batching(L, lam), {1, x, 1} there equals sz_set_solver(1).  After it
 * sz_set_leaf_batching and sz_set_solver still apply their own refusals against the state now in force.  Still refused, and not part of
 * this option: sz_set_search_budgets with budgets != NULL on a reuse_subtree engine, sz_set_root_noise on a reuse_subtree engine (their
 * counterparts for a reuse_subtree engine are sz_set_visit_targets and sz_set_search_root_noise).
 * Never called, every kernel that runs today runs unchanged (the combination is a template instantiation of its own).
 *
 * Setting changes on a reuse_subtree engine: a call that changes leaves_per_step or the solver flag drops every board's kept subtree; the next
 * search of every board starts from a fresh root (a tree built without the solver has no `complete` bits, one built before the in-flight
 * counts existed has none).  A call that changes neither (virtual_loss alone included) keeps the subtrees.
 *
 * Solver with L > 1.  Everything sz_set_leaf_batching and sz_set_solver say holds, with these rules where they meet:
 *   selection      the arg-max runs over the children with R != WIN, over all children if every child is WIN; each child is scored with
 *                  visit count N + k and value sum W + lambda*k (f64) under sqrt(N_parent + k_parent).  Node.get_ucb's arithmetic and the
 *                  first-maximum tie-break are unchanged.  With every k == 0 it is the solver's selection exactly.
 *   proven stop    a descent stops at the first proven node on its way, the root included.  It is backed up on the spot with -1 / 0 / +1,
 *                  counted as a simulation and a terminal_hit at that depth (and in sz_solver_stats out[0] when the node is not terminal),
 *                  never becomes pending and adds nothing to any k; the gather goes on, as it does after a terminal leaf.
 *   terminal leaf  a new terminal leaf is labelled at creation and backed up, then the update walks its path: the only place it runs.
 *   pending leaf   is non-terminal, hence unknown: a parent with a pending child cannot become LOSS or DRAW.  Leaves already pending in
 *                  this step whose ancestors become proven during the gather are still expanded and backed up in the next step, in gather
 *                  order.  R never goes back.  `complete` is set at expansion as without leaf batching.
 *   proven root    if the root becomes proven in the middle of a gather, the remaining descents of the budget (budget - simulations done -
 *                  leaves pending) end at the root in that same step; the board is done once its pending leaves have been consumed.
 *   collision      a descent that ends on a visited non-terminal node without children (a leaf pending in this step) ends the gather.
 * Budgets (sz_set_search_budgets), sz_compact and sz_compact_searching work as with leaf batching alone (leaves_per_step rows per board).
 *
 * reuse_subtree with L > 1.  At the end of a search every in-flight count is 0 (every descent was taken back), and sz_play's compaction
 * only moves edges to lower indices among the edges in use, so a kept subtree has no descent in flight.  A continued search has no root
 * evaluation in flight either: sz_search_begin's descent-only launch gathers up to L leaves (rows slot(b)*L + i) before the first network
 * call.  The three fresh-start conditions of sz_config.reuse_subtree are unchanged, a continued search makes num_searches new simulations,
 * and its length in steps is data-dependent: step until sz_pending_boards is 0.
 *
 * reuse_subtree with the solver.  Labels and `complete` bits travel with their edges through the compaction.  They are relative to the side
 * to move in the node, and the game history below the new root is the history they were computed under, so they stay true.  A chosen child
 * that is proven but has children is kept like any other (fresh-start condition (1) is unchanged).  A continued search whose root is
 * proven counts all num_searches simulations out at the root in the descent-only launch: it never asks for the network and its board is
 * done when sz_search_begin returns.  sz_play on a WIN root plays the first LOSS child; a fresh start labels nothing but a terminal root.
 * All three options together follow from the above.
 * Held bit for bit to the host restatement tests/composeref.py by tests/test_gpu_compose.py.  The effect of any combination on playing
 * strength is unmeasured. */
typedef struct sz_search_options {
    int32_t leaves_per_step;     /* L of sz_set_leaf_batching, 1..SZ_MAX_LEAVES_PER_STEP */
    float   virtual_loss;        /* lambda of sz_set_leaf_batching (ignored at L = 1) */
    int32_t solver;              /* != 0: proven-result propagation on (sz_set_solver) */
} sz_search_options;
int sz_set_search_options(sz_engine* e, const sz_search_options* opt, void* stream);
/* proven results after (or during) a search, device pointers: root_dev [n_boards] int8, child_dev [n_boards,218] int8 in action order, as
 * sz_root_children.  Codes: 0 unknown, 1 WIN, 2 DRAW, 3 LOSS, each for the side to move in that node's own position (a root child
 * with 3 is a move that wins for the root).  All 0 without the solver. */
int sz_root_proven(sz_engine* e, int8_t* root_dev, int8_t* child_dev, void* stream);
/* test / inspection: proven code and complete bit of every node of one board's tree, rows in sz_debug_tree's order (host arrays of
 * max_nodes entries, may be NULL to count) */
int sz_debug_tree_proven(sz_engine* e, int32_t board, int32_t max_nodes, int8_t* proven, uint8_t* complete, int32_t* n_out, void* stream);
/* solver counters, all boards, cumulative since the solver was first switched on (synchronises): out[0] simulations that ended on a proven
 * NON-terminal node, out[1] nodes proven by the update rule (terminal leaves not counted).  sz_stats is unchanged. */
int sz_solver_stats(sz_engine* e, uint64_t out[2], void* stream);

/* NON-REFERENCE option, off by default: FORCED PLAYOUTS and POLICY-TARGET PRUNING (KataGo).  Root noise only helps if a noised move that is
 * good gets enough visits to show it, and the visits noise buys for bad moves must not end up in the policy target.  With the option on, the
 * root of a board's search orders a minimum of visits for every child it has tried, and sz_play takes them out of the record again where the
 * search did not confirm them.  Never switched on, every kernel that runs today runs unchanged (the option is a template instantiation of its
 * own, k_search_begin / k_search_step / k_play<.., ForcedOpts>, as leaf batching and the solver are).
 * k == 0 switches the option off (boards is ignored); k > 0 and finite switches it on for the boards with boards[b] != 0 (HOST array
 * [n_boards]; NULL = all boards).  SZ_ERR_INVALID: k negative or not finite, or k > 0 on an engine created with learning = 0 (an exploration
 * option of self-play, like root noise).  Only between searches (SZ_ERR_STATE during a search, the rule of sz_set_search_budgets; nothing is
 * changed then).  Takes effect at the next sz_search_begin, which latches the board's bit into its status word (ST_FORCED beside ST_QUIET;
 * sz_play clears it), and holds until changed: a call between the end of a search and its sz_play does not change that sz_play.
 * The tree is never modified by the option, so changing k or boards does not drop kept subtrees.  Orthogonal to sz_set_search_options (any L,
 * solver on or off), sz_set_visit_targets, sz_set_search_budgets, sz_set_search_root_noise, sz_compact and sz_compact_searching, on engines
 * with and without reuse_subtree.  Every operator below is one IEEE rounding (-ffp-contract=off).
 *   forced selection  in sz_search_step and in sz_search_begin's descent-only launch, at depth 0 only, on boards with the bit set.  The root's
 *                  children are c = 0..K-1 with counts n_c = N_c + k_c (k_c the in-flight count, 0 without leaf batching), n_p = N_root +
 *                  k_root (what selection takes as the parent's count) and T = n_p - 1.  Child c is FORCED when n_c >= 1 and
 *                  (double)n_c < sqrt(((double)k * (double)P_c) * (double)T), P_c the prior as stored (after any root noise).  With the solver
 *                  a child proven WIN is not forced whenever the arg-max skips WIN children.  If at least one child is forced the selected
 *                  child is the forced child with the lowest index (counted in sz_forced_stats out[0]); otherwise selection is Node.select
 *                  exactly as without the option.  Below the root nothing changes.  A NaN or negative product forces nothing.
 *   pruning        in sz_play, on boards with the bit set, after the zero-visit check (which stays on the counted visits).  T = N_root - 1,
 *                  sq = (float)sqrt((double)N_root), c* = the first maximum of N_c in action order, best = get_ucb(N*, W*, P*, sq, c_puct).
 *                  For every other child with N_c >= 1: m_c = min(N_c, (int)floor(sqrt(((double)k*(double)P_c)*(double)T))) (0 when the root
 *                  is NaN); q_c = the q term of get_ucb at the counted N_c, W_c, held fixed; n' = N_c; at most m_c times: cand = n' - 1,
 *                  u = (((1.0f/(float)(cand+1)) * sq) * c_puct) * P_c, if q_c + u < best then n' = cand, else stop.  Afterwards, if n' < N_c
 *                  and n' <= 1, n' = 0.  Children with N_c = 0 and c* keep their counts.  sz_forced_stats out[1] grows by the sum of N_c - n'.
 *   the pruned counts  are what the record holds (sz_fetch_ply visits), and what sz_play samples or arg-maxes from, with the same sequential
 *                  f64 arithmetic and total' = the sum of n'.  Forced visits are exploration the search ordered, not evidence.  The
 *                  solver's WIN-root rule stays on top.  sz_root_children, sz_debug_tree and the subtree kept by reuse_subtree show the
 *                  counted visits, unchanged.
 * Held bit for bit to the host restatement tests/forcedref.py by tests/test_gpu_forced_playouts.py.  Its effect on playing strength is unmeasured. */
int sz_set_forced_playouts(sz_engine* e, float k, const uint8_t* boards, void* stream);
/* forced-playout counters, all boards, cumulative since the option was first switched on (synchronises): out[0] root selections decided by a
 * forced child, out[1] visits that pruning took out of the records.  sz_stats is unchanged. */
int sz_forced_stats(sz_engine* e, uint64_t out[2], void* stream);
/* test: the DEVICE code of forced selection and of pruning (the functions the option's k_search_step and k_play call) on caller-supplied
 * children, one wavefront per case, in the manner of sz_debug_select.  Case c owns children offsets[c]..offsets[c+1] (<= SZ_MAX_MOVES each) of
 * vc (N), inflight (k), value_sum (f64), prior (f32) and proven (codes of sz_root_proven; NULL = the instantiations without the solver);
 * parent_visits[c] (n_p), c_puct[c], forced_k[c]; virtual_loss is one number for all cases.  Writes per case the selected child and whether a
 * forced child decided it, and, for the case read as a finished search with N_root = parent_visits[c] (in-flight counts ignored), every child's
 * pruned count and c*.  All device pointers. */
int sz_debug_forced(const int32_t* offsets_dev, const int32_t* vc_dev, const int32_t* inflight_dev, const double* value_sum_dev, const float* prior_dev,
                    const int8_t* proven_dev, const int32_t* parent_visits_dev, const float* c_dev, const float* forced_k_dev, float virtual_loss,
                    int32_t* selected_out_dev, int32_t* forced_out_dev, int32_t* pruned_out_dev, int32_t* cstar_out_dev, int32_t n_cases, void* stream);

/* NON-REFERENCE option, off by default: FIRST-PLAY URGENCY for unvisited children (lc0, KataGo).  Node.get_ucb scores a child that was never
 * tried as 1 - ((0 / 1e-6) + 1) / 2 = 0.5, a dead draw, at every node: where the mover is losing every untried move then looks better than
 * everything tried and the search goes wide, where the mover is winning untried moves are handicapped for no reason.  With the option on an
 * unvisited child is scored from a first-play value v0 that is a constant or follows the parent's value, with one setting for the board's
 * root and one for every node below it (lc0's self-play uses a different one at the root, so that root noise gets looked at).  Never switched
 * on, every kernel that runs today runs unchanged: the option is an instantiation of k_search_step of its own, with one more trailing argument
 * beside ForcedOpts (k_search_step<VL, SOLVE, [ForcedOpts,] FpuOpts>).  k_search_begin selects nothing and k_play reads visited children only:
 * neither has an FPU variant.
 * The rule, wherever a child is selected (sz_search_step and the descent-only launch of sz_search_begin) for a parent p with children
 * c = 0..K-1.  All arithmetic is f32, every operator one IEEE rounding (-ffp-contract=off):
 *   counts     n_c = N_c + k_c (k_c the in-flight count, 0 without leaf batching); a child is VISITED when n_c >= 1.  n_p = N_p + k_p and
 *              sq = (float)sqrt((double)n_p), as without the option.
 *   visited    a visited child is scored exactly as without the option: get_ucb on n_c and W_c + lam*k_c.
 *   mode       the mode and value in force are the root's at depth 0 of a descent (the board's root, of a fresh and of a continued search
 *              alike) and the tree's elsewhere.  With SZ_FPU_REFERENCE an unvisited child is scored exactly as without the option.
 *   unvisited  otherwise an unvisited child scores q0 + u, u = (((1.0f / (float)(0 + 1)) * sq) * c_puct) * P_c (get_ucb's second term at a
 *              count of 0) and q0 = (v0 + 1.0f) / 2.0f, with
 *                ABSOLUTE   v0 = value
 *                REDUCTION  v0 = vp - (value * (float)sqrt((double)mass)), where vp = (float)W_p / ((float)N_p + 1e-6f) is taken from the
 *                           parent's own stored edge (the root is edge 0; no in-flight terms; a fresh root's N_p carries the reference's
 *                           extra 1 of mcts.py:46, which is not corrected) and mass is the sum of P_c over the visited children in a fixed
 *                           order: lane l adds children l, l+64, ... ascending, skipping unvisited ones, then an xor butterfly (offsets 32
 *                           down to 1).  A child's proven label does not matter for mass.
 *              then the clamp: if (!(v0 >= -1.0f)) v0 = -1.0f; if (v0 > 1.0f) v0 = 1.0f.  vp and mass are computed once per parent.
 *   arg-max    the arg-max, its first-maximum tie-break and the solver's skipping of WIN children (all children when every child is WIN) are
 *              unchanged.  On a forced board (sz_set_forced_playouts) the forced child decides first, as without the option; it only ever
 *              looks at children with n_c >= 1.  Policy-target pruning and the ending rules read visited children only and are untouched.
 * ABSOLUTE with value 0 gives q0 = 0.5f, exactly what get_ucb yields for an unvisited child: an engine set to ABSOLUTE 0 at both sites builds
 * the same trees as one with the option off, bit for bit, through different kernels.
 * Works with learning 0 and 1.  Only selection changes and the tree is never modified, so changing the option does not drop kept subtrees.
 * Orthogonal to sz_set_search_options (any L, solver on or off), budgets, visit targets, root noise, forced playouts, endings, sz_compact,
 * sz_compact_searching and sz_play_moves, on engines with and without reuse_subtree.
 * Held bit for bit to the host restatement tests/fpuref.py by tests/test_gpu_fpu.py.  Its effect on playing strength is unmeasured. */
enum { SZ_FPU_REFERENCE = 0, SZ_FPU_ABSOLUTE = 1, SZ_FPU_REDUCTION = 2 };
typedef struct sz_fpu_options {
    int32_t tree_mode;  float tree_value;     /* every node below the root */
    int32_t root_mode;  float root_value;     /* the board's root (depth 0 of a descent), fresh or continued search */
} sz_fpu_options;                             /* 16 bytes */
/* opt == NULL, or both modes SZ_FPU_REFERENCE, switches the option off: the kernels that run without it then run.  SZ_ERR_INVALID: a mode
 * outside 0..2, an ABSOLUTE value that is not finite or outside [-1, 1], a REDUCTION value that is not finite, negative or above 2 (the
 * value of a REFERENCE site is ignored).  SZ_ERR_STATE during a search (the rule of sz_set_search_budgets; nothing is changed then).  Takes
 * effect at the next sz_search_begin and holds until changed. */
int sz_set_fpu(sz_engine* e, const sz_fpu_options* opt, void* stream);
/* test: the DEVICE code of selection under the option (the function the option's k_search_step calls) on caller-supplied children, one
 * wavefront per case, in the manner of sz_debug_select and sz_debug_forced.  Case c owns children offsets[c]..offsets[c+1] (1..SZ_MAX_MOVES
 * each) of vc (N), inflight (k), value_sum (f64), prior (f32) and proven (codes of sz_root_proven; NULL = the instantiations without the
 * solver); parent_visits[c] (n_p), the parent's stored parent_n[c] (N_p) and parent_w[c] (W_p, f64), c_puct[c], is_root[c] (!= 0: the
 * root's mode and value apply) and opts[c]; virtual_loss is one number for all cases.  Writes every child's score (a WIN child the arg-max
 * skips included) and per case the selected child.  opts are not checked.  All device pointers. */
int sz_debug_select_fpu(const int32_t* offsets_dev, const int32_t* vc_dev, const int32_t* inflight_dev, const double* value_sum_dev, const float* prior_dev,
                        const int8_t* proven_dev, const int32_t* parent_visits_dev, const int32_t* parent_n_dev, const double* parent_w_dev, const float* c_dev,
                        const int32_t* is_root_dev, const sz_fpu_options* opts_dev, float virtual_loss, float* ucb_out_dev, int32_t* selected_out_dev,
                        int32_t n_cases, void* stream);

/* NON-REFERENCE option, off by default: GUMBEL ROOT SEARCH (Danihelka et al., "Policy improvement by planning with Gumbel", ICLR 2022).  PUCT
 * visit counts with root noise give no policy improvement at small simulation counts.  With the option on the root samples m moves without
 * replacement by Gumbel-top-k, spends the search's simulations on them by sequential halving, sz_play plays the best of the most visited
 * moves, and the training target is the completed-Q improved policy instead of the visit fractions.  A root-only rule, stateless per
 * simulation, one wavefront per board.  Never switched on, every kernel that runs today runs unchanged: the option is an instantiation of its
 * own, k_search_step<false, false, GumbelOpts[, FpuOpts]> (only depth 0 of a descent changes) and k_play<false, GumbelOpts>; k_search_begin
 * has no variant, the root's network value is kept where the root is expanded.
 * The rule.  All arithmetic is f64, every operator one IEEE rounding (-ffp-contract=off), sums run sequentially in ascending child order:
 *   slog, sexp   libm's and the device's log / exp do not round alike, so the rule carries its own, written from + - * / and integer bit
 *                operations only (csrc/sz_gumbel.h; tests/gumbelref.py repeats them operator for operator).
 *                slog(x), x > 0 (a prior that is exactly 0 is dropped at expansion): x = 2^e * mant by bit operations with mant in
 *                [sqrt(1/2), sqrt(2)) (mant >= 1.4142135623730951 is halved, e + 1), s = (mant - 1) / (mant + 1), s2 = s * s,
 *                p = 1/19; p = p * s2 + 1/k for k = 17, 15, ..., 3, 1; slog = (2 * s) * p + (double)e * LN2, LN2 = 0.6931471805599453.  Ten terms:
 *                the first one left out is s^20 / 21 < 2.3e-17 < 2^-53 over |s| <= 0.1716.
 *                sexp(y), y <= 0: 0 when !(y >= -700) (the cutoff; every other result is a normal number); k = floor(y * 1.4426950408889634 +
 *                0.5); r = (y - k * LN2_HI) - k * LN2_LO with LN2_HI = 0x3FE62E42FEE00000, LN2_LO = 0x3DEA39EF35793C76; p = 1/13!;
 *                p = p * r + 1/j! for j = 12, 11, ..., 1, 0; the result is p with k added to its exponent bits.  Fourteen terms: the first one
 *                left out is r^14 / 14! < 4.2e-18 < 2^-53 over |r| <= 0.3466.  Every constant 1/k, 1/j! is the correctly rounded quotient.
 *   root         the root's children c = 0..K-1 with N_c, W_c, P_c as stored (on a learning engine the reference's constant noise mix stays
 *                in P_c).  logit_c = slog((double)P_c).  q_c = 0.5 - 0.5 * (W_c / (double)N_c) for N_c >= 1, the mover's value of move c in
 *                [0, 1] (a child's W is stored from the child's side to move).  vhat = the root's network value as sz_search_step reads it
 *                when it expands the root (one float per board), v01 = 0.5 + 0.5 * (double)vhat.  maxN = max_c N_c.
 *                sigma(x) = (((double)c_visit + (double)maxN) * (double)c_scale) * x.
 *   schedule     goal = the new simulations of this search (sz_search_goals); n = goal - 1 root-child visits, the first simulation expands
 *                the root.  m_eff = min(max_considered, K), L = max(1, ceil(log2 m_eff)).  Phases: the first has c = m_eff considered
 *                children; a phase with c has r = max(1, floor(n / (L * c))) rounds of c visits each; then c <- max(2, floor(c / 2)); the
 *                last phase is cut where n visits are scheduled; with m_eff = 1 every visit goes to that child.  The level l_t of root-child
 *                visit t (0-based) = the rounds completed before the round t falls in, summed over the phases.  The device walks the phases.
 *   selection    at root-child visit t: among the children with N_c == l_t the arg-max of s_c = (g_c + logit_c) + sigma(q_c), the sigma term
 *                0.0 at N_c = 0, first maximum (wave_select_child's loop and tie-break).  The considered set is implicit: a child that is
 *                not picked stays below the level and never matches again; level 0 picks the top m_eff by g + logit.  No child at the
 *                level: the arg-max runs over all children; the schedule makes that impossible for a fresh root, sz_gumbel_stats counts it.
 *                Terminal children are visited and counted like any other.  Below the root nothing changes.
 *   sz_play      after the early return and the zero-visit check, both as without the option: the move is the arg-max of s_c over the
 *                children with N_c == maxN, first maximum; the board's uniform is not read; the record's action and visits stay the counted
 *                visits.
 *   policy       sumN = sum of N_c.  v_mix = v01 when sumN is 0, else (v01 + (double)sumN * (sum over N_c >= 1 of (double)P_c * q_c /
 *                sum over N_c >= 1 of (double)P_c)) / (1.0 + (double)sumN).  cq_c = q_c if N_c >= 1 else v_mix; z_c = logit_c + sigma(cq_c);
 *                zmax = the maximum of z_c; e_c = sexp(z_c - zmax); policy_target[b][c] = (float)(e_c / sum of e) for c < K and 0 beyond.
 * Below the root the paper's deterministic completed-Q selection is an option of its own on top of this one, sz_set_gumbel_tree below.
 * Not done, each a follow-up: recording fast plies as training samples; and every combination refused below.
 * Works with learning 0 and 1, budgets and visit targets on an engine without reuse_subtree (the rule reads the board's goal), sz_compact,
 * sz_compact_searching, sz_play_moves and sz_set_fpu (below the root FPU acts as without the option, unless sz_set_gumbel_tree decides there; its root_mode
 * is not consulted, Gumbel decides there).  Held bit for bit to the host restatement tests/gumbelref.py by tests/test_gpu_gumbel.py.  Strength effect unmeasured. */
typedef struct sz_gumbel_options { int32_t max_considered; float c_visit; float c_scale; } sz_gumbel_options;   /* 12 bytes */
/* opt == NULL switches the option off.  g_dev: device array [n_boards][SZ_MAX_MOVES] of f64 Gumbel(0,1) draws, indexed by root child in action
 * order as gamma_dev is; NULL = all zeros, a deterministic search for match play.  It is read at every root selection and by sz_play: the
 * caller keeps it unchanged from sz_search_begin to sz_play.  SZ_ERR_INVALID: max_considered outside 1..SZ_MAX_MOVES; c_visit or c_scale not
 * finite or negative; a reuse_subtree engine, leaves_per_step > 1, the solver on, forced playouts on, endings on (and sz_set_leaf_batching,
 * sz_set_solver, sz_set_search_options, sz_set_forced_playouts, sz_set_endings refuse to switch those on while Gumbel is on).  SZ_ERR_STATE:
 * a call during a search (the rule of sz_set_search_budgets; nothing is changed then); root noise on (sz_set_root_noise or
 * sz_set_search_root_noise with a gamma), and those two refuse a gamma with SZ_ERR_STATE while Gumbel is on: Gumbel is the root's
 * exploration.  Takes effect at the next sz_search_begin and holds, for that search and its sz_play, until changed. */
int sz_set_gumbel(sz_engine* e, const sz_gumbel_options* opt, const double* g_dev, void* stream);
/* after sz_play: the improved policy policy_target [n_boards][SZ_MAX_MOVES] f32 by root child as sz_fetch_ply's action, v_mix [n_boards] f64
 * and the root's network value root_value [n_boards] f32.  HOST pointers, any may be NULL; rows are valid where sz_fetch_ply's active is 1.
 * SZ_ERR_STATE on an engine the option was never switched on for.  Synchronises the stream. */
int sz_fetch_gumbel(sz_engine* e, float* policy_target, double* v_mix, float* root_value, void* stream);
/* cumulative over all boards: out[0] root selections made by the rule, out[1] those of them that found no child at the level (0 on fresh roots) */
int sz_gumbel_stats(sz_engine* e, uint64_t out[2], void* stream);
/* test: the DEVICE code of the option on caller-supplied cases, one wavefront per case, in the manner of sz_debug_forced.  Three parts, each
 * skipped when its first array is NULL.  Maths: slog_out[c] = slog(x[c]), sexp_out[c] = sexp(x[c]).  Level: tnm[c] = (t, n, m_eff),
 * level_out[c] = l_t, -1 unless 0 <= t < n and m_eff >= 1.  Children: case c owns children offsets[c]..offsets[c+1] (1..SZ_MAX_MOVES each) of
 * vc (N), value_sum (f64), prior (f32) and g (f64, NULL = zeros); visit[c] (t), goal[c], root_value[c] (vhat) and opts[c] (not checked beyond
 * max_considered >= 1 and 0 <= t < goal - 1, else -1s).  Writes the root selection at visit t and whether it fell back to all children, and of
 * the case read as a finished search sz_play's move, every child's policy_target and v_mix.  All device pointers. */
int sz_debug_gumbel(const double* x_dev, double* slog_out_dev, double* sexp_out_dev, const int32_t* tnm_dev, int32_t* level_out_dev,
                    const int32_t* offsets_dev, const int32_t* vc_dev, const double* value_sum_dev, const float* prior_dev, const double* g_dev,
                    const int32_t* visit_dev, const int32_t* goal_dev, const float* root_value_dev, const sz_gumbel_options* opts_dev,
                    int32_t* selected_out_dev, int32_t* fallback_out_dev, int32_t* final_out_dev, float* policy_out_dev, double* v_mix_out_dev,
                    int32_t n_cases, void* stream);

/* NON-REFERENCE option, off by default, on top of sz_set_gumbel: COMPLETED-Q SELECTION BELOW THE ROOT (Danihelka et al., section 5, "Full
 * Gumbel").  With sz_set_gumbel alone every inner node spends its visits by PUCT, a rule tuned for hundreds of visits whose counts at 16 to 64
 * simulations are mostly its c_puct * P * sqrt(N) term.  With this flag an inner node picks the child whose share of the visits lags furthest
 * behind the completed-Q improved policy of that node: deterministic, stateless per simulation, one wavefront per board.  Never switched on,
 * every kernel that runs today runs unchanged: the flag is one more instantiation, k_search_step<false, false, GumbelTreeOpts>, which also
 * keeps every expanded node's network value, [n_boards][num_searches + 2] f32 by node id; k_play and k_search_begin have no variant.
 * The rule applies wherever a child is selected at depth d >= 1 of a descent, in a search begun with Gumbel on and the flag on.  The parent is
 * node p with children c = 0..K-1, N_c, W_c, P_c as stored; vhat_p is the f32 network value sz_search_step read from value_dev when it
 * expanded p.  All arithmetic is f64, every operator one IEEE rounding (-ffp-contract=off); slog, sexp, q_c and the sigma factor are
 * sz_set_gumbel's:
 *   wsum(t)      lane l (0..63) starts from 0.0 and adds t_c for c = l, l+64, l+128, l+192 (< K), ascending; then for off = 32, 16, 8, 4, 2, 1:
 *                v_l = v_l + v_(l xor off).  Every lane ends with the same bits because f64 addition commutes (the argument of sz_set_fpu's
 *                prior mass); the result is read back through readfirstlane.  NOT the sequential sum of sz_play's improved policy, which runs
 *                once per ply: this one runs at every depth of every descent.
 *   q_c          = 0.5 - 0.5 * (W_c / (double)N_c) for N_c >= 1.
 *   maxN         = max_c N_c;  sf = ((double)c_visit + (double)maxN) * (double)c_scale;  sumN = the integer sum of N_c, exact.
 *   v01          = 0.5 + 0.5 * (double)vhat_p.
 *   pq           = wsum(N_c >= 1 ? (double)P_c * q_c : 0.0);  pm = wsum(N_c >= 1 ? (double)P_c : 0.0).
 *   v_mix        = v01 when sumN == 0, else (v01 + (double)sumN * (pq / pm)) / (1.0 + (double)sumN).
 *   z_c          = slog((double)P_c) + sf * (N_c >= 1 ? q_c : v_mix);  zmax = max_c z_c;  e_c = sexp(z_c - zmax);  se = wsum(e_c), at least 1.
 *   score_c      = (e_c / se) - ((double)N_c / (1.0 + (double)sumN)).
 *   selection    the arg-max of score_c, the first maximum in child order (the loop and butterfly tie-break of the root's selection).
 * Terminal children are scored like any other.  The precondition on P_c is slog's own: positive.  Under the rule neither c_puct nor
 * sz_set_fpu's tree setting is consulted (its root setting already is not): FPU is accepted beside the rule and ignored.  Depth 0
 * (sz_set_gumbel's root selection), sz_play and the policy target are unchanged.
 * Latched by sz_search_begin like sz_set_gumbel.  SZ_ERR_INVALID: e is NULL.  SZ_ERR_STATE: a call during a search (nothing is changed
 * then); enabling while Gumbel is not on for the next search.  enable == 0 is always accepted between searches.  sz_set_gumbel(NULL) clears
 * the flag; sz_set_gumbel(opt != NULL) leaves it as it is.  The node values and the counter are allocated by the first enabling call.
 * Everything sz_set_gumbel refuses stays refused.  Held bit for bit to the host restatement tests/gumbeltreeref.py by
 * tests/test_gpu_gumbel_tree.py.  Strength effect unmeasured. */
int sz_set_gumbel_tree(sz_engine* e, int32_t enable, void* stream);
/* cumulative over all boards: out[0] selections below the root made by the rule.  sz_gumbel_stats is unchanged. */
int sz_gumbel_tree_stats(sz_engine* e, uint64_t out[1], void* stream);
/* test: the DEVICE function of the rule on caller-supplied cases, one wavefront per case, in the manner of sz_debug_gumbel.  Case c owns children
 * offsets[c]..offsets[c+1] (1..SZ_MAX_MOVES each, else selected_out -1) of vc (N), value_sum (f64) and prior (f32); node_value[c] is vhat_p and
 * opts[c] the constants (max_considered is not read).  Writes every child's score, the selected child and v_mix.  All device pointers. */
int sz_debug_gumbel_tree(const int32_t* offsets_dev, const int32_t* vc_dev, const double* value_sum_dev, const float* prior_dev, const float* node_value_dev,
                         const sz_gumbel_options* opts_dev, double* score_out_dev, int32_t* selected_out_dev, double* v_mix_out_dev, int32_t n_cases, void* stream);
/* test: the stored network value of every node of one board's tree, rows in sz_debug_tree's order; a node that was never expanded (unvisited,
 * terminal, or waiting for the network) has NaN.  HOST pointers; max_nodes 0 / node_value NULL only counts.  SZ_ERR_STATE unless the search
 * begun last runs under sz_set_gumbel_tree. */
int sz_debug_tree_values(sz_engine* e, int32_t board, int32_t max_nodes, float* node_value, int32_t* n_out, void* stream);

/* NON-REFERENCE option, off by default: RESIGNATION and ADJUDICATED GAME ENDINGS (AlphaZero, lc0, KataGo).  A self-play cycle lasts as long
 * as its longest game, and a game the rules have not ended yet is cut by the host without a result.  With the option on, sz_play ends a
 * board's game INSTEAD of playing a move when the finished search says the game is decided: the mover's most visited move has looked lost for
 * resign_patience of the mover's searches in a row, both sides have looked level for draw_patience searches in a row, or (proven, with the
 * solver on) the root is proven.  Boards flagged in `holdout` play on and only remember the first ply a rule would have ended them at, so the
 * thresholds can be checked against games that were played out.  Never switched on, every kernel that runs today runs unchanged: the option
 * is an instantiation of k_play of its own (k_play<SOLVE, [ForcedOpts,] EndOpts>); k_search_begin and k_search_step have none.
 * The rule, per board that passes sz_play's early return (searching, done, no error, game not over) and its zero-visit check, both first and
 * both on the counted visits.  All arithmetic is f64, every operator one IEEE rounding (-ffp-contract=off):
 *   inputs   colour = the side to move at the root (1 white, 0 black, sz_fetch_ply's colour); c* = the first maximum of the counted N_c over
 *            the root's children in action order (the tree's visits, before any policy-target pruning); m = -(W_c* / (double)N_c*), the
 *            mover's expected outcome of its most visited move (a child's W is stored from the child's side to move).
 *   state    per board: rs[2] (resign streak per colour), ds (draw streak, shared), would_ply (-1 = none), would_kind, would_colour.  Streaks
 *            saturate at 65535.  The array is allocated by the first call with opt != NULL; it is reset for exactly the boards sz_new_games
 *            starts and for the board sz_upload_game fills, never by sz_set_active or by this setter.  While the option is off nothing updates it.
 *   1 proven    if opt.proven != 0, the solver is on and the root's proven code R is not UNKNOWN, the game ends with kind SZ_END_PROVEN: WIN =
 *            the mover wins, LOSS = the mover loses, DRAW = a draw.  Holdout boards too (a proof is not a guess).  Streaks are not touched.
 *   2 streaks   if m <= (double)resign_value then rs[colour]++ else rs[colour] = 0; if fabs(m) <= (double)draw_value then ds++ else ds = 0.  A
 *            NaN m fails both comparisons: both streaks reset.
 *   3 fire      fire_resign = resign_patience > 0 && rs[colour] >= resign_patience && root_ply >= resign_min_ply; fire_draw likewise with ds,
 *            draw_patience, draw_min_ply.  Resign wins over draw.  Every sz_play of the board counts, whatever budget or visit target (a
 *            goal-0 ply on kept visits included) its search had.
 *   4 holdout   on a board with holdout[b] != 0 a firing rule ends nothing: if would_ply < 0 it records would_ply = root_ply, would_kind,
 *            would_colour (counted in sz_ending_stats out[3]); the ply is played exactly as without the option; streaks go on counting.
 *   5 ending    on any other board the game ends instead of a move: no move is played, the ring, the position and game_ply are unchanged, no
 *            subtree is kept, the board is game-over with result +1 / -1 (white / black wins; a resigning mover loses) or 0.  The ply's
 *            record is written as always (planes, actions, visits: pruned if the board is forced) with chosen = -1, game_over = 1 and the
 *            result.  The board's uniform is not read.
 * The solver's WIN-root move rule and policy-target pruning are untouched where no ending fires.  Composes with sz_set_search_options (any L,
 * solver on or off), sz_set_forced_playouts, reuse_subtree, budgets, visit targets, sz_compact and sz_compact_searching.
 * Held bit for bit to the host restatement tests/endingref.py by tests/test_gpu_endings.py.  Its effect on playing strength is unmeasured. */
enum { SZ_END_NONE = 0, SZ_END_RESIGN = 1, SZ_END_DRAW = 2, SZ_END_PROVEN = 3 };
typedef struct sz_ending_options {
    float resign_value;  int32_t resign_patience, resign_min_ply;   /* value in [-1, 1]; patience 0 = rule off, else 1..65535; min_ply >= 0 */
    float draw_value;    int32_t draw_patience,   draw_min_ply;     /* value in [0, 1] */
    int32_t proven;                                                  /* ignored while the solver is off */
} sz_ending_options;
/* opt == NULL switches the option off (holdout is ignored; state and counters stay); otherwise on, for every board, with `holdout` a HOST array
 * [n_boards] (NULL = no holdout board).  SZ_ERR_INVALID: a value outside its range or not finite, a patience outside 0..65535, a negative
 * min_ply.  SZ_ERR_STATE during a search (the rule of sz_set_search_budgets; nothing is changed then).  Takes effect at the next sz_play and
 * holds until changed.  Never drops kept subtrees and never resets streaks or marks: a host calls it at every refill with a new `holdout`. */
int sz_set_endings(sz_engine* e, const sz_ending_options* opt, const uint8_t* holdout, void* stream);
/* HOST arrays [n_boards], any may be NULL; synchronises.  kind[b] (SZ_END_*) and mover_value[b] (m) describe the last sz_play: 0 and NaN for a
 * board that did not play in it, and for every board while the option is off; kind is 0 for a game the rules ended or that goes on.
 * would_ply / would_kind / would_colour are the board's sticky holdout mark for its current game (-1 / 0 / 0 = none). */
int sz_fetch_endings(sz_engine* e, uint8_t* kind, double* mover_value, int32_t* would_ply, uint8_t* would_kind, uint8_t* would_colour, void* stream);
/* ending counters, all boards, cumulative since the option was first switched on (synchronises): out[0] resignations, out[1] adjudicated
 * draws, out[2] proven endings, out[3] holdout marks.  sz_stats is unchanged. */
int sz_ending_stats(sz_engine* e, uint64_t out[4], void* stream);
/* test: the DEVICE code of the ending decision (the function the option's k_play calls) on caller-supplied cases, one wavefront per case, in
 * the manner of sz_debug_forced.  Case c owns children offsets[c]..offsets[c+1] (1..SZ_MAX_MOVES each) of vc (N) and value_sum (f64);
 * root_proven[c] (codes of sz_root_proven), colour[c], ply[c], holdout[c], state_in[c*6..] = rs[0], rs[1], ds, would_ply, would_kind,
 * would_colour, opts[c].  Writes kind_out[c], m_out[c] and state_out[c*6..].  All device pointers. */
int sz_debug_endings(const int32_t* offsets_dev, const int32_t* vc_dev, const double* value_sum_dev, const int8_t* root_proven_dev, const uint8_t* colour_dev,
                     const int32_t* ply_dev, const uint8_t* holdout_dev, const int32_t* state_in_dev, const sz_ending_options* opts_dev,
                     int32_t* kind_out_dev, double* m_out_dev, int32_t* state_out_dev, int32_t n_cases, void* stream);

/* NON-REFERENCE option, off by default: MOVE-SELECTION TEMPERATURE with a visit offset and a value cutoff (AlphaZero, lc0 TempVisitOffset /
 * TempValueCutoff, KataGo).  The reference samples every self-play move from the root's visit counts at temperature 1 (sim.py:68-76), at ply
 * 150 as at ply 1, and the only alternative is a negative uniform, the most visited move.  With the option on sz_play samples child c with a
 * probability proportional to (n_c + visit_offset)^(1/T), T a number per board that the caller rewrites between plies, and never samples a
 * move whose value lies more than value_cutoff below the most visited move's: a one-visit blunder is not played in a won game.  The schedule
 * (T by ply, by game, by fast or full search) is the caller's: the engine reads temps_dev[b] and nothing else.  Never switched on, every kernel
 * that runs today runs unchanged: the option is an instantiation of k_play of its own, k_play<SOLVE, [ForcedOpts,] TempOpts[, EndOpts]>;
 * k_search_begin, k_search_step and k_play_moves have none.
 * The rule, per board that passes sz_play's early return (searching, done, no error, game not over) and its zero-visit check, after the ending
 * decision of sz_set_endings (an ending that fires reads neither uniform nor temperature: nothing below happens on that board) and after
 * policy-target pruning.  All arithmetic is f64, every operator one IEEE rounding (-ffp-contract=off); slog, sexp and SZG_EXP_CUTOFF are
 * sz_set_gumbel's (csrc/sz_gumbel.h):
 *   inputs    the root's children c = 0..K-1 in action order.  n_c = the counts today's sampling reads: the counted visits, or the pruned
 *             counts n' of sz_set_forced_playouts on a forced board.  N_c, W_c = the tree's counted visits and value sums, never pruned.
 *             T = temps_dev[b], u = uniforms_dev[b], both read once.  c* = the first maximum of n_c in child order (n_c* >= 1 after the
 *             zero-visit check; pruning leaves the first maximum where it was).  off = (double)visit_offset.
 *   solver    on a root proven WIN the move is the first child proven LOSS, as without the option, whatever T and u are.
 *   greedy    otherwise, if u < 0.0, or !(T > 0.0) (zero, negative, NaN), or a_c* <= 0.0 with a_c = (double)n_c + off: the move is c*, exactly
 *             the negative-uniform path of sz_play.
 *   eligible  otherwise the move is sampled.  m_c = -(W_c / (double)N_c), the mover's expected outcome of move c (wave_ending's convention; N_c
 *             >= n_c >= 1 where it is read).  Child c is eligible iff n_c >= 1 && a_c > 0.0 && (!use_cutoff || m_c >= m_c* - (double)value_cutoff).
 *             c* is eligible: a_c* > 0.0 here, and m_c* >= m_c* - cutoff for a finite m_c* and a cutoff >= 0 (W is a finite sum of values in
 *             [-1, 1]).  Every positive a_c is a normal number, which is what slog asks for: n_c is an integer >= 1 and off the double of an
 *             f32, so a sum below 0.5 has |off| > 0.5, is exact (Sterbenz) and is a multiple of off's f32 spacing, at least 2^-24; the sums
 *             from 0.5 on are normal anyway.
 *   weights   w_c = 0.0 for a child that is not eligible.  For an eligible child w_c = a_c when T == 1.0, else
 *             d_c = slog(a_c) - slog(a_c*); if (d_c > 0.0) d_c = 0.0; w_c = sexp(d_c / T): normalised by the largest, since 800^20 (N = 800 at
 *             T = 0.05) has no f64.  a_c <= a_c*, so d_c is positive only by slog's own rounding, between neighbouring doubles under an
 *             offset of 2^22 and more; the clamp keeps sexp's argument at or below 0.0 whatever T is.  For every child with n_c = n_c* the
 *             argument is exactly 0.0 and w = sexp(0.0) = 1.0 exactly.  A weight whose argument lies below SZG_EXP_CUTOFF is 0.0; the child
 *             still counts as eligible.
 *   sampling  today's two sequential passes of one lane, in child order, with w_c in the place of (double)n_c and S, the sequential sum of
 *             w_c starting from 0.0, in the place of (double)total: acc = 0.0; acc += w_c / S for every c; last = acc; then acc = 0.0,
 *             idx = 0 and for every c: acc += w_c / S; if (acc / last <= u) idx = c + 1; at the end idx = min(idx, K - 1).  A child of weight
 *             0.0 leaves acc as it is, so for u in [0, 1) the move has a positive weight: no child that is not eligible is ever played.
 *             With T == 1.0, off == 0.0 and no cutoff w_c = (double)n_c and S = (double)total exactly (integer-valued doubles add exactly):
 *             the arithmetic of sz_play without the option, bit for bit.
 *   outputs   n_eligible[b] = the number of eligible children and p_chosen[b] = w_move / S of the last sz_play; 1 and 1.0 on a greedy or
 *             proven-win play; 0 and NaN for a board that did not play a move in it (early return, zero visits, a game ended by
 *             sz_set_endings), and for every board while the option is off.  Counters, per board, cumulative: out[0] plays sampled by the
 *             rule, out[1] greedy plays under the option (proven-win plays included), out[2] children with n_c >= 1 that a sampled play
 *             found not eligible.
 *   record    unchanged: action and visits (pruned where forced) as without the option, `chosen` the action played.  The policy target is not
 *             tempered.  With reuse_subtree the subtree kept is the played child's, as always.
 * Composes with sz_set_search_options (any L, solver on or off), sz_set_forced_playouts, sz_set_endings, sz_set_fpu, reuse_subtree, budgets,
 * visit targets, root noise, sz_compact, sz_compact_searching and sz_play_moves: k_play is independent of all of them.  Gumbel chooses its own
 * move: see the setter.  Held bit for bit to the host restatement tests/tempref.py by tests/test_gpu_temperature.py.  Its effect on playing
 * strength is unmeasured. */
typedef struct sz_temperature_options {
    float   visit_offset;   /* added to every count before the power (lc0 TempVisitOffset); finite, any sign; 0 = none */
    float   value_cutoff;   /* >= 0, finite: a move whose mover value lies more than this below the most visited move's is not sampled (lc0 TempValueCutoff) */
    int32_t use_cutoff;     /* 0 = value_cutoff ignored (and not checked) */
} sz_temperature_options;                         /* 12 bytes */
/* opt == NULL switches the option off (temps_dev is ignored; the counters stay); otherwise on, for every board.  temps_dev: device array
 * [n_boards] of f64, read by every sz_play while the option is on; the caller rewrites its contents between plies, as it does with
 * uniforms_dev, and keeps it alive until the option is off or set anew.  SZ_ERR_INVALID: e NULL; opt != NULL with temps_dev NULL; visit_offset
 * not finite; with use_cutoff != 0 a value_cutoff that is negative or not finite.  SZ_ERR_STATE: a call during a search (the rule of
 * sz_set_search_budgets; nothing is changed then); switching on while Gumbel is on for the next search, and sz_set_gumbel(opt != NULL)
 * refuses with SZ_ERR_STATE while this option is on.  Takes effect at the next sz_play and holds until changed.  Never drops kept subtrees.
 * The arrays (weights [n_boards][SZ_MAX_MOVES] f64, the two outputs, the counters) are allocated by the first enabling call. */
int sz_set_move_temperature(sz_engine* e, const sz_temperature_options* opt, const double* temps_dev, void* stream);
/* HOST arrays [n_boards], either may be NULL; synchronises.  n_eligible and p_chosen of the last sz_play as the rule's `outputs` says. */
int sz_fetch_temperature(sz_engine* e, int32_t* n_eligible, double* p_chosen, void* stream);
/* temperature counters, all boards, cumulative since the option was first switched on (synchronises): out[0] sampled plays, out[1] greedy
 * plays, out[2] excluded children.  sz_stats is unchanged. */
int sz_temperature_stats(sz_engine* e, uint64_t out[3], void* stream);
/* test: the DEVICE code of the move choice (the function the option's k_play calls) on caller-supplied cases, one wavefront per case, in the
 * manner of sz_debug_endings.  Case c owns children offsets[c]..offsets[c+1] (1..SZ_MAX_MOVES each, else chosen_out -1) of vc (n_c, the counts
 * sampled from), tree_vc (N_c; NULL = vc) and value_sum (W_c, f64); temps[c] (T), uniforms[c] (u), proven_move[c] (the proving move of a
 * WIN root, -1 = none; the array may be NULL) and opts[c] (not checked).  Writes per case the move, how it was chosen (0 sampled, 1 greedy,
 * 2 proven win), n_eligible, p_chosen and the number of excluded children, and for a sampled case every child's weight w_c into
 * weights_out[offsets[c]..] (left as it is otherwise).  All device pointers. */
int sz_debug_temperature(const int32_t* offsets_dev, const int32_t* vc_dev, const int32_t* tree_vc_dev, const double* value_sum_dev, const double* temps_dev,
                         const double* uniforms_dev, const int32_t* proven_move_dev, const sz_temperature_options* opts_dev, int32_t* chosen_out_dev,
                         int32_t* kind_out_dev, int32_t* n_eligible_out_dev, double* p_chosen_out_dev, int32_t* excluded_out_dev, double* weights_out_dev,
                         int32_t n_cases, void* stream);

/* NON-REFERENCE option, off by default: a VISIT-DEPENDENT EXPLORATION RATE (AlphaZero's c(s) = log((1 + N(s) + c_base) / c_base) + c_init with
 * c_base = 19652, c_init = 1.25; lc0's CPuct + CPuctFactor * log((N + CPuctBase) / CPuctBase) with a second triple for the root).  Selection
 * everywhere is q + c * P * sqrt(n_p) / (1 + n_c) with the one constant c = sz_config.c_puct (Node.get_ucb).  With the option on c grows with the
 * parent's visit count, by one triple (init, base, factor) for the board's root and one for every node below it.  The growth matters at 800
 * simulations and more, and where a kept root starts a search with hundreds of visits (reuse_subtree, sz_set_visit_targets).  Never switched
 * on, every kernel that runs today runs unchanged: the option is an instantiation of its own, PuctOpts after FpuOpts and before TempOpts in the
 * pack: k_search_step<VL, SOLVE, [ForcedOpts,] [FpuOpts,] PuctOpts>, and k_play<SOLVE, ForcedOpts, PuctOpts[, TempOpts][, EndOpts]> because
 * policy-target pruning is k_play's only use of c.  k_search_begin and k_play_moves have no variant.
 * The rule:
 *   site       the root triple is used where a child of the root is selected (depth 0 of a descent, of a fresh and of a continued search alike)
 *              and by policy-target pruning; the tree triple is used at depth >= 1.
 *   n_p        the parent count that selection's sqrt already reads: in k_search_step N_p, or N_p + k_p under leaf batching (k_p the parent's
 *              in-flight count); in policy-target pruning the root's counted N.  A kept root's visits count (and a fresh root's N carries the
 *              reference's extra 1 of mcts.py:46, as in the sqrt).
 *   c          all in f64, every operator one IEEE rounding (-ffp-contract=off); slog is sz_set_gumbel's (csrc/sz_gumbel.h):
 *                x = (((double)n_p + (double)base) + 1.0) / (double)base
 *                c = (float)((double)init + (double)factor * slog(x))
 *              This f32 takes c_puct's place in ucb_value / ucb_u, whose operation order is not touched.  x > 1 always (base >= 1, n_p >= 0), so
 *              slog's precondition holds.  AlphaZero is (1.25, 19652, 1); lc0's form is the same up to the + 1.  The scalar function is
 *              sz_cpuct in csrc/sz_cpuct.h, plain C++ for host and device; it is evaluated once per selection, uniform across the wave, and
 *              not cached per node.
 *   identity   at factor == 0, c == init exactly: an engine with the option at (C, any base, 0) at both sites builds the trees and records of
 *              the engine without the option and c_puct = C, bit for bit, through different kernels.
 *   unchanged  q, the first-play rule of sz_set_fpu (its u takes the same c), the forced-child rule n_c < sqrt(k P_c T), the arg-max and its
 *              tie-break, the solver's skipping of WIN children, virtual loss, and sz_play's sampling.
 *   pruning    wave_prune reads the root triple's c at the root's counted N for both `best` and the candidates' u.
 * sz_search_begin latches the setting, like sz_set_fpu's: a search, its steps and its sz_play (which prunes under what its search ran under)
 * see what their sz_search_begin saw.  Only selection and pruning change and the tree is never modified: kept subtrees are never dropped.
 * Composes with sz_set_search_options (any L, solver, reuse), budgets, visit targets, root noise, forced playouts, sz_set_fpu, endings, the
 * move temperature, sz_compact, sz_compact_searching and sz_play_moves.  Gumbel exists for 16 to 64 simulations, where the growth is nil, and
 * its restatement is a separate chain: the two refuse each other, see the setter; combining them is a follow-up.
 * Held bit for bit to the host restatement tests/puctref.py by tests/test_gpu_cpuct.py.  Its effect on playing strength is unmeasured. */
typedef struct sz_cpuct_options {
    float tree_init, tree_base, tree_factor;      /* every node below the root */
    float root_init, root_base, root_factor;      /* the board's root (depth 0 of a descent) and policy-target pruning */
} sz_cpuct_options;                               /* 24 bytes */
/* opt == NULL switches the option off: the kernels that run without it then run, with sz_config.c_puct.  SZ_ERR_INVALID (nothing is changed):
 * a field that is not finite, an init outside [0, 100], a factor outside [0, 100], a base outside [1, 1e9].  SZ_ERR_STATE: a call during a
 * search (the rule of sz_set_search_budgets; nothing is changed then); switching on while Gumbel is on for the next search, and
 * sz_set_gumbel(opt != NULL) refuses with SZ_ERR_STATE while this option is on.  Takes effect at the next sz_search_begin and holds until
 * changed. */
int sz_set_cpuct(sz_engine* e, const sz_cpuct_options* opt, void* stream);
/* test: the DEVICE code of the rate (sz_cpuct as the option's kernels call it) on caller-supplied cases, one lane per case, in the manner of
 * sz_debug_gumbel's maths part: c_out[i] = the c of opts[i] at parent count n_p[i], by the root triple where is_root[i] != 0 and the tree triple
 * otherwise.  opts are not checked.  All device pointers. */
int sz_debug_cpuct(const int32_t* n_p_dev, const uint8_t* is_root_dev, const sz_cpuct_options* opts_dev, float* c_out_dev, int32_t n_cases, void* stream);

/* NON-REFERENCE option, default off: KLD-gain early stopping of a board's search (lc0's minimum-kldgain-per-node / kldgain-average-interval;
 * its training runs used 5e-6 and 100).  Every other option changes where a simulation goes; this one lets a board stop when further
 * simulations no longer change its answer: the root's visit distribution is compared with its last snapshot at check points the caller chooses,
 * and the board's goal is lowered to what it has made and has in flight when the Kullback-Leibler gain per new visit is below min_gain.
 * Never switched on, every kernel that runs today runs unchanged, and with it on too: k_search_begin, k_search_step and k_play have no variant.
 * The rule lives in small kernels of its own beside them; the search kernels read the board's goal where they read a budget.
 * Per-board state, reset by sz_search_begin for every board that starts a search, fresh or continued: prev[SZ_MAX_MOVES] (int32, the root
 * children's N at the last snapshot), prev_total = 0, has_prev = 0, stopped_at = -1, checks = 0, last_gain = NaN.
 * The check (sz_search_check_stop), one wavefront per board, for a board that searches, is not done, not in error and has stopped_at < 0:
 *   1. K = the root's child count.  K == 0 (the root is not expanded yet): nothing happens.
 *   2. now_c = N_c of the root's children in action order: counted visits only, the in-flight counts k of leaf batching are not included.
 *      new_total = sum of now_c, in integer arithmetic.
 *   3. new_total < prev_total + interval: nothing happens.
 *   4. has_prev != 0 and prev_total > 0: the gain is formed, all in f64, every operator one IEEE rounding (-ffp-contract=off); slog is
 *      sz_set_gumbel's (csrc/sz_gumbel.h), the term is sz_kld_term in csrc/sz_kldgain.h, plain C++ for host and device:
 *        for every child with prev_c != 0:  o = (double)prev_c / (double)prev_total;  n = (double)now_c / (double)new_total;
 *                                           term_c = o * slog(o / n)              (0.0 for a child with prev_c == 0)
 *        gain = the sum of the terms in the fixed order: lane l adds term_l, term_{l+64}, ... ascending from 0.0, then the xor butterfly
 *               (offsets 32, 16, .., 1: acc = acc + other)
 *        g = gain / (double)(new_total - prev_total);  last_gain = g;  checks += 1
 *      Visits never fall within a search, so now_c >= prev_c > 0 and slog's precondition holds.  The board stops iff
 *      g < min_gain && sims_done >= min_simulations (sims_done: the new simulations this search has made).
 *   5. a stop: stopped_at = goal[b] = sims_done + pending, pending the board's leaves in flight (n_pend under leaf batching, else 1 while
 *      the board waits for the network, else 0).  Nothing else on the board changes: the next sz_search_step consumes what is in flight,
 *      finds its simulations made, starts no descent and sets the board done.  A board with nothing in flight is set done by the check.
 *   6. otherwise, the first evaluated check included, which only takes the snapshot: prev = now, prev_total = new_total, has_prev = 1.
 * The goals: while the option is on every kernel reads a board's simulations from one array, which sz_search_begin fills for every board: the
 * goal sz_set_visit_targets derives, else the board's budget (sz_set_search_budgets), else num_searches.  sz_search_goals reports that value,
 * sz_fetch_kld_stop where the board stopped.  Budgets and targets work underneath; the option only ever lowers a goal.
 * The invariant: a board stopped at s ends with the tree, record and counters of the same search run with goal s from the start (as a budget,
 * or on a reuse_subtree engine as the visit target s + N_kept - 1), bit for bit; under leaf batching the last gather ended at
 * sims_done + pending == s either way.
 * Composes with budgets, visit targets, reuse_subtree (a kept root's children carry their visits into the first snapshot), leaf batching,
 * the solver (a proven root is done before any check), forced playouts, sz_set_fpu, sz_set_cpuct, root noise, endings, the move temperature,
 * sz_compact and sz_compact_searching.  sz_set_gumbel plans sequential halving on the goal: the two refuse each other, see the setter.
 * Held bit for bit to the host restatement tests/kldref.py by tests/test_gpu_kld_stop.py.  Its effect on playing strength is unmeasured. */
typedef struct sz_kld_stop_options {
    double  min_gain;          /* stop when the gain per new root-child visit is below this; finite, in (0, 1] */
    int32_t interval;          /* a check is evaluated only when the root's children gained >= interval visits since the last snapshot; 1..num_searches */
    int32_t min_simulations;   /* never stop a board before its search has made this many new simulations; 0..num_searches */
} sz_kld_stop_options;                            /* 16 bytes */
/* opt == NULL switches the option off.  SZ_ERR_INVALID (nothing is changed): min_gain not finite or outside (0, 1], interval outside
 * 1..num_searches, min_simulations outside 0..num_searches.  SZ_ERR_STATE: a call during a search (the rule of sz_set_search_budgets; nothing
 * is changed then); switching on while Gumbel is on for the next search, and sz_set_gumbel(opt != NULL) refuses with SZ_ERR_STATE while this
 * option is on.  The setter never touches a tree: kept subtrees survive a change.  Holds from the next sz_search_begin until changed. */
int sz_set_kld_stop(sz_engine* e, const sz_kld_stop_options* opt, void* stream);
/* the check above for every board: one kernel launch on `stream`, no synchronisation.  With the option off a successful no-op, so that a driver
 * may call it unconditionally.  SZ_ERR_STATE, as the host knows it without asking the device: before the first sz_search_begin, after sz_play /
 * sz_play_moves, and after a sz_compact_searching that found no board searching. */
int sz_search_check_stop(sz_engine* e, void* stream);
/* host arrays [n_boards], each may be NULL: stopped_at (-1: not stopped), checks and last_gain (NaN: none evaluated) of each board's last
 * search.  Synchronises the stream.  SZ_ERR_STATE when the option was never on. */
int sz_fetch_kld_stop(sz_engine* e, int32_t* stopped_at, int32_t* checks, double* last_gain, void* stream);
/* boards stopped early, checks evaluated, simulations not made (goal at begin - stopped_at), all boards, cumulative; zeros when never on */
int sz_kld_stop_stats(sz_engine* e, uint64_t out[3], void* stream);
/* test: the DEVICE code of the gain (wave_kld_gain as k_kld_check calls it) on caller-supplied cases, one wavefront per case: prev / now are
 * [n_cases][SZ_MAX_MOVES] int32, n_child[i] in 0..SZ_MAX_MOVES the children of case i, the totals are the integer sums of the first n_child[i]
 * entries; gain_out[i] = the summed gain, before the division by the new visits.  All device pointers. */
int sz_debug_kld_gain(const int32_t* prev_dev, const int32_t* now_dev, const int32_t* n_child_dev, double* gain_out_dev, int32_t n_cases, void* stream);

/* NON-REFERENCE option, default off: the search summary.  Every other option changes where a simulation goes, when a search stops or which move
 * is played; this one changes nothing and records what a finished search hands to a trainer beside the visit counts: the search's own value of
 * the root (lc0 trains its value head on (1 - q_ratio) * z + q_ratio * q) and how far the policy target lies from the prior the search started
 * from (KataGo's policy surprise weighting).  While it is on sz_play launches two more kernels on the caller's stream, k_summary_pre before
 * k_play (the tree is intact: k_play compacts it in place under reuse_subtree) and k_summary_post after it (the ply's record exists: the pruned
 * counts of a forced-playouts board exist nowhere else).  k_play, k_search_begin, k_search_step and k_play_moves run unchanged, on or off.
 * One wavefront per board.  All arithmetic is f64, every operator one IEEE rounding (-ffp-contract=off); slog is sz_set_gumbel's
 * (csrc/sz_gumbel.h), the term o * slog(o / n) is csrc/sz_kldgain.h's sz_kld_term, the scalar functions are csrc/sz_summary.h's, plain C++ for
 * host and device.
 *   wsum(term): sz_set_gumbel_tree's fixed-order sum: lane l adds the terms c = l, l + 64, l + 128, l + 192 ascending from 0.0, then the xor
 *               butterfly with offsets 32, 16, .., 1 (acc = acc + other); the result is read through readfirstlane.
 * Before k_play, for a board that plays in this sz_play (it searches, is done, has no error, its game is not over: k_play's early return,
 * restated) and passes k_play's zero-visit check (K > 0 and total > 0; otherwise k_play sets SZ_ERR_ZERO_VISITS):
 *   K = the root's child count; for the children in the tree's order N_c (counted visits, no in-flight count), W_c (f64, stored from the
 *   child's side to move), P_c (f32, the stored prior the search used: the noised one where root noise is on)
 *   total  = the sum of N_c, in integer arithmetic
 *   root_q = -(wsum(N_c >= 1 ? W_c : 0.0) / (double)total)      the mover's expected outcome over the whole search, in [-1, 1]
 *   best_q = -(W_c* / (double)N_c*), c* the first maximum of N_c: the m of sz_set_endings, bit for bit
 *   valid = 1, surprise = NaN, and the K priors are kept for the second kernel
 * Any other board: valid = 0, root_q = best_q = surprise = NaN.
 * After k_play, for a board with valid = 1, on the record k_play just wrote (sz_fetch_ply's; its child order is the tree root's, see
 * csrc/sz_summary.h; an ending that fires still writes it):
 *   n_c = visits[c] for c < n_child: the pruned counts on a forced-playouts board, the policy target as trained on
 *   rtotal = the sum of n_c, in integer arithmetic;  rtotal == 0: surprise = NaN
 *   t_c = (double)n_c / (double)rtotal;  term_c = n_c > 0 ? t_c * slog(t_c / (double)P_c) : 0.0;  surprise = wsum(term_c)
 *   a P_c that is not a normal positive finite f32 (expansion stores none): term_c = 0.0 and the term is counted, see the stats
 * The priors are read as the tree stores them.  Where they sum to 1 (learning off, or Dirichlet root noise: sz_set_root_noise /
 * sz_set_search_root_noise) surprise is KL(target || prior) up to rounding: >= 0 but for a few ulp of the largest term, and exactly 0.0 at
 * K = 1 with P_0 = 1.  Under the reference's learning noise every stored prior is 0.75 p + 0.25 * noise_value with noise_value near 1: they
 * sum to more than 1 and the same sum can be negative; it is reported as it is.
 * Composes with budgets, visit targets, reuse_subtree, leaf batching, the solver, forced playouts, sz_set_fpu, sz_set_cpuct, root noise, the move
 * temperature, sz_set_kld_stop, sz_set_endings, sz_compact and sz_compact_searching.  sz_play_moves makes no summary and leaves the last one as
 * it is.  sz_set_gumbel's record is pi' and it exports v_mix itself: the two refuse each other, see the setter.
 * Held bit for bit to the host restatement tests/summaryref.py by tests/test_gpu_search_summary.py.  Its effect on training is unmeasured. */
/* enable != 0 switches the option on, 0 off; takes effect at the next sz_play.  SZ_ERR_STATE: a call during a search (the rule of
 * sz_set_search_budgets; nothing is changed then); switching on while Gumbel is on for the next search, and sz_set_gumbel(opt != NULL) refuses
 * with SZ_ERR_STATE while this option is on.  The setter never touches a tree.  The first enabling call allocates the per-board arrays. */
int sz_set_search_summary(sz_engine* e, int32_t enable, void* stream);
/* host arrays [n_boards], each may be NULL: the summary of each board's last sz_play made with the option on (valid = 0 and NaNs: the board
 * did not play then, or no sz_play was made yet).  Synchronises the stream.  SZ_ERR_STATE when the option was never on. */
int sz_fetch_search_summary(sz_engine* e, double* root_q, double* best_q, double* surprise, uint8_t* valid, void* stream);
/* out[0] = summaries made, out[1] = surprise terms dropped by the rule on P_c above, all boards, cumulative; zeros when never on */
int sz_search_summary_stats(sz_engine* e, uint64_t out[2], void* stream);
/* test: the DEVICE functions the two kernels call (wave_summary_values, wave_summary_surprise) on caller-supplied cases, one wavefront per case:
 * tree_vc / record_vc are [n_cases][SZ_MAX_MOVES] int32, value_sum [n_cases][SZ_MAX_MOVES] f64, prior [n_cases][SZ_MAX_MOVES] f32, n_child[i] in
 * 0..SZ_MAX_MOVES the children of case i.  out3[i] = root_q, best_q (NaN both when n_child[i] == 0 or the tree counts sum to 0), surprise (NaN
 * when the record counts sum to 0).  All device pointers. */
int sz_debug_search_summary(const int32_t* n_child_dev, const int32_t* tree_vc_dev, const double* value_sum_dev, const float* prior_dev, const int32_t* record_vc_dev,
                            double* out3_dev, int32_t n_cases, void* stream);

/* NON-REFERENCE option, default off: the spread of the values backed up through every edge, and lower-confidence-bound (LCB) move selection on
 * it (KataGo's useLcbForSelection, lcbStdevs = 5.0, minVisitPropForLCB = 0.15).  Every other option leaves what the tree knows about an edge at
 * W, N, P; with this one on the tree also keeps Q, the sum of the squares of the values W sums, and where sz_play would play "the most visited
 * move" it plays, among the well-visited root moves, the one whose mean value is best after z standard errors are taken off.
 * All arithmetic is f64, every operator one IEEE rounding (-ffp-contract=off); ssqrt and the scalar functions are csrc/sz_lcb.h's, plain C++
 * for host and device (ssqrt: a square root from + - * / and bit operations; ssqrt(0.0) = 0.0; an argument that is neither 0.0 nor a positive
 * normal number counts as 0.0 and is counted, see the stats).
 * The second moment.  Q is one f64 per edge, [n_boards][edges], allocated by the first enabling call (8 bytes per edge beside the tree's 32).
 * It is written by the searches begun with the option on, at these sites and nowhere else, in the order W is written:
 *   Q[e] = 0.0            where an edge is created: the root edge of a fresh root (sz_search_begin), the children at expansion (sz_search_step)
 *   Q[e] = Q[e] + sv * sv wherever sv is added to W[e] in a backup, sv = +v or -v by the level's parity, v the (double) of the network's f32
 *                         value or a terminal / proven -1, 0, +1: the evaluated leaf (under leaf batching every pending leaf, in leaf order), a
 *                         visited terminal, a new terminal, the solver's proven stop (a proven root counts the rest of its budget out this
 *                         way, one simulation at a time).  The product is exact, the sum one rounding.
 *   Q[0] = (tv * tv) * (double)S   the terminal root, whose budget S is counted out at once beside W[0] = tv * (double)S
 * The move choice, in sz_play, for a board that passes its early return and zero-visit check, after the ending decision (an ending that fires
 * makes no choice) and after policy-target pruning.  The root's children c = 0..K-1 in action order; n_c the counts the move choice reads
 * (pruned on a forced-playouts board); N_c, W_c, Q_c the tree's, never pruned; c* the first maximum of n_c; z = (double)stdevs,
 * p = (double)min_visit_prop.  For a child with N_c >= 2:
 *   m_c   = -(W_c / (double)N_c)                                       the mover's value, sz_set_endings' convention
 *   s_c   = Q_c / (double)N_c - m_c * m_c;  if (!(s_c > 0.0)) s_c = 0.0
 *   r_c   = z * ssqrt(s_c / (double)(N_c - 1))                          z standard errors of the mean, with the unbiased variance
 *   lcb_c = m_c - r_c
 * and lcb_c = NaN for a child with N_c < 2.  Child c is a candidate iff N_c >= 2 && n_c >= 1 && (double)n_c >= p * (double)n_c*.  The rule's
 * move is the first maximum of lcb_c over the candidates (lanes = children; each lane keeps its first strict maximum over c, c + 64, ..; the
 * wave64 xor butterfly keeps the larger value and the lower index on a tie, as in selection); without a candidate it is c*.
 * Where it applies: exactly where sz_play would play the most visited move: a negative uniform without sz_set_move_temperature, the greedy kind
 * of that option with it (u < 0, T not above 0, or no count above minus the offset).  A sampled play is chosen as without the option, and on
 * a root proven WIN the proving move is played as without it.  With select == 0 the option observes: the move is always the one without the
 * option, while Q, the outputs and the counters are produced all the same.
 * Not combined with reuse_subtree (the kept subtree's Q would have to be compacted with it) nor with sz_set_gumbel: follow-ups, see the setter.
 * Composes with budgets, leaf batching, the solver, forced playouts, sz_set_fpu, sz_set_cpuct,
 * root noise, the move temperature, sz_set_kld_stop, sz_set_endings, the search summary, sz_compact and sz_compact_searching.
 * Held bit for bit to the host restatement tests/lcbref.py by tests/test_gpu_lcb.py.  Its effect on playing strength is unmeasured. */
typedef struct sz_lcb_options {
    float stdevs;                 /* z >= 0, finite; KataGo: 5.0 */
    float min_visit_prop;         /* p in [0, 1]; KataGo: 0.15 */
    int32_t select;               /* != 0: the rule's move is played where it applies; 0: observe only */
} sz_lcb_options;                 /* 12 bytes */
/* opt == NULL switches the option off.  Takes effect at the next sz_search_begin, whole: a search, its steps and its sz_play run with what its
 * sz_search_begin saw, and a sz_play after a search that was begun without the option plays as without it.  SZ_ERR_INVALID: stdevs not finite
 * or negative, min_visit_prop outside [0, 1] or NaN.  SZ_ERR_STATE: a call during a search (nothing is changed then); switching on on a
 * reuse_subtree engine; switching on while Gumbel is on for the next search, and sz_set_gumbel(opt != NULL) refuses with SZ_ERR_STATE while this
 * option is on for the next search.  The setter never touches a tree.  The first enabling call allocates Q and the per-board arrays. */
int sz_set_lcb(sz_engine* e, const sz_lcb_options* opt, void* stream);
/* host arrays [n_boards], each may be NULL: what the rule found at each board's last sz_play made under the option.  move: the rule's move as a
 * child index; cstar: c*; lcb_move / lcb_cstar: their bounds (NaN where the child has N < 2); n_candidates; decided: 1 when the rule decided
 * the move played (it applied and select != 0).  A board that made no choice then (it did not play, an ending fired, zero visits), or before
 * any such sz_play: -1, -1, NaN, NaN, 0, 0.  Synchronises the stream.  SZ_ERR_STATE when the option was never on. */
int sz_fetch_lcb(sz_engine* e, int32_t* move, int32_t* cstar, double* lcb_move, double* lcb_cstar, int32_t* n_candidates, uint8_t* decided, void* stream);
/* out[0] = plays the rule decided, out[1] = plays at which the rule's move differs from c* (decided or not: sampled plays and select == 0
 * count), out[2] = ssqrt arguments treated as 0.0 (expect 0), all boards, cumulative; zeros when never on */
int sz_lcb_stats(sz_engine* e, uint64_t out[3], void* stream);
/* the root children's Q_c of every board, device f64 [n_boards][SZ_MAX_MOVES] in sz_root_children's order, 0.0 beyond the children; on the
 * caller's stream, not synchronised.  SZ_ERR_STATE unless the search begun last ran with the option. */
int sz_root_value_spread(sz_engine* e, double* sq_sum_dev, void* stream);
/* test: every edge's Q of one board in sz_debug_tree's order (host array, may be NULL for the count alone).  SZ_ERR_STATE as above. */
int sz_debug_tree_spread(sz_engine* e, int32_t board, int32_t max_nodes, double* sq_sum, int32_t* n_out, void* stream);
/* test: the DEVICE functions of the option on caller-supplied data.  Two parts, each skipped when its first array is NULL.  ssqrt_out[i] =
 * ssqrt(x[i]) for i < n_x, x_bad_out[i] (optional) = 1 where the argument was treated as 0.0.  wave_lcb, the function k_play calls, one
 * wavefront per case: case i has the children offsets[i] .. offsets[i + 1] - 1 (1..SZ_MAX_MOVES of them) of the flat arrays vc (n_c), tree_vc
 * (N_c), value_sum (W_c), sq_sum (Q_c) and the options opts[i]; move_out / cstar_out / n_candidates_out / bad_out [n_cases], lcb_out flat like
 * the inputs: every child's lcb_c.  All device pointers. */
int sz_debug_lcb(const double* x_dev, double* ssqrt_out_dev, int32_t* x_bad_out_dev, int32_t n_x, const int32_t* offsets_dev, const int32_t* vc_dev,
                 const int32_t* tree_vc_dev, const double* value_sum_dev, const double* sq_sum_dev, const sz_lcb_options* opts_dev, int32_t* move_out_dev,
                 int32_t* cstar_out_dev, int32_t* n_candidates_out_dev, int32_t* bad_out_dev, double* lcb_out_dev, int32_t n_cases, void* stream);

/* diagnostic only: with a device buffer of n_boards*8 uint64, sz_search_step records s_memtime at its phase boundaries per board
 * (0 start, 1 after expand+backprop, 2 after select, 3 after move/movegen/repetition/terminal, 4 after encode); NULL = off (default) */
int sz_debug_step_stamps(sz_engine* e, void* dev_buffer);

/* test / debug readback of the pending leaves: legal-move mask [n_boards,73] uint64 (bit v of word p =
 * action p*64+v), leaf depth, node count, edge count, status per board (host pointers, may be NULL). */
int sz_debug_pending(sz_engine* e, uint64_t* mask, int32_t* depth, int32_t* n_nodes, int32_t* n_edges,
                     int32_t* status, void* stream);
/* test / inspection: the WHOLE tree of one board after a search, depth-first in child order (= a recursive walk over Node.children
 * of mctsnode.py:7-18).  Row 0 is the root itself (depth -1, action -1); rows 1.. are its descendants: depth (0 = root child),
 * action index (action_taken), visit_count, value_sum (f64), prior (f32).  Host arrays of max_nodes entries (may be NULL to count);
 * *n_out = number of nodes in the tree. */
int sz_debug_tree(sz_engine* e, int32_t board, int32_t max_nodes, int32_t* depth, int32_t* action, int32_t* visits, double* value_sum,
                  float* prior, int32_t* n_out, void* stream);
/* test: the DEVICE code of Node.select / Node.get_ucb (mctsnode.py:23-37) on caller-supplied children, one wavefront per case.
 * Case c owns children offsets[c]..offsets[c+1] (<= SZ_MAX_MOVES each) of vc (visit_count), value_sum (f64), prior (f32); parent_visits[c],
 * c_puct[c].  Writes every child's UCB value and the selected child per case.  All device pointers. */
int sz_debug_select(const int32_t* offsets_dev, const int32_t* vc_dev, const double* value_sum_dev, const float* prior_dev,
                    const int32_t* parent_visits_dev, const float* c_dev, float* ucb_out_dev, int32_t* argmax_out_dev, int32_t n_cases, void* stream);
/* copy one board's current game position record (SZ_POS_BYTES) to the host */
int sz_debug_position(sz_engine* e, int32_t board, void* pos_out, int32_t* ply, void* stream);

/* ------------------------------------------------------------------ network tower (MFMA, gfx950) */

/* One fused layer of policyNN's tower (network.py:36-83 BasicBlock halves, :105 stem, :141 conv_p1):
 * conv (3x3 pad 1 or 1x1) with BatchNorm folded + bias (+ residual) (+ ReLU); NHWC bf16 in/out, f32 accumulate.
 * in [n_boards,64,cin] (cin 128 or 256), out/residual [n_boards,64,256], bias [256] f32, w_packed from sz_nn_pack_weights. */
int sz_nn_conv_bf16(const void* in, const void* w_packed, const float* bias, const void* residual, void* out,
                    int32_t n_boards, int32_t cin, int32_t ksize, int32_t relu, void* stream);
/* flag for `relu`/`flags` of the two entry points below: the weights were packed by sz_nn_pack_weights16 and the
 * 16x16x32 MFMA kernels are used (same results; the chip holds a higher clock on that shape) */
#define SZ_NN_W16 0x40000
/* flag for the stem (cin 128, ksize 3, SZ_NN_W16) and for sz_nn_tower_bf16: `in` is the engine's SZ_PLANES_NHWC128_BITS image */
#define SZ_NN_IN_BITS 0x1000000
/* One whole BasicBlock (network.py:36-83) in one launch: out = relu(conv3x3(relu(conv3x3(in,w1)+b1),w2)+b2+in); the
 * intermediate activation stays in LDS.  in/out [n_boards,64,256] bf16 NHWC, out != in. */
int sz_nn_block_bf16(const void* in, const void* w1_packed, const float* bias1, const void* w2_packed, const float* bias2, void* out,
                     int32_t n_boards, int32_t flags, void* stream);
/* host: torch conv weight [256,cin_real,k,k] f32 -> MFMA fragment order [k*k][cin_padded/16][8][64][8] bf16 */
int sz_nn_pack_weights(const float* w_in, int32_t cin_real, int32_t cin_padded, int32_t ksize, uint16_t* out);

int sz_nn_pack_weights16(const float* w_in, int32_t cin_real, int32_t cin_padded, int32_t ksize, uint16_t* out);
/* f16 operands instead of bf16 for sz_nn_tower_bf16 (in `flags`) and sz_nn_heads_bf16 (or-ed into `do_softmax`): v_mfma_f32_16x16x32_f16 runs at the bf16
 * rate and f16 keeps 11 bits of mantissa instead of 8; activations and BatchNorm-folded weights of this network are O(1), far inside f16's range.  The
 * weights are then packed with the _f16 packers, the tower output / heads input [n_boards,64,256] holds f16 bit patterns. */
#define SZ_NN_F16 0x8000000
int sz_nn_pack_weights16_f16(const float* w_in, int32_t cin_real, int32_t cin_padded, int32_t ksize, uint16_t* out);
int sz_nn_pack_head16_f16(const float* w_in, uint16_t* out);

/* The whole tower (network.py:176-184: stem conv + n_blocks BasicBlocks) in ONE persistent launch: a workgroup keeps its
 * boards' activations in LDS through all 1 + 2*n_blocks convolutions; only weights stream.  planes [n_boards,64,128] bf16
 * (SZ_PLANES_NHWC128_BF16; or _BITS with SZ_NN_IN_BITS), out [n_boards,64,256] bf16; w_packed / bias: HOST arrays of 1 + 2*n_blocks DEVICE pointers
 * (sz_nn_pack_weights16 order; [0] = stem packed with cin_padded = 128).
 * The workgroups that share an XCD start their tile rounds together (bounded wait on one arrival counter per XCD, allocated on first use), so a layer's
 * weights cross the fabric once per XCD and round; environment SZ_NN_PACE=0 switches that off.  Results do not depend on it. */
/* Two boards per workgroup when n_boards exceeds the number of CUs, else one (half the latency of a forward at small batches: a search of one position, the
 * tail of a self-play run); a board's result does not depend on the form.  SZ_NN_TOWER_WGB1 / _WGB2 force one (tests). */
#define SZ_NN_TOWER_WGB1 0x10000000
#define SZ_NN_TOWER_WGB2 0x20000000
int sz_nn_tower_bf16(const void* planes, const void* const* w_packed, const float* const* bias, int32_t n_blocks, void* out,
                     int32_t n_boards, int32_t flags /* SZ_NN_IN_BITS | SZ_NN_F16 | SZ_NN_TOWER_WGB* */, void* stream);
/* The same tower at the REFERENCE's precision class (network.py:176-184 is fp32 end to end) on the matrix cores: every operand carried as two bf16
 * numbers (hi = bf16(x), lo = bf16(x - hi): 16 bits of mantissa), every product as three MFMAs (hi*hi + lo*hi + hi*lo) with f32 accumulation, bias /
 * residual / ReLU in f32.  w_stream: ONE device buffer with the weights of the whole tower in k-step order, built on the host with
 * sz_nn_pack_split_stream (sz_nn_split_stream_elems(n_blocks) bf16 elements); bias: device [1 + 2*n_blocks][256] f32 (BatchNorm folded);
 * out [n_boards,64,256] F32 NHWC (the heads then run in fp32).  Two boards per workgroup when n_boards exceeds the number of CUs, else one; a
 * board's result does not depend on which (SZ_NN_SPLIT_WGB1 / _WGB2 force one form: tests).  About 100x closer to the fp32 network than
 * sz_nn_tower_bf16 at about 2.5x its time. */
#define SZ_NN_SPLIT_WGB1 0x2000000
#define SZ_NN_SPLIT_WGB2 0x4000000
int sz_nn_tower_split(const void* planes, const void* w_stream, const float* bias, int32_t n_blocks, float* out,
                      int32_t n_boards, int32_t flags /* SZ_NN_IN_BITS | SZ_NN_SPLIT_WGB* */, void* stream);
/* host: number of bf16 elements of the weight stream; one convolution (conv 0 = stem, cin_real 119; conv c >= 1: the c-th 256-channel 3x3
 * convolution in forward order) from the torch weight [256,cin_real,3,3] f32 into its place in the stream */
int64_t sz_nn_split_stream_elems(int32_t n_blocks);
int sz_nn_pack_split_stream(const float* w_in, int32_t cin_real, int32_t ksize /* 3; 1 for conv_p1 */, int32_t conv, uint16_t* stream);
/* The WHOLE network (network.py:176-192) at that precision class in two launches: the tower above with both heads fused onto each tile while it is still in
 * LDS — conv_p1 (packed into the stream as convolution 1 + 2*n_blocks with ksize 1, its folded bias as the last row of `bias`) -> ReLU -> conv_p2
 * (w_p2_packed from sz_nn_pack_split_head, 8*2*5*64*8 bf16 elements; b_p2 [73]) -> softmax over the 4672 logits, all on hi + lo operands; conv_v1 (wv [256],
 * bv: v_norm folded) in f32 — then the value MLP (sz_nn_value_mlp).  probs [n_boards,4672] f32 in the reference's flatten order (logits if !do_softmax),
 * value [n_boards], v1_scratch [n_boards*64] f32, tower_out: NULL or [n_boards,64,256] f32.  Every reduction runs in an order that does not depend on the
 * batch size or on the neighbours of a board: a position's policy and value are the same bit for bit at batch 1 and at batch 4096. */
int sz_nn_forward_split(const void* planes, const void* w_stream, const float* bias, int32_t n_blocks, const void* w_p2_packed, const float* b_p2,
                        const float* wv, float bv, const float* fc1_w_t, const float* fc1_b, const float* fc2_w, float fc2_b, float* probs, float* value,
                        float* v1_scratch, float* tower_out, int32_t n_boards, int32_t do_softmax, int32_t flags, void* stream);
int sz_nn_pack_split_head(const float* w_in /* conv_p2.weight [73,256] */, uint16_t* out);
/* SZ_NN_F16 in `flags` of sz_nn_tower_split / sz_nn_forward_split: hi + lo F16 operands (22 bits of mantissa: fp32's own class, logits 5e-7 from fp64) instead of hi + lo
 * bf16 (16 bits).  The stream and the head weights then come from the _f16 packers, which multiply the weights by 2^10 (exact; keeps the lo parts of weights down to 1e-3
 * normal f16 numbers); the caller passes the per-convolution biases (incl. conv_p1's) multiplied by 2^10 as well; the kernels scale every accumulator back. */
int sz_nn_pack_split_stream_f16(const float* w_in, int32_t cin_real, int32_t ksize, int32_t conv, uint16_t* stream);
int sz_nn_pack_split_head_f16(const float* w_in, uint16_t* out);
/* Training-step convolutions (train_RL.py:103-122 runs network.py:28,30's 3x3 convolutions forward and backward in fp32) at the reference's precision class on the
 * matrix cores: y = conv3x3(x, w), padding 1, no bias, 256 -> 256 channels; x, y device [n_boards,256,8,8] f32 NCHW.  w_stream (72*2048*16 bytes, device) comes from
 * sz_nn_pack_conv_split_dev(w [256,256,3,3] f32 device, transposed): transposed = 0 for the forward convolution, 1 for backward-data (the same kernel applied to the
 * output gradient).  zero256: device [256] f32 zeros.  f16 = 1 (both calls alike): hi + lo f16 operands (22 bits of mantissa: fp32's class) with exact power-of-two
 * scaling of the weights and of every board; f16 = 0: hi + lo bf16 (16 bits). */
int sz_nn_conv3x3_split_f32(const float* x, const void* w_stream, const float* zero256, float* y, int32_t n_boards, int32_t f16, void* amax_bits, void* stream);
/* weight gradient of the same convolution on hi + lo f16 operands: dw[co][ci][tap] = sum_b,pos gy[b][co][pos] * x[b][ci][pos + off(tap)].  amax_gy / amax_x: device uint32
 * with the f32 bit pattern of max|gy| / max|x| — the optional `amax_bits` output (f16 = 1; atomicMax into a zeroed word) of sz_nn_conv3x3_split_f32 run on those tensors;
 * part: device scratch, 16*9*256*256 f32; dw: device [256,256,3,3] f32, overwritten. */
int sz_nn_wgrad3x3_split_f32(const float* gy, const float* x, const void* amax_gy, const void* amax_x, float* part, float* dw, int32_t n_boards, void* stream);
int sz_nn_pack_conv_split_dev(const float* w, int32_t transposed, int32_t f16, void* w_stream, void* zero_u32 /* optional: device uint32 set to 0 = the amax_bits slot of the convolution that follows */, void* stream);
/* both streams of one convolution in one launch: w_stream (forward) and w_stream_t (backward-data), 72*2048*16 bytes each; zero_u32: optional device uint32[2], both set to 0 */
int sz_nn_pack_conv_split_both(const float* w, int32_t f16, void* w_stream, void* w_stream_t, void* zero_u32, void* stream);
/* One call per direction of a training convolution.  forward: pack (both streams when w_stream_t != NULL) + y = conv3x3(x, w); amax2: optional device uint32[2],
 * zeroed, slot 0 receives max|x|.  backward: gx = backward-data convolution of gy on w_stream_t (NULL: skipped; slot 1 of amax2 receives max|gy|), then dw = weight gradient
 * (NULL: skipped; f16 operands only; part: scratch as in sz_nn_wgrad3x3_split_f32). */
int sz_nn_conv3x3_train_fwd(const float* x, const float* w, int32_t f16, void* w_stream, void* w_stream_t, const float* zero256, float* y, int32_t n_boards, void* amax2, void* stream);
int sz_nn_conv3x3_train_bwd(const float* gy, const float* x, const void* w_stream_t, const float* zero256, float* gx, void* amax2, float* part, float* dw, int32_t n_boards,
                            int32_t f16, void* stream);
/* Train-mode BatchNorm2d + optional skip connection + ReLU in one launch per direction (network.py:62-83 under train_RL.py:103-122; csrc/sz_train.hip):
 * y = relu(bn(x) [+ residual]) with batch statistics over (boards, 8, 8) per channel, running statistics updated in place with `momentum` (NULL: not tracked),
 * save_mean / save_invstd [channels] kept for backward.  x, y, residual, gy, dx, dres: device [n_boards, channels, 8, 8] f32; dres NULL without a residual. */
int sz_bn_act_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps, const float* residual,
                        float* y, float* save_mean, float* save_invstd, int32_t n_boards, int32_t channels, void* stream);
int sz_bn_act_train_bwd(const float* gy, const float* x, const float* y, const float* gamma, const float* save_mean, const float* save_invstd, float* dx, float* dres,
                        float* dgamma, float* dbeta, int32_t n_boards, int32_t channels, void* stream);
/* value MLP alone (network.py:162-172): v1 [n_boards,64] f32 = relu(bn(conv_v1(x))) -> fc_v1 -> ReLU -> fc_v2 -> tanh -> value [n_boards] */
int sz_nn_value_mlp(const float* v1, const float* fc1_w_t, const float* fc1_b, const float* fc2_w, float fc2_b, float* value, int32_t n_boards, void* stream);
/* diagnostic only: device buffer of 256*4*16 uint64; sz_nn_tower_split then launches its stamped build (tools/split_stamps.py); NULL = shipped kernel */
int sz_nn_debug_split_stamps(void* dev_buffer, int32_t mode /* 1 = stamps; 2/3/4 = stamps + no weight loads / no LDS reads / neither (timing only) */);
/* diagnostic only: when set to a device buffer of 256*4*16 uint64, sz_nn_tower_bf16 launches its stamped build, which records
 * s_memtime at the phase boundaries of one block (tools/tower_stamps.py); NULL switches back to the shipped kernel */
int sz_nn_debug_tower_stamps(void* dev_buffer, int32_t mode /* 1 = stamps; 2/3/4 = stamps + no weight loads / no LDS reads / neither (timing only) */);
/* counter calibration only (tools/fetch_calib.py): reads `bytes` of src exactly once, 16 B per lane, with flat global loads (mode 0) or buffer loads (mode 1) */
int sz_debug_stream_read(const void* src, uint64_t bytes, int32_t mode, void* sink16, void* stream);
/* Heads of policyNN (network.py:141-174) as two small kernels:
 *  policy: t = relu(bn(conv_p1(x))) [n_boards,64,256] bf16 -> conv_p2 + bias -> (softmax) -> probs [n_boards,4672] f32 in the
 *          reference's flatten order (plane*64 + row*8 + col); w_packed from sz_nn_pack_head16(conv_p2.weight [73,256]);
 *  value : x [n_boards,64,256] bf16 -> conv_v1 (+v_norm folded: wv[256], bv) -> ReLU -> fc_v1 -> ReLU -> fc_v2 -> tanh -> [n_boards]. */
int sz_nn_policy_head_bf16(const void* t, const void* w_packed, const float* bias, float* probs, int32_t n_boards, int32_t do_softmax, void* stream);
int sz_nn_value_head_bf16(const void* x, const float* wv, float bv, const float* fc1_w_t, const float* fc1_b, const float* fc2_w, float fc2_b,
                          float* value, int32_t n_boards, void* stream);
int sz_nn_pack_head16(const float* w_in, uint16_t* out);
/* Both heads from ONE read of the tower output x (replaces sz_nn_conv_bf16(ksize 1) + the two calls above): conv_p1 -> LDS -> conv_p2 ->
 * softmax -> probs, and conv_v1 -> value MLP -> value.  w_p1_packed: conv_p1 with p_norm1 folded, sz_nn_pack_weights16(cin_padded 256,
 * ksize 1); v1_scratch: [n_boards*64] f32 device scratch (conv_v1 outputs between the two internal launches). */
int sz_nn_heads_bf16(const void* x, const void* w_p1_packed, const float* b_p1, const void* w_p2_packed, const float* b_p2, const float* wv, float bv,
                     const float* fc1_w_t, const float* fc1_b, const float* fc2_w, float fc2_b, float* probs, float* value, float* v1_scratch,
                     int32_t n_boards, int32_t do_softmax, void* stream);
/* sz_nn_tower_bf16 / sz_nn_heads_bf16 / sz_nn_forward_split with a range flag for f16 operands (SZ_NN_F16): the device word *range_flag is OR-ed with 1 when an
 * activation that the kernels stored as f16 (stem, t, block output, the policy head's t; split precision: the hi image) was 65520 or more, i.e. +inf.  The next convolution makes NaN of such a value and the
 * integer ReLU can erase that NaN again, so the outputs alone do not show it.  NULL, or bf16 operands: nothing is reported. */
int sz_nn_tower_f16_checked(const void* planes, const void* const* w_packed, const float* const* bias, int32_t n_blocks, void* out,
                            int32_t n_boards, int32_t flags, uint32_t* range_flag, void* stream);
int sz_nn_heads_f16_checked(const void* x, const void* w_p1_packed, const float* b_p1, const void* w_p2_packed, const float* b_p2, const float* wv, float bv,
                            const float* fc1_w_t, const float* fc1_b, const float* fc2_w, float fc2_b, float* probs, float* value, float* v1_scratch,
                            int32_t n_boards, int32_t do_softmax, uint32_t* range_flag, void* stream);
int sz_nn_forward_split_checked(const void* planes, const void* w_stream, const float* bias, int32_t n_blocks, const void* w_p2_packed, const float* b_p2,
                                const float* wv, float bv, const float* fc1_w_t, const float* fc1_b, const float* fc2_w, float fc2_b, float* probs, float* value,
                                float* v1_scratch, float* tower_out, int32_t n_boards, int32_t do_softmax, int32_t flags, uint32_t* range_flag, void* stream);

const char* sz_error_string(int code);
int sz_device_count(void);

/* ------------------------------------------------------------------ host mirror (no GPU) */

/* One game = the reference's ChessTensor object (chess_tensor.py:30-188), rules from the same
 * __host__ __device__ code the kernels run.  Piece codes follow python-chess: N=2 B=3 R=4 Q=5. */
typedef struct szh_game szh_game;

szh_game* szh_game_new(int chess960, int scharnagl);                 /* ChessTensor(chess960) ; :69 / :71 */
szh_game* szh_game_from_fen(const char* fen, int chess960);
szh_game* szh_game_copy(const szh_game* g);                          /* copy.deepcopy(game), mcts.py:58 */
void      szh_game_free(szh_game* g);
int  szh_legal_actions(const szh_game* g, int32_t* idx);             /* actionsToTensor(get_valid_moves()) support, ascending */
int  szh_action_to_move(const szh_game* g, int idx, int32_t* from, int32_t* to, int32_t* promo);  /* tensorToAction, :309-410 */
int  szh_move_to_action(int from, int to, int promo, int white);    /* actionToTensor, :221-306 */
int  szh_push_action(szh_game* g, int idx);                          /* move_piece, :88-129 */
int  szh_push_move(szh_game* g, int from, int to, int promo);
void szh_status(const szh_game* g, int32_t* out12);
void szh_planes(const szh_game* g, uint8_t* out /* 119*64 */);        /* get_representation, :131-142 */
uint64_t szh_perft(szh_game* g, int depth);
void szh_bitboards(const szh_game* g, uint64_t* out10);
int  szh_export(const szh_game* g, void* ring_out, int32_t* ply, int32_t* chess960);
int  szh_is_chess960(const szh_game* g);
int  szh_plane_bits_mismatches(const szh_game* g);                   /* test hook: kernels' bit-parallel mask extraction vs its definition; 0 = identical */

#ifdef __cplusplus
}
#endif
#endif
