"""Repetition, the 75-move rule and draws by material on positions the DEVICE creates deep in the tree, and the longest descent a search
can make.

tests/perftwalk.py holds device-created nodes to the host mirror at tree depth 1 only.  wave_count_reps, ancestor_ptr and
wave_load_history switch between tree nodes (npos[path[D-j]]) and the game ring (ring[(root_ply+D-j) & 255]) at j == D, and nothing placed
a repetition cycle, a 75-move expiry, a ring wrap or a draw by material at a chosen depth and at every offset across that boundary.  Nor
did anything run a tree that is one chain num_searches long (p_cap = n_cap in sz_create, `d >= v.p_cap` in k_search_step).

The scripted descent.  Every line of tests/ending_lines.py sits on one board: its history goes in through upload_game (the ring), its
continuation is walked inside the tree.  The policy fed for a board is one-hot on the line's next action, so the renormalised prior of
that move is exactly 1.0 and every other move has prior 0 and is dropped at expansion (policy.nonzero()): the tree is a chain, and
simulation k expands depth k.  The value fed at depth k is (k + 1) / 64, so every value sum is exact in binary.  At every step and board
  * debug_pending's depth equals the scripted depth, and n_nodes what the chain restatement below gives;
  * the legal mask equals the host mirror's at that depth, all 73 words;
  * eng.planes equals the host mirror's get_representation(), all 119 planes: eight history steps that straddle the root at depths 1..7,
    and the repetition planes of every step;
  * planes 12 and 13 of the newest step also equal the plain statement's is_repetition(2) and is_repetition(3) directly.
Where the plain statement (tests/plainendings.py) says the line's position at depth d is over, the board expands nothing further: n_nodes
stops at d + 1, the engine's terminal_hits grows by one per remaining simulation in that very step, and debug_tree's visit counts and
value sums along the chain equal chain_backup() below (alternating signs, 0 for a draw, -1 for the mated side to move): a draw is told
from "not over, value 0", and a mate at clock 150 from a draw.  Where it says not over, the chain keeps growing (the cycle one ply short
of fivefold, clock 149, K+N+N v K, opposite bishops, =Q, =R).
Full-length chains: lines of num_searches quiet plies for S = 8 and S = 40 end with no error flag, num_searches nodes (simulation k expands
depth k, the root's own expansion being simulation 0 as in mcts.py:49; depths 0 .. S - 1), and the deepest leaf's planes are the host mirror's.

The references are the host mirror (masks, planes) and the plain statement (what is over, the repetition flags, the chain); the oracle is
not used here.  test_plain_endings.py holds the host mirror to the plain statement on the same lines, ply by ply, on the CPU.
No tolerance anywhere.  Three engines: standard S = 40 (77 boards, 1,008 positions compared inside the tree, 73 endings met there, filler
included), Chess960 S = 40 (3 boards, 96 positions), standard S = 8 (47 boards, 246 positions).  On MI355X the module takes 1.3 s.
Teeth: a wrong clock threshold or an identity without castling rights, put into a copy of the plain statement, fails the comparison inside
the tree (last test); test_plain_endings.py shows the same for five clauses on the CPU.
Teeth on the device side (shown once with scratch libraries whose DEVICE code alone was changed, not committed): with ancestor_ptr reading
the ring one ply too old below depth 1, this module fails by name ("cycle:fivefold_at_depth_03 at depth 2: device differs from the host
mirror at plane 43") while test_rule_endings_on_the_device, which stops at depth 1, passes; with wave_count_reps making no second pass over
its lanes below depth 1, 543 of the 550 tests of the GPU suite pass, this module fails by name ("snake:root_80_plies_in at depth 4: ...
plane 12: got 0, want all ones") and the only other test to notice is test_gpu_subtree_reuse.py, whose search happens to walk into the
84-ply window at its step 33.
"""
import numpy as np
import pytest

import ending_lines as L
import perftwalk as W
import plainendings as E

ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_RAN = {}                          # (chess960, S) -> {"kinds": ..., "deepest": ...}, read by the coverage test


def value_at(depth):
    return (depth + 1) / 64.0


def chain_backup(S, over_depth, terminal_value):
    """The search of a tree that is one chain, restated: simulation k = 0 .. S-1 walks to the first node without children.  That is
    depth k, which is expanded and evaluated to value_at(k), unless the position at over_depth is over: it is created by simulation
    over_depth, never expanded, and every later simulation ends on it with terminal_value.  A value v found at depth leaf is added to
    depth j as v * (-1)^(leaf - j); the root starts with one visit (mcts.py:46).
    Returns (visits, value sums) per depth 0 .. the deepest edge, the number of created nodes, and the simulations that ended on a
    terminal node."""
    deepest = S if over_depth is None or over_depth > S else over_depth                # the last expansion leaves one unvisited child
    visits, sums = [0] * (deepest + 1), [0.0] * (deepest + 1)
    visits[0] = 1
    nodes = hits = 0
    for k in range(S):
        if over_depth is not None and k >= over_depth:
            leaf, v = over_depth, float(terminal_value)
            hits += 1
            nodes += k == over_depth
        else:
            leaf, v = k, value_at(k)
            nodes += 1
        for j in range(leaf + 1):
            visits[j] += 1
            sums[j] += v if (leaf - j) % 2 == 0 else -v
    return np.array(visits, np.int32), np.array(sums, np.float64), nodes, hits


def test_chain_backup_by_hand():
    v, w, nodes, hits = chain_backup(3, None, 0)
    assert v.tolist() == [4, 2, 1, 0] and nodes == 3 and hits == 0
    assert w.tolist() == [1 / 64 - 2 / 64 + 3 / 64, 2 / 64 - 3 / 64, 3 / 64, 0.0]
    v, w, nodes, hits = chain_backup(5, 2, -1)                          # the position at depth 2 is mate: three simulations end there
    assert v.tolist() == [6, 4, 3] and nodes == 3 and hits == 3
    assert w.tolist() == [1 / 64 - 2 / 64 - 3.0, 2 / 64 + 3.0, -3.0]
    assert chain_backup(4, 4, 0)[2:] == (4, 0) and len(chain_backup(4, 4, 0)[0]) == 5   # an ending one ply past the last expansion is never seen


class HostLine:
    """the host mirror along a built line: per depth the legal mask, the packed planes and the action that leads on"""

    def __init__(self, built, S):
        self.built = built
        ct = L.host_game(built.fen, built.chess960)
        g = built.game
        for ply in range(built.root):
            ct.push_action(L.host_actions(ct)[L.host_spelling(g.pos[ply], g.moves[ply], built.chess960)])
        self.root = ct.copy()
        self.last = min(built.depths, S) if built.over_depth is not None else S - 1     # the deepest position the search creates
        games, self.action = [], []
        for d in range(self.last + 1):
            games.append(ct.copy())
            if d < built.depths:
                a = L.host_actions(ct)[L.host_spelling(g.pos[built.root + d], built.move(d), built.chess960)]
                self.action.append(a)
                ct.push_action(a)
        H = W.HostLevel([((), c) for c in games], children=False)
        self.mask, self.planes, self.status = H.mask, H.planes, H.status


def run_lines(lines, S, chess960, rules=E.RULES):
    import torch
    from sigma_zero_amd import _native as N
    from sigma_zero_amd.selfplay import SelfPlayEngine
    built = [L.build(line, S, rules, claims=rules is E.RULES) for line in lines]
    assert all(b.chess960 == chess960 for b in built) and len(built) <= 96
    B = len(built)
    host = [HostLine(b, S) for b in built]
    over = [b.over_depth if b.over_depth is not None and b.over_depth < S else None for b in built]   # what the search can see
    want = []
    for b, o in zip(built, over):
        tv = 0 if o is None else b.at(o)[2][1]
        want.append(chain_backup(S, o, tv))
    final_nodes = np.array([w[2] for w in want])
    last_pending = np.array([S - 1 if o is None else o - 1 for o in over])               # the deepest depth handed to the evaluator
    eng = SelfPlayEngine(None, {"C": 2, "num_searches": S}, B, learning=False, chess960=chess960)
    deepest = 0
    try:
        for i, h in enumerate(host):
            eng.upload_game(i, h.root)
        policy = np.zeros((B, N.SZ_ACTIONS), np.float32)
        eng.begin()
        for step in range(S + 1):
            torch.cuda.synchronize()
            mask, depth, n_nodes, _, status = eng.debug_pending()
            pend = (status & 2) != 0
            tag = "S = %d, step %d" % (S, step)
            bad = np.nonzero(pend != (step <= last_pending))[0]
            assert not len(bad), "%s: %s: pending %s, but the plain statement says the game is over at depth %s" % (
                tag, built[bad[0]].name, bool(pend[bad[0]]), over[bad[0]])
            bad = np.nonzero(n_nodes != np.minimum(step + 1, final_nodes))[0]
            assert not len(bad), "%s: %s: %d nodes, the chain has %d" % (tag, built[bad[0]].name, n_nodes[bad[0]], min(step + 1, final_nodes[bad[0]]))
            st = eng.stats()
            hits = sum(w[3] for w, o in zip(want, over) if o is not None and o <= step)
            assert st["terminal_hits"] == hits and st["boards_error"] == 0, "%s: terminal_hits %d, the chains have %d" % (tag, st["terminal_hits"], hits)
            if not pend.any():
                break
            sel = np.nonzero(pend)[0]
            assert (depth[sel] == step).all(), "%s: pending depth %s" % (tag, depth[sel].tolist())
            got_planes = W._gpu_pack(eng.planes)[torch.as_tensor(sel, device=eng.device)].cpu().numpy().view(np.uint64)
            want_mask = np.stack([host[i].mask[step] for i in sel])
            want_planes = np.stack([host[i].planes[step] for i in sel])
            d = W.first_difference(mask[sel], want_mask, got_planes, want_planes)
            assert d is None, "%s: %s at depth %d: device differs from the host mirror at %s" % (tag, built[sel[d[0]]].name, step, d[1])
            policy[:] = 0.0
            for k, i in enumerate(sel):
                _, _, outcome, rep2, rep3, _ = built[i].at(step)
                assert outcome is None and host[i].status[step, 4] == 0
                flags = (got_planes[k, 12] == ALL_ONES, got_planes[k, 13] == ALL_ONES)
                assert flags == (rep2, rep3) and got_planes[k, 12] in (0, ALL_ONES) and got_planes[k, 13] in (0, ALL_ONES), \
                    "%s: %s at depth %d: repetition planes %s, the plain statement says %s" % (tag, built[i].name, step, flags, (rep2, rep3))
                policy[i, host[i].action[step]] = 1.0
            deepest = max(deepest, step)
            value = torch.full((B,), value_at(step), dtype=torch.float32, device=eng.device)
            eng.step(torch.from_numpy(policy).to(eng.device), value)
        st = eng.check_errors()
        assert st["boards_error"] == 0 and st["boards_done"] == B and st["boards_pending"] == 0
        assert st["expansions"] + st["terminal_hits"] == B * S == st["simulations"]
        for i, (b, (visits, sums, nodes, _)) in enumerate(zip(built, want)):
            d, a, v, w, pr = eng.debug_tree(i)
            n = len(visits)
            assert d.tolist() == list(range(-1, n - 1)), "%s: the tree is no chain of %d edges: depths %s" % (b.name, n, d.tolist())
            assert a[1:].tolist() == host[i].action[:n - 1], "%s: actions along the chain" % b.name
            assert v.tolist() == visits.tolist(), "%s: visits %s, the chain restatement %s" % (b.name, v.tolist(), visits.tolist())
            assert w.tolist() == sums.tolist(), "%s: value sums %s, the chain restatement %s" % (b.name, w.tolist(), sums.tolist())
            assert (pr[1:] == 1.0).all()
            if over[i] is not None:                                     # the terminal node: host mirror and plain statement, then the device through the chain
                o = b.at(over[i])[2]
                assert host[i].status[over[i], 4] != 0 and (host[i].status[over[i], 5] != 0) == (o[0] == E.MATE)
    finally:
        eng.close()
    print("S = %d, chess960 = %s: %d boards, %d positions compared with the host mirror, %d endings inside the tree" % (
        S, chess960, B, int((last_pending + 1).sum()), sum(o is not None for o in over)))
    if rules is not E.RULES:
        return built, over, final_nodes
    _RAN[(chess960, S)] = {"kinds": {b.kind for b in built}, "deepest": deepest,
                           "over_kinds": {b.at(o)[2][0] for b, o in zip(built, over) if o is not None and o >= b.scripted and b.line[5]["over"]},
                           "deepest_ending": max([o for b, o in zip(built, over) if o is not None and b.line[5]["over"]] or [0])}
    return built, over, final_nodes


STANDARD = [l for l in L.LINES if not l[2]]
CHESS960 = [l for l in L.LINES if l[2]]


@pytest.mark.gpu
def test_lines_at_depth_standard():
    built, over, nodes = run_lines(STANDARD, 40, False)
    by_name = {b.name: (o, n) for b, o, n in zip(built, over, nodes)}
    assert by_name["chain:40_quiet_plies"] == (None, 40)                # no ending; one node per depth 0 .. 39
    assert by_name["cycle:fivefold_at_depth_16"] == (16, 17) and by_name["wrap:root_at_ply_247"] == (17, 18)
    assert by_name["mate150:depth_5"] == (5, 6) and by_name["clock:draw_at_depth_12"] == (12, 13)


@pytest.mark.gpu
def test_lines_at_depth_chess960():
    built, over, _ = run_lines(CHESS960, 40, True)
    assert {b.name: o for b, o in zip(built, over)}["identity960:knight_cycle_on_start_617"] == 16


@pytest.mark.gpu
def test_full_length_chain_of_8():
    """num_searches = 8: the 8-ply chain, and every standard line whose continuation fits, once more with the shorter budget (an ending
    at depth 8 exactly lies one ply past the last expansion and must go unseen)"""
    built, over, nodes = run_lines([l for l in STANDARD if len(l[4]) <= 8], 8, False)
    by_name = {b.name: (o, n) for b, o, n in zip(built, over, nodes)}
    assert by_name["chain:8_quiet_plies"] == (None, 8)
    assert by_name["clock:draw_at_depth_08"] == (None, 8) and by_name["clock:draw_at_depth_07"] == (7, 8)


@pytest.mark.gpu
def test_every_kind_of_line_ran_and_deep_enough():
    for key, test in (((False, 40), test_lines_at_depth_standard), ((True, 40), test_lines_at_depth_chess960), ((False, 8), test_full_length_chain_of_8)):
        if key not in _RAN:
            test()
    kinds = set().union(*(r["kinds"] for r in _RAN.values()))
    assert kinds == set(L.KINDS), "kinds that did not run: %s" % sorted(set(L.KINDS) - kinds)
    assert set().union(*(r["over_kinds"] for r in _RAN.values())) == {E.MATE, E.MATERIAL, E.CLOCK, E.FIVEFOLD}
    assert max(r["deepest"] for r in _RAN.values()) == 39 and max(r["deepest_ending"] for r in _RAN.values()) >= 16


class _Clock149(E.Rules):
    CLOCK_LIMIT = 149


class _IgnoresRights(E.Rules):
    def identity(self, pos, legal):
        return (tuple(pos.board), pos.white, pos.ep if self.legal_en_passant(pos, legal) else None)


@pytest.mark.gpu
@pytest.mark.parametrize("rules,kind,what", [(_Clock149, "clock", "pending"), (_IgnoresRights, "identity", "repetition planes")])
def test_a_wrong_clause_in_a_copy_of_the_plain_statement_is_noticed_on_the_device(rules, kind, what):
    """teeth, by symmetric injection as in test_plain_endings.py: the device is untouched, the wrong clause sits in a copy of the plain
    statement, and the comparison inside the tree fails"""
    with pytest.raises(AssertionError, match=what):
        run_lines([l for l in STANDARD if L.kind_of(l) == kind], 16, False, rules())
