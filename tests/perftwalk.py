"""Perft walk: make a search enumerate every child of a root, so that the rules code under test generates, applies and
classifies every move of a perft tree (tests/test_perft_walk_driver.py on the CPU oracle, tests/test_gpu_device_perft.py on the device).

The walk.  A search with the uniform evaluator (policy 1/4672 everywhere, value 0), learning off, a very large C and
num_searches = K + 1 visits each of the K root children exactly once, in ascending action-index order: unvisited children all score
q = 0.5, u = C * sqrt(N) / K; a visited child's u is halved; ties go to the lowest index.  THE LARGE C MATTERS: at the usual C = 2 a
child that is checkmate gets q = 1 after its first visit and is selected again and again (1 + u/2 beats 0.5 + u when u < 1), so the
other children are never created.  With num_searches > K + 1 (boards of one engine share num_searches) the surplus simulations go
below the children, after every child has been created; those leaves (depth 2 and deeper) are not part of the walk.

PERFT holds the public tables (name, FEN or None, chess960, [perft(1), perft(2), ...]); nothing else in tests/ repeats the numbers."""
import ctypes as C

import numpy as np

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N

PERFT = [
    ("startpos", None, False, [20, 400, 8902, 197281, 4865609]),
    ("kiwipete", "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1", False, [48, 2039, 97862, 4085603]),
    ("pos3", "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1", False, [14, 191, 2812, 43238, 674624, 11030083]),
    ("pos4", "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1", False, [6, 264, 9467, 422333, 15833292]),
    ("pos5", "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8", False, [44, 1486, 62379, 2103487]),
    ("pos6", "r4rk1/1pp1qppp/p1np1n2/2b1p1B1/2B1P1b1/P1NP1N2/1PP1QPPP/R4RK1 w - - 0 10", False, [46, 2079, 89890, 3894594]),
    ("c960", "bqnb1rkr/pp3ppp/3ppn2/2p5/5P2/P2P4/NPP1P1PP/BQ1BNRKR w HFhf - 2 9", True, [21, 528, 12189, 326672, 8146062]),
]
PERFT_BY_NAME = {p[0]: p for p in PERFT}

WALK_C = 1.0e6                 # see the module docstring: must dwarf every q
MATE_IN_ONE = "6k1/5ppp/8/8/8/8/5PPP/R5K1 w - - 0 1"
MAX_FANOUT = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"
UNIFORM_P = np.float32(1.0) / np.float32(N.SZ_ACTIONS)
RECORD_WORDS = ["pawns", "knights", "bishops", "rooks", "queens", "kings", "white", "meta", "key", "castling"]

MW = N.SZ_MASK_WORDS


def table_root(name, chess960=None):
    _, fen, c960, _ = PERFT_BY_NAME[name]
    c960 = c960 if chess960 is None else chess960
    return sz.ChessTensor(chess960=c960, fen=fen) if fen else sz.ChessTensor(chess960=c960, scharnagl=518 if c960 else None)


def positions_at_depth(root, depth, path=()):
    """every position `depth` plies below `root` in the perft sense (move generation only), as (action path, ChessTensor); depth-first in
    action order.  A generator: a caller that works in chunks never holds the whole level."""
    if depth == 0:
        yield tuple(path), root
        return
    for a in root.legal_action_indices():
        ch = root.copy()
        ch.push_action(a)
        yield from positions_at_depth(ch, depth - 1, tuple(path) + (a,))


def children_that_take_a_right(root):
    """(action, child) for the children of `root` reached by a castling (the king moves onto its own rook) or by the capture of a rook
    that carried a castling right, read off the host mirror's record"""
    rec = dict(zip(RECORD_WORDS, root.board.bitboards()))
    for a in root.legal_action_indices():
        m = root.move_from_index(a)
        f, t = 1 << m.from_square, 1 << m.to_square
        same_colour = bool(rec["white"] & f) == bool(rec["white"] & t)
        if (rec["kings"] & f and rec["rooks"] & t and same_colour) or (rec["castling"] & rec["rooks"] & t and not same_colour):
            ch = root.copy()
            ch.push_action(a)
            yield a, ch


def chunks(it, n_max, weight=lambda x: 1):
    buf, w = [], 0
    for x in it:
        wx = weight(x)
        if buf and w + wx > n_max:
            yield buf
            buf, w = [], 0
        buf.append(x)
        w += wx
    if buf:
        yield buf


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum(dtype=np.int64))


def mask_words(idx_rows, n_rows):
    """legal action lists (int32 [n,218], counts [n]) -> [n,73] uint64 masks, bit v of word p = action p*64+v"""
    out = np.zeros((len(n_rows), MW), np.uint64)
    r = np.repeat(np.arange(len(n_rows)), n_rows)
    a = idx_rows[np.arange(idx_rows.shape[1])[None, :] < np.asarray(n_rows)[:, None]].astype(np.int64)
    np.bitwise_or.at(out, (r, a >> 6), np.uint64(1) << (a & 63).astype(np.uint64))
    return out


def pack_rows(planes_u8):
    """[n,119,64] 0/1 -> [n,119] uint64, bit (row*8 + col) of a word = the cell"""
    b = np.packbits(np.ascontiguousarray(planes_u8, dtype=np.uint8).reshape(len(planes_u8), N.SZ_PLANES, 64), axis=-1, bitorder="little")
    return b.view(np.uint64).reshape(len(planes_u8), N.SZ_PLANES)


class HostLevel:
    """The host mirror's view of a list of roots and of every child of every root, as numpy arrays built in one pass.
    Row o[r] + i is child i (ascending action order) of root r."""

    def __init__(self, roots, children=True):
        L = N.lib()
        self.paths = [p for p, _ in roots]
        self.games = [g for _, g in roots]
        R = len(roots)
        idx = np.zeros((R, N.SZ_MAX_MOVES), np.int32)
        idx_c = (C.c_int32 * N.SZ_MAX_MOVES * R).from_buffer(idx)
        self.K = np.array([L.szh_legal_actions(g._g, idx_c[r]) for r, g in enumerate(self.games)], np.int64)
        self.actions = idx
        self.status = np.array([g.board._st() for g in self.games], np.int32).reshape(R, 12)
        self.K_live = np.where(self.status[:, 4] != 0, 0, self.K)          # a terminal root (mate, stalemate, rule draw) is never expanded
        self.mask = mask_words(idx, self.K)
        planes = np.zeros((R, N.SZ_PLANES, 64), np.uint8)
        for r, g in enumerate(self.games):
            L.szh_planes(g._g, planes.ctypes.data + r * planes.strides[0])
        self.planes = pack_rows(planes)
        self.o = np.concatenate([[0], np.cumsum(self.K_live)]).astype(np.int64)
        if not children:
            return
        n = int(self.o[-1])
        self.c_root = np.repeat(np.arange(R), self.K_live)
        self.c_index = np.arange(n) - self.o[self.c_root]
        self.c_action = idx[self.c_root, self.c_index] if n else np.zeros(0, np.int32)
        c_idx = np.zeros((max(n, 1), N.SZ_MAX_MOVES), np.int32)
        c_idx_c = (C.c_int32 * N.SZ_MAX_MOVES * max(n, 1)).from_buffer(c_idx)
        c_st = np.zeros((max(n, 1), 12), np.int32)
        c_st_c = (C.c_int32 * 12 * max(n, 1)).from_buffer(c_st)
        c_rec = np.zeros((max(n, 1), 10), np.uint64)
        c_rec_c = (C.c_uint64 * 10 * max(n, 1)).from_buffer(c_rec)
        c_nl = np.zeros(max(n, 1), np.int64)
        c_pl = np.zeros((max(n, 1), N.SZ_PLANES, 64), np.uint8)
        base, stride = c_pl.ctypes.data, c_pl.strides[0]
        copy, push, free, legal, status, planes_f, bitboards = (L.szh_game_copy, L.szh_push_action, L.szh_game_free, L.szh_legal_actions,
                                                                L.szh_status, L.szh_planes, L.szh_bitboards)
        k = 0
        for r, g in enumerate(self.games):
            for i in range(int(self.K_live[r])):
                c = copy(g._g)
                if push(c, int(idx[r, i])) != N.SZ_OK:
                    raise AssertionError("host mirror refuses its own legal move")
                c_nl[k] = legal(c, c_idx_c[k])
                status(c, c_st_c[k])
                bitboards(c, c_rec_c[k])
                planes_f(c, base + k * stride)
                free(c)
                k += 1
        self.c_status, self.c_record = c_st[:n], c_rec[:n]
        self.c_term = c_st[:n, 4] != 0                          # get_value_and_terminated()[1]
        self.c_loss = c_st[:n, 5] != 0                          # ... and the value is -1 (the side to move is mated)
        self.c_nlegal = c_nl[:n]
        self.c_mask = mask_words(c_idx[:n], c_nl[:n])
        self.c_planes = pack_rows(c_pl[:n])

    def name(self, r, i=None):
        s = "root path %s" % (list(self.paths[r]),)
        return s if i is None else s + ", child action %d" % int(self.actions[r, i])


def first_difference(got_mask, want_mask, got_planes, want_planes):
    """index of the first row that differs and a description of the first differing mask word / plane, or None"""
    bad_m, bad_p = (got_mask != want_mask).any(1), (got_planes != want_planes).any(1)
    bad = np.nonzero(bad_m | bad_p)[0]
    if not len(bad):
        return None
    j = int(bad[0])
    if bad_m[j]:
        w = int(np.nonzero(got_mask[j] != want_mask[j])[0][0])
        return j, "legal-mask word %d: got %#018x, want %#018x" % (w, int(got_mask[j, w]), int(want_mask[j, w]))
    p = int(np.nonzero(got_planes[j] != want_planes[j])[0][0])
    return j, "plane %d: got %#018x, want %#018x" % (p, int(got_planes[j, p]), int(want_planes[j, p]))


# ------------------------------------------------------------------------------------------------ the walk on the CPU oracle
def oracle_walk(oct_, c=WALK_C, extra=0):
    """The walk on oracle.Search: returns (K, visits per root child, root-child indices in the order in which they became pending leaves
    (terminal children never do), sum of those leaves' legal-move counts, legal-move count of the root)."""
    from oracle import oracle as O
    K = len(oct_.legal_action_indices()[0])
    s = O.Search.on_chess(oct_, c=float(c), num_searches=K + 1 + extra, learning=False)
    policy = np.full(N.SZ_ACTIONS, UNIFORM_P, np.float32)
    order, leaf_total, root_legal, deeper = [], 0, None, False
    while s.advance():
        tr = s.trace()
        if len(tr) == 0:
            root_legal = len(s.leaf_actions())
        elif len(tr) == 1:
            assert not deeper, "a root child was created after a simulation had gone below the children"
            order.append(tr[0])
            leaf_total += len(s.leaf_actions())
        else:
            deeper = True
        s.feed(policy, 0.0)
    _, vis, _ = s.root_children()
    return K, vis, order, leaf_total, root_legal


# ------------------------------------------------------------------------------------------------ the walk on the device
def _gpu_pack(planes):
    """engine planes [B,119,8,8] f32 on the device -> [B,119] int64 bit patterns on the device, same bit order as pack_rows"""
    import torch
    B = planes.shape[0]
    w = (torch.ones(1, dtype=torch.int64, device=planes.device) << torch.arange(64, device=planes.device, dtype=torch.int64))
    return ((planes.reshape(B, N.SZ_PLANES, 64) != 0).to(torch.int64) * w).sum(-1)


class WalkResult:
    def __init__(self):
        self.roots = self.root_moves = self.children = self.child_moves = self.terminal_children = 0

    def add(self, o):
        for k in self.__dict__:
            setattr(self, k, getattr(self, k) + getattr(o, k))


def device_walk(tag, roots, chess960, compare=True, scharnagl=None):
    """Upload `roots` ((path, ChessTensor) pairs, ring included) to one engine and run the walk.  Counts come from the DEVICE's masks and
    tree only; with `compare` every root and every device-created child is held to the host mirror (legal mask, 119 planes, terminal or not,
    loss or draw), exact equality.  Asserts per board that exactly its K children were seen, each once: pending at depth 1, or terminal.
    With `scharnagl` (one start-position number per root) nothing is uploaded: the device creates the roots itself (new_games), and
    `roots` are the host mirror's games for the same numbers."""
    import torch
    from sigma_zero_amd.selfplay import SelfPlayEngine
    H = HostLevel(roots, children=compare)
    B, K = len(roots), H.K_live
    S = int(K.max()) + 1
    eng = SelfPlayEngine(None, {"C": WALK_C, "num_searches": S}, B, chess960=chess960, learning=False)
    try:
        if scharnagl is not None:
            assert len(scharnagl) == B
            eng.new_games(scharnagl)
        else:
            for b, g in enumerate(H.games):
                eng.upload_game(b, g)
        policy = torch.full((B, N.SZ_ACTIONS), float(UNIFORM_P), dtype=torch.float32, device=eng.device)
        value = torch.zeros(B, dtype=torch.float32, device=eng.device)
        res = WalkResult()
        res.roots = B
        seen = np.zeros((B, N.SZ_MAX_MOVES), np.int32)
        last_child = np.full(B, -1, np.int64)
        eng.begin()
        for step in range(S + 2):
            torch.cuda.synchronize()
            mask, depth, n_nodes, _, status = eng.debug_pending()
            pend = (status & 2) != 0
            if not pend.any():
                break
            assert step <= S, "%s: boards still pending after num_searches steps" % tag
            ci = None
            if step == 0:
                assert (depth[pend] == 0).all() and (pend == (H.status[:, 4] == 0)).all(), "%s: the pending roots are not the non-terminal roots" % tag
                sel = np.nonzero(pend)[0]
                res.root_moves += popcount(mask[sel])
                want_rows, want_mask, want_planes = sel, H.mask, H.planes
            else:
                sel = np.nonzero(pend & (depth == 1))[0]                # deeper leaves: surplus simulations of boards with K + 1 < num_searches
                ci = n_nodes[sel].astype(np.int64) - 2                 # nodes are created in visiting order: root, child 0, child 1, ...
                assert ((ci >= 0) & (ci < K[sel]) & (ci > last_child[sel])).all(), "%s: children were not created one by one in index order" % tag
                last_child[sel] = ci
                seen[sel, ci] += 1
                res.child_moves += popcount(mask[sel])
                if compare:
                    want_rows, want_mask, want_planes = H.o[sel] + ci, H.c_mask, H.c_planes
            if compare and len(sel):
                got_planes = _gpu_pack(eng.planes)[torch.as_tensor(sel, device=eng.device)].cpu().numpy().view(np.uint64)
                d = first_difference(mask[sel], want_mask[want_rows], got_planes, want_planes[want_rows])
                if d is not None:
                    b = int(sel[d[0]])
                    raise AssertionError("%s: %s: device differs from the host mirror at %s"
                                         % (tag, H.name(b, None if ci is None else int(ci[d[0]])), d[1]))
            eng.step(policy, value)
        eng.check_errors()
        action, visits, n_child, _, wsum = eng.root_children()
        col = np.arange(N.SZ_MAX_MOVES)[None, :]
        live = col < K[:, None]
        assert (n_child == K).all(), "%s: root child counts differ from the host's legal-move counts" % tag
        assert (action[live] == H.actions[live]).all(), "%s: root children are not the host's legal moves in index order" % tag
        assert (visits[live] >= 1).all() and (visits[~live] == 0).all(), "%s: a root child was never visited" % tag
        exact = K == S - 1                                              # boards whose K + 1 is the engine's num_searches: one visit per child
        assert (visits[exact][live[exact]] == 1).all(), "%s: a board with K + 1 simulations did not visit every child exactly once" % tag
        assert (seen <= 1).all(), "%s: a child was pending twice" % tag
        term = live & (seen == 0)                                       # never handed to the evaluator: backed up inside the launch = terminal
        dev_loss = term & (wsum == -visits.astype(np.float64)) & (visits > 0)
        assert (wsum[term & ~dev_loss] == 0.0).all(), "%s: a terminal child's value sum is neither -visits (mate) nor 0 (draw)" % tag
        res.children = int(K.sum())
        res.terminal_children = int(term.sum())
        assert int(seen.sum()) + res.terminal_children == res.children
        # a terminal child has visits but no descendants; a child that was pending was expanded: it has descendants
        for b in np.nonzero(term.any(1))[0]:
            d, a, v, w, _ = eng.debug_tree(int(b))
            rows = np.nonzero(d == 0)[0]
            assert len(rows) == K[b] and (a[rows] == H.actions[b, :K[b]]).all()
            has_desc = np.array([r + 1 < len(d) and d[r + 1] == 1 for r in rows])
            assert (has_desc == ~term[b, :K[b]]).all(), "%s: %s: terminal children and children without descendants differ" % (tag, H.name(int(b)))
        if compare:
            h_term = np.zeros_like(term)
            h_loss = np.zeros_like(term)
            h_term[H.c_root, H.c_index] = H.c_term
            h_loss[H.c_root, H.c_index] = H.c_loss
            for what, dev, host in (("terminal", term, h_term), ("checkmate", dev_loss, h_loss)):
                bad = np.argwhere(dev != host)
                assert not len(bad), "%s: %s: device says %s = %s, the host mirror says %s" % (
                    tag, H.name(int(bad[0][0]), int(bad[0][1])), what, bool(dev[tuple(bad[0])]), bool(host[tuple(bad[0])]))
        return res
    finally:
        eng.close()


def sample_uniforms(visits, n_child, child):
    """the uniform from the middle of child i's interval of the cdf that np.random.choice (and sz_play) builds from the visit counts"""
    u = np.zeros(len(child), np.float64)
    for b in range(len(child)):
        v = visits[b, :n_child[b]].astype(np.float64)
        cdf = np.cumsum(v / v.sum())
        cdf /= cdf[-1]
        i = int(child[b])
        u[b] = 0.5 * ((cdf[i - 1] if i else 0.0) + cdf[i])
    return u


def device_play(tag, roots, chess960):
    """k_play applies every legal move: root r sits on K_r boards, the walk runs on each, and the i-th copy plays child i.  The position
    record the device then holds (bitboards, meta, key: its own sz_finish_meta, hash key, repetition count, check flag) equals the host
    mirror's record after the same move byte for byte (no field is masked: both sides derive every bit from the same parent record), and
    sz_fetch_ply's chosen / game_over / result equal the host's.  Returns the number of boards played."""
    import torch
    from sigma_zero_amd.selfplay import SelfPlayEngine
    H = HostLevel(roots, children=True)
    n = int(H.o[-1])
    if n == 0:
        return 0
    S = int(H.K_live.max()) + 1
    eng = SelfPlayEngine(None, {"C": WALK_C, "num_searches": S}, n, chess960=chess960, learning=False)
    try:
        for b in range(n):
            eng.upload_game(b, H.games[int(H.c_root[b])])
        policy = torch.full((n, N.SZ_ACTIONS), float(UNIFORM_P), dtype=torch.float32, device=eng.device)
        value = torch.zeros(n, dtype=torch.float32, device=eng.device)
        eng.begin()
        for _ in range(S):
            eng.step(policy, value)
        st = eng.check_errors()
        assert st["boards_done"] == n and st["boards_pending"] == 0, "%s: searches did not finish" % tag
        action, visits, n_child, _, _ = eng.root_children()
        assert (n_child == H.K_live[H.c_root]).all() and (visits[np.arange(n), H.c_index] >= 1).all(), tag
        eng.play(sample_uniforms(visits, n_child, H.c_index))
        rec = eng.fetch_ply()
        eng.check_errors()
        assert rec["active"].all(), tag
        where = lambda b: "%s: %s" % (tag, H.name(int(H.c_root[b]), int(H.c_index[b])))
        bad = np.nonzero(rec["chosen"] != H.c_action)[0]
        assert not len(bad), "%s: sz_play chose action %d" % (where(bad[0]), rec["chosen"][bad[0]])
        want_result = np.where(H.c_loss, np.where(H.c_status[:, 0] != 0, -1, 1), 0)      # the side to move is mated
        for b in range(n):
            pos, ply = eng.debug_position(b)
            if not np.array_equal(pos, H.c_record[b]):
                w = int(np.nonzero(pos != H.c_record[b])[0][0])
                raise AssertionError("%s: position record after k_play differs from the host mirror's in %s: got %#018x, want %#018x"
                                     % (where(b), RECORD_WORDS[w], int(pos[w]), int(H.c_record[b, w])))
            assert ply == H.c_status[b, 1], "%s: game ply %d" % (where(b), ply)
            assert bool(rec["game_over"][b]) == bool(H.c_term[b]), "%s: game_over %d" % (where(b), rec["game_over"][b])
            assert int(rec["result"][b]) == int(want_result[b]), "%s: result %d" % (where(b), rec["result"][b])
        return n
    finally:
        eng.close()
