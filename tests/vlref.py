"""Plain-Python restatement of the engine's leaf-batched search (sz_set_leaf_batching, a NON-REFERENCE option; include/sigmazero.h):
up to L leaves per board per network call, steered apart by a virtual loss lam per descent in flight.  It is what the HIP kernel
(csrc/sz_engine.hip search_step<true>) is held to, bit for bit:

  * every edge carries an in-flight count k, kept apart from W / N; selection scores a child with vc = N + k and wsum = W + lam*k
    (f64), under the parent term sqrt(N_parent + k_parent), then the reference's fp32 UCB (mctsnode.py:33-37) and first-maximum argmax;
  * one step = expand and back up every pending leaf in gather order (k taken back along its path), then descend until L leaves are
    pending or sims_done + pending == S: a terminal leaf is backed up on the spot, a new non-terminal leaf becomes pending (k + 1 along
    its path, its network input at row i), a descent that ends on a leaf already pending in this step (a collision) ends the gather.

At L = 1 this is the reference's MCTS0.search (mcts.py:39-122); tests/test_leaf_batching_ref.py pins that against the reference's own
traces.  Positions come from the product's host rules (ChessTensor over csrc/sz_chess.h), the network is hashmodel.evaluate_packed."""
import math

import numpy as np

from hashmodel import evaluate_packed, pack_planes

F32 = np.float32
NOISE_REFERENCE = float(np.float32(1.0) - np.float32(2.0 ** -24))     # the engine's default noise_value (selfplay.NOISE_REFERENCE)


def ucb(vc, wsum, prior, sqrt_parent, c):
    """Node.get_ucb in torch's float32 operation order (csrc/sz_engine.hip ucb_value), over arrays of children"""
    vsum = wsum.astype(np.float32)
    t1 = vc.astype(np.float32) + F32(1e-6)
    q = F32(1.0) - ((vsum / t1) + F32(1.0)) / F32(2.0)
    r = F32(1.0) / (vc + 1).astype(np.float32)
    u = ((r * sqrt_parent) * c) * prior
    return q + u


def masked_sum(pol, acts):
    """the engine's fixed-order sum of the legal policy entries: per lane (action % 64) over planes ascending, then an xor butterfly"""
    lanes = np.zeros(64, np.float32)
    for a in acts:                                       # ascending action index = planes ascending within each lane
        lanes[a % 64] = lanes[a % 64] + pol[a]
    off = 32
    while off >= 1:
        lanes = lanes + lanes[np.arange(64) ^ off]
        off >>= 1
    return lanes[0]


class Search:
    """One board's search.  Edges are numbered like the engine's store (edge 0 = the root); run() plays the whole search."""

    def __init__(self, game, S, c=2.0, learning=False, noise=NOISE_REFERENCE, L=1, lam=1.0, mode="dyadic", salt=0):
        self.S, self.c, self.learning, self.noise, self.L, self.lam = int(S), F32(c), bool(learning), F32(noise), int(L), float(np.float32(lam))
        self.mode, self.salt = mode, int(salt)
        cap = max(self.S, 1) * 218 + 2
        self.W = np.zeros(cap, np.float64)
        self.N = np.zeros(cap, np.int64)
        self.P = np.zeros(cap, np.float32)
        self.K = np.zeros(cap, np.int64)
        self.first = np.full(cap, -1, np.int64)
        self.n = np.zeros(cap, np.int64)
        self.action = np.zeros(cap, np.int64)
        self.term = np.zeros(cap, np.int8)
        self.tval = np.zeros(cap, np.int8)
        self.games = {0: game.copy()}
        self.n_edges = 1
        self.N[0] = 1                                    # root.visit_count = 1 (mcts.py:46)
        self.steps = []                                  # per network call: packed planes [n_pend,119,8] of rows 0..n_pend-1
        self.collisions = 0
        self.gather_terminals = 0                        # terminal leaves backed up while a gather had leaves pending
        self.sims = 0

    # -- tree operations (mcts.py:77-109, mctsnode.py:23-63)
    def _expand(self, e, pol):
        acts = np.asarray(self.games[e].legal_action_indices(), np.int64)
        total = masked_sum(pol, acts)
        p = pol[acts] / total if len(acts) else np.zeros(0, np.float32)
        keep = ~(p == F32(0.0))                          # policy.nonzero(): NaN stays
        acts, p = acts[keep], p[keep].astype(np.float32)
        if self.learning:
            p = (F32(0.75) * p) + (F32(0.25) * self.noise)
        f, k = self.n_edges, len(acts)
        self.P[f:f + k], self.action[f:f + k] = p, acts
        self.first[e], self.n[e] = f, k
        self.n_edges += k

    def _backprop(self, path, v):
        d = len(path) - 1
        for j, e in enumerate(path):
            self.W[e] += v if (d - j) % 2 == 0 else -v
            self.N[e] += 1
        self.sims += 1

    def _descend(self):
        path, e = [0], 0
        lam = np.float64(self.lam)
        while self.n[e] > 0:
            f, k = self.first[e], self.n[e]
            kk = self.K[f:f + k]
            sq = F32(math.sqrt(float(self.N[e] + self.K[e])))
            u = ucb(self.N[f:f + k] + kk, self.W[f:f + k] + lam * kk.astype(np.float64), self.P[f:f + k], sq, self.c)
            e = f + int(np.argmax(u))
            path.append(e)
        return path

    def _planes(self, e):
        return pack_planes(self.games[e].get_representation().numpy())

    def run(self):
        root = self.games[0]
        tv, term = root.get_value_and_terminated()
        if term or self.S <= 0:                          # a terminal root: every simulation re-visits it (mcts.py:104-109)
            S = max(self.S, 0)
            self.W[0], self.N[0], self.sims = float(tv) * S, 1 + S, S
            return self
        pending = [([0], self._planes(0))]
        self.K[0] = 1
        self.steps.append(np.stack([p for _, p in pending]))
        while pending:
            for path, planes in pending:                 # the network call of this step, then expand + back up in gather order
                pol, val = evaluate_packed(planes, self.mode, self.salt)
                self._expand(path[-1], pol)
                self.K[path] -= 1
                self._backprop(path, float(val))
            pending = []
            while self.sims + len(pending) < self.S and len(pending) < self.L:
                path = self._descend()
                e = path[-1]
                if e in self.games:
                    if not self.term[e] and self.first[e] < 0:      # pending in this step: a collision ends the gather
                        self.collisions += 1
                        break
                    self._backprop(path, float(self.tval[e]))       # visited leaf without children
                    self.gather_terminals += 1 if pending else 0
                    continue
                g = self.games[path[-2]].copy()
                g.push_action(int(self.action[e]))
                self.games[e] = g
                v, t = g.get_value_and_terminated()
                self.term[e], self.tval[e] = int(t), int(v) if t else 0
                if t:
                    self._backprop(path, float(v))
                    self.gather_terminals += 1 if pending else 0
                    continue
                self.K[path] += 1
                pending.append((path, self._planes(e)))
            if pending:
                self.steps.append(np.stack([p for _, p in pending]))
        return self

    # -- readouts
    def tree(self):
        """(depth, action, visits, value_sum, prior) depth-first in child order, row 0 = the root (sz_debug_tree's layout)"""
        rows = [(-1, -1, int(self.N[0]), float(self.W[0]), float(self.P[0]))]
        stack = [(self.first[0] + k, 0) for k in range(int(self.n[0]) - 1, -1, -1)] if self.first[0] >= 0 else []
        while stack:
            e, d = stack.pop()
            rows.append((d, int(self.action[e]), int(self.N[e]), float(self.W[e]), float(self.P[e])))
            if self.first[e] >= 0:
                stack += [(self.first[e] + k, d + 1) for k in range(int(self.n[e]) - 1, -1, -1)]
        d, a, v, w, p = zip(*rows)
        return (np.array(d, np.int32), np.array(a, np.int32), np.array(v, np.int32), np.array(w, np.float64), np.array(p, np.float32))

    def root_children(self):
        f, k = int(self.first[0]), int(self.n[0])
        if f < 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        return self.action[f:f + k].copy(), self.N[f:f + k].copy()


def search(game, S, **kw):
    return Search(game, S, **kw).run()
