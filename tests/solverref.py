"""Plain-Python restatement of the engine's search with proven-result propagation (sz_set_solver, a NON-REFERENCE option;
include/sigmazero.h is the specification).  It is what the HIP kernels (csrc/sz_engine.hip k_search_step<false, true>, k_play<true>) are
held to, bit for bit.  A sibling of vlref.Search at L = 1 with its own run loop; with solver=False that loop is vlref's search, which
tests/test_solver_ref.py pins.

  * every node e carries R[e] in {UNKNOWN, WIN, DRAW, LOSS} for the side to move in its position and complete[e] (expansion kept every
    legal move);
  * a terminal leaf is labelled when its position is made; after its backup the labels are carried up the backed-up path (_update);
  * a descent ends at the first proven node (the root included) and backs up -1 / 0 / +1; selection skips children that are WIN.

The counters beyond the engine's (skips, proved_by_label, two_up, root_proven_at) exist for the tests' conditions only."""
import math

import numpy as np

import vlref
from hashmodel import evaluate_packed
from vlref import F32, ucb

UNKNOWN, WIN, DRAW, LOSS = 0, 1, 2, 3                   # the codes of sz_root_proven
VALUE = {WIN: 1.0, DRAW: 0.0, LOSS: -1.0}


class Search(vlref.Search):
    def __init__(self, game, S, solver=True, **kw):
        super().__init__(game, S, L=1, **kw)
        self.solver = bool(solver)
        self.R = np.zeros(len(self.W), np.int8)
        self.complete = np.zeros(len(self.W), np.uint8)
        self.expansions = self.terminal_hits = self.sum_depth = 0       # sz_get_stats
        self.proven_stops = self.proved = 0                              # sz_solver_stats
        self.skips = 0                                   # selections whose unrestricted arg-max was a WIN child
        self.proved_by_label = {WIN: 0, DRAW: 0, LOSS: 0}
        self.two_up = 0                                  # nodes proven two or more levels above the terminal leaf that started the walk
        self.root_proven_at = None                       # simulations done when the root became proven

    def _expand(self, e, pol):
        super()._expand(e, pol)
        if self.solver and int(self.n[e]) == len(self.games[e].legal_action_indices()):
            self.complete[e] = 1

    def _descend(self):
        path, e = [0], 0
        while self.n[e] > 0 and not (self.solver and self.R[e]):
            f, k = self.first[e], self.n[e]
            sq = F32(math.sqrt(float(self.N[e])))
            u = ucb(self.N[f:f + k], self.W[f:f + k], self.P[f:f + k], sq, self.c)
            i = int(np.argmax(u))
            if self.solver:
                cand = np.nonzero(self.R[f:f + k] != WIN)[0]
                if len(cand):                            # every child WIN: all children, as without the solver
                    self.skips += 1 if self.R[f + i] == WIN else 0
                    i = int(cand[np.argmax(u[cand])])
            e = f + i
            path.append(e)
        return path

    def _update(self, path):
        """path[-1] has just become proven: recompute the parents towards the root, each from its children alone"""
        for j in range(len(path) - 1, 0, -1):
            p = path[j - 1]
            r = self.R[self.first[p]:self.first[p] + self.n[p]]
            if (r == LOSS).any():
                new = WIN
            elif self.complete[p] and (r != UNKNOWN).all():
                new = DRAW if (r == DRAW).any() else LOSS
            else:
                new = UNKNOWN
            if new == self.R[p]:
                break
            self.R[p] = new
            self.proved += 1
            self.proved_by_label[new] += 1
            self.two_up += 1 if len(path) - j >= 2 else 0
            if p == 0:
                self.root_proven_at = self.sims

    def _end(self, path, v):
        self._backprop(path, v)
        self.terminal_hits += 1
        self.sum_depth += len(path) - 1

    def run(self):
        root = self.games[0]
        tv, term = root.get_value_and_terminated()
        if term or self.S <= 0:                          # a terminal root: every simulation re-visits it (mcts.py:104-109)
            S = max(self.S, 0)
            self.W[0], self.N[0], self.sims, self.terminal_hits = float(tv) * S, 1 + S, S, S
            if self.solver and term:
                self.R[0] = LOSS if tv == -1 else DRAW
            return self
        pending = ([0], self._planes(0))
        while pending is not None:
            path, planes = pending
            self.steps.append(planes[None])
            pol, val = evaluate_packed(planes, self.mode, self.salt)
            self._expand(path[-1], pol)
            self._backprop(path, float(val))
            self.expansions += 1
            self.sum_depth += len(path) - 1
            pending = None
            while self.sims < self.S:
                path = self._descend()
                e = path[-1]
                if self.solver and self.R[e]:            # the first proven node on the way (a visited terminal leaf is one)
                    self._end(path, VALUE[int(self.R[e])])
                    self.proven_stops += 0 if self.term[e] else 1
                    continue
                if e in self.games:                      # visited leaf without children
                    self._end(path, float(self.tval[e]))
                    continue
                g = self.games[path[-2]].copy()
                g.push_action(int(self.action[e]))
                self.games[e] = g
                v, t = g.get_value_and_terminated()
                self.term[e], self.tval[e] = int(t), int(v) if t else 0
                if t:
                    if self.solver:
                        self.R[e] = LOSS if v == -1 else DRAW
                    self._end(path, float(v))
                    if self.solver:
                        self._update(path)
                    continue
                pending = (path, self._planes(e))
                break
        return self

    # -- readouts
    def tree_proven(self):
        """(proven, complete) of every node in tree()'s order (sz_debug_tree_proven)"""
        out, stack = [], [0]
        while stack:
            e = stack.pop()
            out.append((int(self.R[e]), int(self.complete[e])))
            if self.first[e] >= 0:
                stack += [self.first[e] + k for k in range(int(self.n[e]) - 1, -1, -1)]
        r, c = zip(*out)
        return np.array(r, np.int8), np.array(c, np.uint8)

    def root_proven(self):
        """(root code, codes of the root's children in action order) (sz_root_proven)"""
        f, k = int(self.first[0]), int(self.n[0])
        return int(self.R[0]), (self.R[f:f + k].copy() if f >= 0 else np.zeros(0, np.int8))

    def choose(self, u):
        """index of the root child sz_play plays: the first LOSS child of a WIN root, else np.random.choice(p = visits / sum) given the
        uniform it draws (cumulative f64 sums divided by the last, searchsorted 'right', clamped); u < 0: the first most visited child"""
        r, rc = self.root_proven()
        if self.solver and r == WIN:
            return int(np.nonzero(rc == LOSS)[0][0])
        vis = self.root_children()[1]
        if u < 0.0:
            return int(np.argmax(vis))
        cdf = np.cumsum(vis.astype(np.float64) / np.float64(vis.sum()))
        cdf = cdf / cdf[-1]
        return min(int(np.searchsorted(cdf, u, side="right")), len(vis) - 1)


def search(game, S, **kw):
    return Search(game, S, **kw).run()
