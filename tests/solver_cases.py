"""Case set shared by the solver tests (tests/test_solver_ref.py on the host, tests/test_gpu_solver.py on the device): constructed
positions with known game-theoretic answers, and the fixpoint check of a finished tree's labels.  Every position was checked with the
host restatement (tests/solverref.py) before it was relied on; tests/test_solver_ref.py asserts what is claimed here."""
import numpy as np

import solverref
from solverref import UNKNOWN, WIN, DRAW, LOSS

FENS = {
    "mate_in_1": "6k1/5ppp/8/8/8/8/8/R6K w - - 0 1",                     # Ra8#: 16 moves, one of them mates
    "moves_218": "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1",  # 218 legal moves: the root's children span four 64-lane passes
    "forced_draw": "7k/8/8/8/8/8/1q6/K7 w - - 0 1",                       # Kxb2 is the only legal move and leaves bare kings
    "mated_in_2": "k7/8/1K6/8/8/p7/8/7R b - - 0 1",                       # ...Kb8 and ...a2 both allow Rh8#
    "refuted_move": "6k1/5ppp/8/8/8/8/8/R6K b - - 0 1",                   # ...Kh8 walks into Ra8#, the other seven moves do not
    "endgame_6_men": "8/2k5/4p3/8/8/4P3/1Q2K3/7R w - - 0 1",
}

# (name, S, salt of the hash network).  The salts were chosen so that, at learning = 0, the search visits what the case is about
# within S <= 200 simulations; the tests assert it.
CASES = [
    ("mate_in_1", 64, 0), ("mate_in_1", 200, 1),
    ("moves_218", 200, 0), ("moves_218", 64, 1),
    ("forced_draw", 64, 0),
    ("mated_in_2", 200, 0), ("mated_in_2", 200, 2),
    ("refuted_move", 200, 2), ("refuted_move", 64, 2),
]


def game(name):
    import sigma_zero_amd as sz
    return sz.ChessTensor(fen=FENS[name])


def fixpoint_labels(s):
    """Labels of every edge of the finished tree of search `s`, recomputed bottom-up from terminal leaves and `complete` alone (no use of
    s.R): edges are created after their parents, so one pass over the edge indices in descending order sees children before parents."""
    lab = np.zeros(s.n_edges, np.int8)
    for e in range(s.n_edges - 1, -1, -1):
        if s.term[e]:
            lab[e] = LOSS if s.tval[e] == -1 else DRAW
        elif s.n[e] > 0:
            lab[e] = combine(lab[s.first[e]:s.first[e] + s.n[e]], s.complete[e])
    return lab


def combine(child_labels, complete):
    if (child_labels == LOSS).any():
        return WIN
    if complete and (child_labels != UNKNOWN).all():
        return DRAW if (child_labels == DRAW).any() else LOSS
    return UNKNOWN


def check_fixpoint(s, tag=""):
    lab = fixpoint_labels(s)
    R = s.R[:s.n_edges]
    proven = np.nonzero(R != UNKNOWN)[0]
    assert np.array_equal(R[proven], lab[proven]), "%s: a node proven by the search carries another label than the recursion" % tag
    for e in range(s.n_edges):                                  # what can be proven from already-proven children is proven
        if s.n[e] > 0 and not s.term[e]:
            want = combine(R[s.first[e]:s.first[e] + s.n[e]], s.complete[e])
            assert R[e] == want, "%s: edge %d is %d, its children give %d" % (tag, e, R[e], want)
    assert np.array_equal(R, lab), tag
    return lab


def run(name, S, salt, learning=False, solver=True):
    return solverref.search(game(name), S, solver=solver, learning=learning, mode="dyadic", salt=salt)
