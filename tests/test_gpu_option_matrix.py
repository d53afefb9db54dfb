"""The option setters of the C ABI as one table: which option may be switched on while which other is on, through the return codes alone.

The refusals are also asserted where each option is tested (test_gpu_gumbel, test_gpu_compose, test_gpu_solver, test_gpu_virtual_loss,
test_gpu_visit_targets); here they stand together.  For every ordered pair (A on, then B on) over leaf batching, the solver,
sz_set_search_options (L > 1, solver, both), forced playouts, first-play urgency, Gumbel, endings and the two root-noise setters, on an engine
without options, one created with reuse_subtree and one with learning = 0, B's return code is compared with a literal table; then the disabling
call of each must be accepted.  No search runs for the table.  A second test calls every setter that is bound to "only between searches"
inside a 2-simulation search: each returns SZ_ERR_STATE, and the search, its sz_play and the next search come out as without the calls.

The codes were read off the setters of csrc/sz_engine.hip before their refusals were gathered into one function: '.' SZ_OK, 'I'
SZ_ERR_INVALID (an argument or a combination, decided before the engine is asked whether it searches), 'S' SZ_ERR_STATE."""
import ctypes as C

import numpy as np
import pytest
import torch

from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel

pytestmark = pytest.mark.gpu

B = 2
CODE = {".": N.SZ_OK, "I": N.SZ_ERR_INVALID, "S": N.SZ_ERR_STATE}

#          name    what it is
SETTERS = ["LB",   # sz_set_leaf_batching(2, 1.0)                  off: (1, 1.0)
           "SV",   # sz_set_solver(1)                              off: (0)
           "SOL",  # sz_set_search_options({4, 1.0, 0})            off: ({1, 1.0, 0})
           "SOS",  # sz_set_search_options({1, 1.0, 1})
           "SOB",  # sz_set_search_options({4, 1.0, 1})
           "FP",   # sz_set_forced_playouts(2.0, NULL)             off: (0.0, NULL)
           "FPU",  # sz_set_fpu({reduction 0.33, absolute 1.0})    off: (NULL)
           "GB",   # sz_set_gumbel({16, 50.0, 1.0}, NULL)          off: (NULL, NULL)
           "EN",   # sz_set_endings({-0.9, 3, 0, 0.0, 0, 0, 0})    off: (NULL, NULL)
           "RN",   # sz_set_root_noise(gamma)                      off: (NULL)
           "SRN"]  # sz_set_search_root_noise(gamma, NULL)         off: (NULL, NULL)

# ALONE[engine]: the code of each setter's enabling call on a fresh engine, in SETTERS' order.
# AFTER[engine][A]: the code of each setter's enabling call right after A's enabling call (which returned ALONE[engine][A]; a refused A
# leaves nothing on, so its row is ALONE again).
#                    LB SV SOL SOS SOB FP FPU GB EN RN SRN
ALONE = {"plain":    "...........",
         "reuse":    "II.....I.S.",       # leaf batching, the solver and Gumbel need sz_set_search_options or no reuse; sz_set_root_noise: SZ_ERR_STATE
         "no-learn": ".....I....."}       # forced playouts are an exploration option of self-play
AFTER = {
    "plain": {
        "LB":  ".I.....I...",             # L > 1: the solver's own setter and Gumbel are refused
        "SV":  "I......I...",
        "SOL": ".I.....I...",             # sz_set_search_options leaves sz_set_leaf_batching / sz_set_solver their refusals of each other
        "SOS": "I......I...",
        "SOB": "II.....I...",
        "FP":  ".......I...",
        "FPU": "...........",
        "GB":  "IIIIII..ISS",             # Gumbel on: everything but first-play urgency is refused, root noise with SZ_ERR_STATE
        "EN":  ".......I...",
        "RN":  ".......S...",             # root noise on: Gumbel is refused with SZ_ERR_STATE, after the question whether the engine searches
        "SRN": ".......S..."},
    "reuse": {a: "II.....I.S." for a in SETTERS},                     # nothing that can be on there changes what reuse_subtree refuses
    "no-learn": {
        "LB":  ".I...I.I...",
        "SV":  "I....I.I...",
        "SOL": ".I...I.I...",
        "SOS": "I....I.I...",
        "SOB": "II...I.I...",
        "FP":  ".....I.....",
        "FPU": ".....I.....",
        "GB":  "IIIIII..ISS",
        "EN":  ".....I.I...",
        "RN":  ".....I.S...",
        "SRN": ".....I.S..."}}


def _engine(kind, num_searches=8):
    args = {"C": 2, "num_searches": num_searches}
    if kind == "reuse":
        args["reuse_subtree"] = True
    return SelfPlayEngine(HashModel(), args, B, chess960=True, learning=kind != "no-learn")


class Calls:
    """the enabling and the disabling call of every setter on one engine; the arguments stay alive with the object"""

    def __init__(self, eng):
        lib, e, s = N.lib(), eng._e, eng._stream()
        self.gamma = torch.ones(B, N.SZ_MAX_MOVES, dtype=torch.float32, device="cuda")
        g = C.c_void_p(self.gamma.data_ptr())
        sopt = lambda L, solver: C.byref(N.sz_search_options(L, 1.0, solver))
        fpu = N.sz_fpu_options(N.SZ_FPU_REDUCTION, 0.33, N.SZ_FPU_ABSOLUTE, 1.0)
        gumbel = N.sz_gumbel_options(16, 50.0, 1.0)
        ending = N.sz_ending_options(-0.9, 3, 0, 0.0, 0, 0, 0)
        so_off = lambda: lib.sz_set_search_options(e, sopt(1, 0), s)
        self.on = {"LB": lambda: lib.sz_set_leaf_batching(e, 2, 1.0, s),
                   "SV": lambda: lib.sz_set_solver(e, 1, s),
                   "SOL": lambda: lib.sz_set_search_options(e, sopt(4, 0), s),
                   "SOS": lambda: lib.sz_set_search_options(e, sopt(1, 1), s),
                   "SOB": lambda: lib.sz_set_search_options(e, sopt(4, 1), s),
                   "FP": lambda: lib.sz_set_forced_playouts(e, 2.0, None, s),
                   "FPU": lambda: lib.sz_set_fpu(e, C.byref(fpu), s),
                   "GB": lambda: lib.sz_set_gumbel(e, C.byref(gumbel), None, s),
                   "EN": lambda: lib.sz_set_endings(e, C.byref(ending), None, s),
                   "RN": lambda: lib.sz_set_root_noise(e, g),
                   "SRN": lambda: lib.sz_set_search_root_noise(e, g, None, s)}
        self.off = {"LB": lambda: lib.sz_set_leaf_batching(e, 1, 1.0, s),
                    "SV": lambda: lib.sz_set_solver(e, 0, s),
                    "SOL": so_off, "SOS": so_off, "SOB": so_off,
                    "FP": lambda: lib.sz_set_forced_playouts(e, 0.0, None, s),
                    "FPU": lambda: lib.sz_set_fpu(e, None, s),
                    "GB": lambda: lib.sz_set_gumbel(e, None, None, s),
                    "EN": lambda: lib.sz_set_endings(e, None, None, s),
                    "RN": lambda: lib.sz_set_root_noise(e, None),
                    "SRN": lambda: lib.sz_set_search_root_noise(e, None, None, s)}

    def all_off(self, tag):
        # sz_set_search_root_noise first: while its noise is on, a reuse_subtree engine is left through that setter alone (asserted below)
        for name in ["SRN"] + SETTERS[:-1]:
            assert self.off[name]() == N.SZ_OK, "%s: switching %s off" % (tag, name)


def test_tables_are_whole():
    for kind in ALONE:
        assert len(ALONE[kind]) == len(SETTERS) and sorted(AFTER[kind]) == sorted(SETTERS)
        assert all(len(row) == len(SETTERS) and set(row) <= set(CODE) for row in AFTER[kind].values())


@pytest.mark.parametrize("kind", ["plain", "reuse", "no-learn"])
def test_every_ordered_pair(kind):
    eng = _engine(kind)
    calls = Calls(eng)
    wrong = []
    for i, a in enumerate(SETTERS):
        rc = calls.on[a]()
        if rc != CODE[ALONE[kind][i]]:
            wrong.append("%s alone: %d, table %s" % (a, rc, ALONE[kind][i]))
        calls.all_off("%s after %s" % (kind, a))
    for i, a in enumerate(SETTERS):
        for j, b in enumerate(SETTERS):
            tag = "%s: %s then %s" % (kind, a, b)
            assert calls.on[a]() == CODE[ALONE[kind][i]], tag
            rc = calls.on[b]()
            if rc != CODE[AFTER[kind][a][j]]:
                wrong.append("%s then %s: %d, table %s" % (a, b, rc, AFTER[kind][a][j]))
            calls.all_off(tag)
    if kind == "reuse":
        # the one disabling call with a rule of its own: a reuse_subtree engine under sz_set_search_root_noise leaves it through that setter
        assert calls.on["SRN"]() == N.SZ_OK
        assert calls.off["RN"]() == N.SZ_ERR_STATE
        assert calls.off["SRN"]() == N.SZ_OK and calls.off["RN"]() == N.SZ_OK
    eng.close()
    assert not wrong, "%s engine, %d of %d codes differ:\n%s" % (kind, len(wrong), len(SETTERS) * (len(SETTERS) + 1), "\n".join(wrong))


def _two_plies(meddle):
    """a 2-simulation search, sz_play and the next search; meddle: every between-searches setter is called after sz_search_begin and after
    the first step, and must answer SZ_ERR_STATE.  sz_set_root_noise is not among them: it takes no stream and the header binds it to no
    such rule (it answers SZ_OK inside a search on this engine)."""
    eng = _engine("plain", num_searches=2)
    calls = Calls(eng)
    lib, e, s = N.lib(), eng._e, eng._stream()
    two = (C.c_int32 * B)(1, 2)
    bound = [n for n in SETTERS if n != "RN"]
    inside = [(n + " on", calls.on[n]) for n in bound] + [(n + " off", calls.off[n]) for n in bound] + [
        ("budgets", lambda: lib.sz_set_search_budgets(e, two, s)), ("budgets off", lambda: lib.sz_set_search_budgets(e, None, s)),
        ("targets", lambda: lib.sz_set_visit_targets(e, two, s)), ("targets off", lambda: lib.sz_set_visit_targets(e, None, s))]
    eng.new_games([0, 518])
    eng.begin()
    for step in range(2):
        if meddle:
            for name, call in inside:
                assert call() == N.SZ_ERR_STATE, "%s before step %d of the search" % (name, step + 1)
        eng.step(*eng.evaluate(eng.planes))
    assert eng.check_errors()["boards_done"] == B
    out = [[eng.debug_tree(b) for b in range(B)], eng.root_children()]
    eng.play([0.5] * B)
    rec = eng.fetch_ply()
    out.append([rec[k] for k in sorted(rec)])
    eng.search()
    eng.check_errors()
    out.append([eng.debug_tree(b) for b in range(B)])
    if meddle:                                                       # the search is over: the same calls are accepted again
        for n in bound:
            assert calls.on[n]() == N.SZ_OK, n
            calls.all_off(n)
    eng.close()
    return out


def _flat(x):
    return [x] if isinstance(x, np.ndarray) else [y for part in x for y in _flat(part)]


def test_inside_a_search_every_setter_is_refused_and_nothing_changes():
    want, got = _flat(_two_plies(False)), _flat(_two_plies(True))
    assert len(want) == len(got) and len(want) > 10
    assert all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(want, got))
