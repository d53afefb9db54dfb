"""args["leaves_per_step"] / ["virtual_loss"] / ["solver"] / ["combine_options"] / ["reuse_subtree"] as SelfPlayEngine reads them
(selfplay.search_options_of, a pure function): what each valid combination parses to, and the ValueError every refused one raises,
message text and order of the checks included.  Needs no GPU."""
import numpy as np
import pytest

from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import search_options_of

LMAX = N.SZ_MAX_LEAVES_PER_STEP
BASE = {"C": 2, "num_searches": 16}

E_L = r"args\['leaves_per_step'\] must be an integer in 1\.\.%d, got %%s" % LMAX
E_LAM = r"args\['virtual_loss'\] must be a finite number >= 0, got %s"
E_COMBINE = r"args\['combine_options'\] must be True or False, got %s"
E_SOLVER = r"args\['solver'\] must be True or False, got %s"
E_L_REUSE = r"args\['leaves_per_step'\] > 1 and args\['reuse_subtree'\] exclude each other \(without args\['combine_options'\]\)"
E_SOLVER_REUSE = r"args\['solver'\] and args\['reuse_subtree'\] exclude each other \(without args\['combine_options'\]\)"
E_SOLVER_L = r"args\['solver'\] and args\['leaves_per_step'\] > 1 exclude each other \(without args\['combine_options'\]\)"


def test_defaults():
    assert search_options_of(BASE) == (1, 1.0, False, False)
    assert search_options_of({}) == (1, 1.0, False, False)                 # reads the option keys only
    out = search_options_of({"leaves_per_step": np.int32(4), "virtual_loss": np.float32(0.5), "solver": np.bool_(False), "combine_options": np.bool_(True)})
    assert out == (4, 0.5, False, True)
    assert [type(x) for x in out] == [int, float, bool, bool]


# one option at a time needs no combine_options; every pair and the triple are legal with it, in any combination
@pytest.mark.parametrize("combine", [False, True])
@pytest.mark.parametrize("L,solver,reuse", [(1, False, False), (7, False, False), (LMAX, False, False), (1, True, False), (1, False, True),
                                            (7, True, False), (7, False, True), (1, True, True), (7, True, True)])
def test_valid_combinations(L, solver, reuse, combine):
    args = dict(BASE, leaves_per_step=L, virtual_loss=0.25, solver=solver, reuse_subtree=reuse, combine_options=combine)
    pairs = (L > 1) + bool(solver) + bool(reuse) > 1
    if pairs and not combine:
        with pytest.raises(ValueError):
            search_options_of(args)
    else:
        assert search_options_of(args) == (L, 0.25, solver, combine)
    assert args == dict(BASE, leaves_per_step=L, virtual_loss=0.25, solver=solver, reuse_subtree=reuse, combine_options=combine)    # args untouched


@pytest.mark.parametrize("args,message", [
    ({"leaves_per_step": True}, E_L % "True"),
    ({"leaves_per_step": 0}, E_L % "0"),
    ({"leaves_per_step": LMAX + 1}, E_L % str(LMAX + 1)),
    ({"leaves_per_step": 2.0}, E_L % r"2\.0"),
    ({"virtual_loss": -0.5}, E_LAM % r"-0\.5"),
    ({"virtual_loss": float("nan")}, E_LAM % "nan"),
    ({"virtual_loss": float("inf")}, E_LAM % "inf"),
    ({"virtual_loss": True}, E_LAM % "True"),
    ({"combine_options": 1}, E_COMBINE % "1"),
    ({"combine_options": "yes"}, E_COMBINE % "'yes'"),
    ({"solver": 1}, E_SOLVER % "1"),
    ({"solver": None}, E_SOLVER % "None"),
    ({"leaves_per_step": 2, "reuse_subtree": True}, E_L_REUSE),
    ({"solver": True, "reuse_subtree": True}, E_SOLVER_REUSE),
    ({"solver": True, "leaves_per_step": 2}, E_SOLVER_L),
])
def test_refusals(args, message):
    with pytest.raises(ValueError, match="^" + message + "$"):
        search_options_of(dict(BASE, **args))


# the checks run in a fixed order: the first one that fails speaks
@pytest.mark.parametrize("args,message", [
    ({"leaves_per_step": 0, "virtual_loss": -1.0, "combine_options": 1, "solver": 1}, E_L % "0"),
    ({"virtual_loss": -1.0, "combine_options": 1, "solver": 1}, E_LAM % r"-1\.0"),
    ({"combine_options": 1, "leaves_per_step": 2, "reuse_subtree": True, "solver": 1}, E_COMBINE % "1"),
    ({"leaves_per_step": 2, "reuse_subtree": True, "solver": 1}, E_L_REUSE),
    ({"solver": 1, "reuse_subtree": True}, E_SOLVER % "1"),
    ({"solver": True, "reuse_subtree": True, "leaves_per_step": 1}, E_SOLVER_REUSE),
    ({"solver": True, "reuse_subtree": True, "leaves_per_step": 2}, E_L_REUSE),
])
def test_order_of_checks(args, message):
    with pytest.raises(ValueError, match="^" + message + "$"):
        search_options_of(dict(BASE, **args))
