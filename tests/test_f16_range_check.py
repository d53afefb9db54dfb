"""SelfPlayEngine.check_errors()'s look at the evaluator's range flag (selfplay.raise_if_overflowed), without a GPU: the message, the sticky read, and the
evaluators that have no flag."""
import pytest
import torch

from sigma_zero_amd.selfplay import raise_if_overflowed


class _Flagged:
    operands = "fp16"

    def __init__(self, hits):
        self.hits = list(hits)

    def overflowed(self):
        return self.hits.pop(0)


def test_overflow_is_a_value_error_that_names_the_way_out():
    net = _Flagged([True, False])
    with pytest.raises(ValueError) as e:
        raise_if_overflowed(net)
    msg = str(e.value)
    assert "_Flagged(operands='fp16')" in msg and "65504" in msg and "inf / NaN" in msg and 'use operands="bf16" or SplitPolicyNet' in msg
    raise_if_overflowed(net)                                 # the read cleared it: the second look passes
    assert net.hits == []


def test_evaluators_without_a_flag_pass():
    raise_if_overflowed(None)                                # an engine driven by the caller (model=None)
    raise_if_overflowed(torch.nn.Linear(2, 2))               # a torch module: no overflowed()
    odd = torch.nn.Linear(2, 2)
    odd.overflowed = 1                                       # an attribute that is no method is not called
    raise_if_overflowed(odd)
    raise_if_overflowed(_Flagged([False]))                   # a bf16 network's flag: always False
