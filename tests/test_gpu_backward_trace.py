"""GPU: the launch schedule of the backbone's autograd layer (erd_amd.functional: the stage and block nodes, ConvBNAct, DeformConvBNAct,
HeadConvBias) against the pinned one in tests/golden/backward_launch_trace.json -- which kernel entry goes out, in which order, on which
stream (main / trailing / auxiliary), and how many members a weight-gradient launch carries.  The numerical tests of these nodes check
each of them against a reference; none of them notices a launch that moved to another stream, a reduce that became an AccumulateGrad
add, or a grouped launch that fell back to one launch per block.  A change that alters the schedule on purpose regenerates the fixture
(tools/gen_backward_trace_golden.py)."""
import json
import os

import pytest

import backward_trace_cases as B

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backward_launch_trace.json")) as _f:
    PINNED = json.load(_f)


def test_every_case_is_pinned():
    assert sorted(PINNED) == sorted(B.CASES)


@pytest.mark.parametrize("name", list(B.CASES))
def test_backward_launch_trace(name):
    trace, grads = B.record(name)
    want = PINNED[name]
    print(f"{name}: {len(trace)} launches ({sum(e[1] == 'trail' for e in trace)} trailing), pinned {len(want)}")
    assert len(trace) > 0 and all(float(g.abs().max()) > 0 for g in grads.values())
    diff = B.first_difference(trace, want)
    assert diff is None, f"{name}: {diff}"
