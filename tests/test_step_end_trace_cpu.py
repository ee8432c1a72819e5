"""What the step end launches, call for call, held to a recording of the commit a change to it started from.

tests/step_end_trace.py runs three consecutive step ends of AdamWeightDecay, Adam and SGD with momentum - host-driven
(``_ArenaOptimizer.step``) and resident (``ResidentStepTail.launch``), with and without a loss-scale manager, with and without
clipping, on a module with both decay groups and on one whose decay group is empty - on host tensors against a recording library
(no device).  tests/golden/step_end_launch_trace.json holds, per case, the SHA-256 of that trace and its counts per name; it is
written by tests/golden/gen_step_end_trace.py IN A WORKTREE OF THE PARENT COMMIT and never regenerated from changed modules.
``empty*`` allocations may only go down.
"""
import json
import os

import pytest

from tests import step_end_trace

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_end_launch_trace.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(step_end_trace.CASES)
    assert len(step_end_trace.CASES) == 3 * 2 * 8


@pytest.mark.parametrize("name", list(step_end_trace.CASES))
def test_step_end_trace_equals_parent(name):
    got = step_end_trace.summarise(*step_end_trace.trace_case(name))
    want = GOLDEN[name]
    assert got["counts"] == want["counts"]  # first: a difference here says where to look
    assert got["events"] == want["events"]
    assert got["sha256"] == want["sha256"]
    assert got["empty"] <= want["empty"]


def test_the_cases_exercise_what_they_name():
    """The empty decay group launches nothing, the host-driven step under a manager skips its second update, and clipping reaches
    the update launches as a factor of the gradient scale."""
    def updates(name):
        return [e for e in step_end_trace.trace_case(name)[0] if e[0] in ("mp_adamw_step_scaled", "mp_adamw_step_resident")]

    assert len(updates("adamw-two_groups-host-plain-noclip")) == 2 * step_end_trace.STEPS
    assert len(updates("adamw-no_decay_only-host-plain-noclip")) == step_end_trace.STEPS
    assert len(updates("adamw-two_groups-host-manager-noclip")) == 2 * (step_end_trace.STEPS - 1)
    assert len(updates("adamw-two_groups-resident-manager-clip")) == 2 * step_end_trace.STEPS
    plain, clipped = updates("adamw-two_groups-host-plain-noclip")[0], updates("adamw-two_groups-host-plain-clip")[0]
    assert clipped[11] == 0.5 * plain[11]  # grad_scale
