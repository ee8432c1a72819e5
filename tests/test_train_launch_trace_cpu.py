"""What the training path launches, call for call, held to a recording of the commit a change to train_ops.py started from.

tests/train_trace.py runs whole training steps and every autograd Function of `mindpose_amd/models/train_ops.py` on host tensors
against a recording library (no device): every library call with its normalised arguments and every torch op that does work, in
order.  tests/golden/train_launch_trace.json holds, per case, the SHA-256 of that trace and its counts per name; it is written by
tests/golden/gen_train_launch_trace.py IN A WORKTREE OF THE PARENT COMMIT and never regenerated from a changed train_ops.py (a
change that means to alter a launch regenerates it from its own parent first and then shows the diff of the two ``--dump``s).

The fake library's answers: ``*_bytes`` 1024, ``*_parts`` 4, ``mp_conv_winograd_supported`` 0, ``mp_f16_conv_pre_supported`` 1,
everything else 0.  ``empty*`` allocations may only go down.
"""
import json
import os

import pytest

from tests import train_trace

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_launch_trace.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(train_trace.CASES)


@pytest.mark.parametrize("name", list(train_trace.CASES))
def test_launch_trace_equals_parent(name):
    got = train_trace.summarise(*train_trace.trace_case(name))
    want = GOLDEN[name]
    assert got["counts"] == want["counts"]  # first: a difference here says where to look
    assert got["events"] == want["events"]
    assert got["sha256"] == want["sha256"]
    assert got["empty"] <= want["empty"]


def test_trace_repeats():
    """A case traces the same wherever it stands in a run (every process-wide cache is cleared around it)."""
    first = train_trace.summarise(*train_trace.trace_case("hrnet_o2"))
    train_trace.trace_case("fn_conv_k3s2_f16_direct")
    assert train_trace.summarise(*train_trace.trace_case("hrnet_o2")) == first
