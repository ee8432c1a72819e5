"""The fp16 convolution kernels give the bits of the commit they were merged from.

tests/f16_conv_bits.py runs every served (case, variant) pair of the tables of tests/f16_matrix.py - one-tile, persistent multi-tile
(groups 1 and 3), weights in registers (stride 1 and 2), weight-stationary (groups 2 and 5) and the four-phase data gradient - as the
plain launch, with epilogue statistics in both modes where they are served, and with the BatchNorm on the operand where that form is
served, on seeded inputs over pre-filled outputs.  tests/golden/f16_conv_bits.json holds one SHA-256 per (case, variant, knob set)
over the output, partial-sum and activation bytes of all its modes (variants that leave the same bytes stand under one digest),
recorded by tests/golden/gen_f16_conv_bits.py on the GPU FROM THE PARENT COMMIT'S LIBRARY: a changed k order, epilogue association,
partial-sum slot or an element that is no longer written changes a digest.
"""
import json
import os

import pytest

from tests import f16_conv_bits as cb

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16_conv_bits.json")) as _f:
    GOLDEN = json.load(_f)


def _recorded_keys(group):
    return [f"{run.split('|')[0]}-v{v}|{run.split('|')[1]}" for run, by_digest in GOLDEN[group].items() for vs in by_digest.values() for v in vs]


@pytest.mark.parametrize("group", list(cb.GROUPS))
def test_every_served_pair_is_recorded(group):
    assert GOLDEN[group] and sorted(_recorded_keys(group)) == sorted(cb.expected_keys(group))


@pytest.mark.gpu
@pytest.mark.parametrize("group,ci,env", [pytest.param(g, ci, env, id=f"{g}-case{ci}-{cb.knob_id(env)}") for g in cb.GROUPS
                                          for ci, env in cb.runs(g)])
def test_conv_bits_equal_parent(group, ci, env):
    assert cb.pack(cb.digests(group, ci, env)) == GOLDEN[group].get(cb.run_id(ci, env), {})
