"""The update entries of csrc/step_end.hip give the bits of the commit their kernels were merged from.

tests/step_end_bits.py runs every update entry - ``mp_adamw_step``, ``mp_adamw_step_scaled`` (no flag, skip 0, skip 1),
``mp_adamw_step_resident`` (skip 0, skip 1), ``mp_optimizer_step`` and ``mp_optimizer_step_resident`` for the eight variants of
tests/glue_matrix.py - at counts 1, 3, 255, 256, 257 and one that crosses the grid cap with a ragged end, on finite values of every
magnitude, and once more at 257 with +inf, -inf and NaN planted in the gradient.  tests/golden/step_end_update_digests.json holds
the SHA-256 of the parameter and state bytes each case leaves behind (planted cases: the digest of the outputs that are not NaN and
the indices of those that are), recorded by tests/golden/gen_step_end_golden.py on the GPU FROM THE PARENT COMMIT'S LIBRARY: a
changed contraction or association inside an inlined update rule changes a digest.
"""
import json
import os

import pytest

from tests import step_end_bits

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_end_update_digests.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(step_end_bits.case_id(*c) for c in step_end_bits.CASES)
    assert len(step_end_bits.ENTRIES) == 6 + 2 * 8


@pytest.mark.parametrize("entry", list(step_end_bits.ENTRIES))
def test_update_bits_equal_parent(entry):
    for case in step_end_bits.CASES:
        if case[0] == entry:
            assert step_end_bits.digest(*case) == GOLDEN[step_end_bits.case_id(*case)], step_end_bits.case_id(*case)
