"""The weight-gradient kernels give the bits of the commit they were merged from.

tests/wgrad_bits.py runs every row of the three tables of tests/wgrad_matrix.py - every kernel instantiation, form and reduce kernel
on workgroups of three tiles or more, and every job of the grouped rows - with accumulate = 0 and with accumulate = 1 on a seeded
destination.  tests/golden/wgrad_bits.json holds the SHA-256 of each weight gradient, recorded by tests/golden/gen_wgrad_bits.py on the
GPU FROM THE PARENT COMMIT'S LIBRARY: a changed tile order, split partition, reduce association, scale or accumulate step changes a
digest.
"""
import json
import os

import pytest

from tests import wgrad_matrix as wm

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_bits.json")) as _f:
    GOLDEN = json.load(_f)

ROWS = {"f32": [(c, k, 1) for c, k, _ in wm.F32_CASES], "f16": [(c, k, 1) for c, k, _ in wm.F16_CASES], "f16_grouped": wm.F16_GROUPED_CASES}


def test_every_row_and_job_is_recorded():
    for table, rows in ROWS.items():
        assert list(GOLDEN[table]) == [wm.case_id(c, k) for c, k, _ in rows], table
        for (c, k, jobs), rec in zip(rows, GOLDEN[table].values()):
            assert sorted(rec) == [f"job{j}" for j in range(jobs)] and all(len(v) == 2 and v[0] != v[1] for v in rec.values())


@pytest.mark.gpu
@pytest.mark.parametrize("table,i", [pytest.param(t, i, id=f"{t}-{wm.case_id(c, k)}") for t, rows in ROWS.items()
                                     for i, (c, k, _) in enumerate(rows)])
def test_wgrad_bits_equal_parent(table, i):
    from tests import wgrad_bits as wb
    assert wb.digests(table, i) == GOLDEN[table][wb.run_id(table, i)]
