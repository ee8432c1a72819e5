"""The weight-gradient family builds the launches of the commit its host code was merged from.

tests/wgrad_launch_words.py asks ``mp_conv_wgrad_launch_words`` (host-only) for the launch of every row of the tables of
tests/wgrad_matrix.py, of the layer shapes of the two bench tools (single-layer and grouped) and of 600 seeded random shapes under
their knob draws; tests/golden/wgrad_launch_words.json holds one SHA-256 per record over those launches - return code, every
non-pointer field of the kernel parameter block, grid, block, LDS bytes, kernel and slab reduce - recorded by
tests/golden/gen_wgrad_launch_words.py FROM THE PARENT COMMIT'S LIBRARY: a changed tile height, pitch, split count, magic number,
kernel pick, reduce pick or refusal changes a digest.  The number of accepted launches shows that real launches were compared, and
seven records carry their word lists so that a mismatch can be read.
"""
import functools
import json

import pytest

from tests import wgrad_launch_words as lw

with open(lw.GOLDEN_PATH) as _f:
    GOLDEN = json.load(_f)

QUERIES = lw.queries()


@functools.lru_cache(maxsize=None)
def _records():
    return {name: lw.record(name, qs) for name, qs in QUERIES.items()}


def test_every_record_is_there_and_launches_are_accepted():
    assert list(GOLDEN["sha256"]) == list(QUERIES)
    assert sorted(GOLDEN["words"]) == sorted(lw.FULL) and all(w[0] == 0 for lists in GOLDEN["words"].values() for w in lists)
    assert GOLDEN["accepted"] > len(QUERIES)
    assert sum(rec[1] for rec in _records().values()) == GOLDEN["accepted"]


@pytest.mark.parametrize("name", lw.FULL)
def test_launch_words_read_as_the_parent_s(name):
    for (case, half, jobs, env), got, want in zip(QUERIES[name], _records()[name][2], GOLDEN["words"][name]):
        fields = lw.wm.WORDS16 if half else lw.wm.WORDS32
        assert dict(zip(fields, got)) == dict(zip(fields, want)), (name, jobs)


@pytest.mark.parametrize("table", ["f32", "f16", "f16_grouped", "bench32", "bench16", "random"])
def test_launch_words_equal_parent(table):
    names = [name for name in QUERIES if name.split("/")[0] == table]
    assert names
    for name in names:
        assert _records()[name][0] == GOLDEN["sha256"][name], name
