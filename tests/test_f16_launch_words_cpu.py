"""The fp16 convolution family builds the launch records of the commit its host code was merged from.

tests/f16_launch_words.py asks ``mp_f16_conv_launch_words`` (host-only) for the launch of every desc of the test tables and of the
three bench plans, under every variant (-1 .. 47), residual count / statistics mode and test knob, and
tests/golden/f16_launch_words.json holds one SHA-256 per (desc, knob set) over all of those records (stored where it differs from
the desc's digest without knobs) - return codes, LDS bytes and
every field of the kernel parameter block - recorded by tests/golden/gen_f16_launch_words.py FROM THE PARENT COMMIT'S LIBRARY: a
changed tile height, plane pitch, magic number or refusal changes a digest.  The numbers of accepted combinations per kernel family
show that real launches were compared, and six descs carry their word lists so that a mismatch can be read.
"""
import functools
import json

import pytest

from tests import f16_launch_words as lw

with open(lw.GOLDEN_PATH) as _f:
    GOLDEN = json.load(_f)

DESCS = lw.descs()


@functools.lru_cache(maxsize=None)
def _records(knob_set):
    """{desc: (digest, served, word lists)} under one knob set, computed once"""
    return {name: lw.record(d, knob_set, full=(lw.FULL.get(name) == knob_set)) for name, d in DESCS.items()}


def test_every_desc_is_recorded_and_every_family_is_served():
    assert sorted(GOLDEN["sha256"]) == sorted(DESCS) and all("none" in v and set(v) <= set(lw.KNOBS) for v in GOLDEN["sha256"].values())
    assert sorted(GOLDEN["words"]) == sorted(lw.FULL) and all(GOLDEN["words"].values())
    assert set(GOLDEN["served_total"]) == set(lw.FAMILIES) | {"heuristic"}
    assert all(n > 0 for n in GOLDEN["served_total"].values()), GOLDEN["served_total"]
    got = {family: sum(rec[1][family] for ks in lw.KNOBS for rec in _records(ks).values()) for family in GOLDEN["served_total"]}
    assert got == GOLDEN["served_total"]


@pytest.mark.parametrize("name", list(lw.FULL))
def test_launch_words_read_as_the_parent_s(name):
    got = lw.pack_words(_records(lw.FULL[name])[name][2])
    want = GOLDEN["words"][name]
    assert sorted(got) == sorted(want), "the variants that build"
    for v in want:
        for mode in want[v]:
            assert got[v][mode] == want[v][mode], f"{name}, variant {v}, {mode}"


@pytest.mark.parametrize("knob_set", list(lw.KNOBS))
def test_launch_words_equal_parent(knob_set):
    for name, rec in _records(knob_set).items():  # a knob set that is not stored has the digest of "none"
        assert rec[0] == GOLDEN["sha256"][name].get(knob_set, GOLDEN["sha256"][name]["none"]), f"{name}, {knob_set}"
