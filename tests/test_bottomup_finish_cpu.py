"""The device tail of a bottom-up batch without a GPU: the restatement of its arithmetic (``tests/finish_restated.py``) held bit for
bit to this machine's numpy and to the host ``refine_missing_joint``, every host-side refusal of ``mp_bottomup_finish_people``
(each case returns before a launch; its pointers are dummy addresses that are never dereferenced) and the argument checks of
``finish_people_batch`` / ``match_by_tag_device``."""
import numpy as np
import pytest
import torch

from mindpose_amd import _lib
from mindpose_amd.engine.inferencer.bottomup_inferencer import refine_missing_joint
from mindpose_amd.utils.match import finish_people_batch, match_by_tag_device
from tests.finish_restated import finish_person_restated, located_tags, map_coord, mean_tag, numpy_sum, score

MP_OK, MP_ERR_NULL, MP_ERR_SHAPE, MP_ERR_UNSUPPORTED, MP_ERR_WORKSPACE = 0, -1, -2, -3, -5
DUMMY = 0x1000  # a non-null address that no refused call reads


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _values(rng, kind, *shape):
    """random-normal values, or values of very different magnitude (2^-20 .. 2^20 with both signs): summation order shows"""
    if kind == "normal":
        return rng.randn(*shape).astype(np.float32)
    return (rng.randn(*shape) * np.exp2(rng.randint(-20, 21, shape))).astype(np.float32)


# ---- (a), (b): the score is numpy's mean of a strided column ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "magnitudes"])
@pytest.mark.parametrize("k", [1, 2, 7, 8, 9, 16, 17, 24, 25, 64])
def test_score_is_numpys_mean_of_the_value_column(k, kind):
    rng = np.random.RandomState(1000 + k)
    for num_tags in (1, 2, 4):
        for _ in range(8):
            person = _values(rng, kind, k, 3 + num_tags)
            column = person[:, 2]  # as the inferencer takes it: a strided view of [K, 3 + L]
            assert k == 1 or not column.flags["C_CONTIGUOUS"]
            want = column.mean()
            assert want.dtype == np.float32
            assert _bits(score(person)) == _bits(want)
    # the order is visible: with values this far apart a sequential sum gives other bits for some row
    if kind == "magnitudes" and k >= 16:
        rows = [_values(rng, kind, k, 4) for _ in range(64)]
        sequential = [np.float32(sum((np.float32(v) for v in r[1:, 2]), np.float32(r[0, 2])) / np.float32(k)) for r in rows]
        assert any(_bits(s) != _bits(score(r)) for s, r in zip(sequential, rows))


# ---- (c): the mean tag is numpy's mean along axis 0 -----------------------------------------------------------------------------
MEAN_CASES = [(17, j) for j in range(1, 18)] + [(64, j) for j in (1, 7, 8, 9, 64)]


@pytest.mark.parametrize("kind", ["normal", "magnitudes"])
@pytest.mark.parametrize("num_tags", [1, 2, 4])
@pytest.mark.parametrize("k,count", MEAN_CASES)
def test_mean_tag_is_numpys_mean_over_the_located_joints(k, count, num_tags, kind):
    rng = np.random.RandomState(100 * k + count + num_tags)
    for _ in range(4):
        tags = _values(rng, kind, count, num_tags)
        got = _bits(mean_tag([list(t) for t in tags]))
        # the three forms the host path takes it in: a list of [L] rows (refine_missing_joint), a slice of the [J_total, L] download
        # (_refine_on_device), the array itself
        padded = np.concatenate([_values(rng, kind, 3, num_tags), tags, _values(rng, kind, 2, num_tags)])
        for want in (np.mean([t for t in tags], axis=0), np.mean(padded[3:3 + count], axis=0), np.mean(tags, axis=0)):
            assert want.dtype == np.float32 and want.shape == (num_tags,)
            assert np.array_equal(got, _bits(want))


def test_numpy_sum_switches_at_eight_values():
    a = [np.float32(v) for v in (1e8, 1.0, -1e8, 1.0, 1.0, 1.0, 1.0, 1.0)]
    assert numpy_sum(a[:7]) == np.asarray(a[:7]).sum() == 4.0  # sequential: the first 1.0 is absorbed by 1e8, the other four count
    # eight accumulators: (1e8 + 1) + (-1e8 + 1) absorbs two of the ones; a sequential sum of the eight would give 5.0
    assert numpy_sum(a) == np.asarray(a).sum() == 4.0


# ---- (d), (e): where the tags are read ------------------------------------------------------------------------------------------
def test_map_coord_truncates_then_clamps():
    values = [0.0, 0.25, 0.75, 3.25, 3.75, 15.0, 15.75, 16.0, 99.5, -0.25, -0.75, -1.0, -1.5, -7.25, 1e9, -1e9]
    want = np.clip(np.asarray(values, np.float32).astype(np.int32), 0, 15)
    assert [map_coord(np.float32(v), 16) for v in values] == want.tolist()
    assert map_coord(np.float32("nan"), 16) == 0 and map_coord(np.float32("inf"), 16) == 15 and map_coord(np.float32("-inf"), 16) == 0


def _maps(rng, k, ktag, h, w, num_tags):
    return (rng.randint(-1024, 1024, (k, h, w)) / 1024.0).astype(np.float32), (rng.randint(-4096, 4096, (ktag, h, w, num_tags)) / 1024.0).astype(np.float32)


def _person(rng, k, h, w, num_tags, located):
    person = np.zeros((k, 3 + num_tags), np.float32)
    joints = rng.permutation(k)[:located]
    person[joints, 0] = rng.randint(0, w, located) + 0.25
    person[joints, 1] = rng.randint(0, h, located) + 0.75
    person[joints, 2] = rng.rand(located).astype(np.float32) + 0.125
    person[joints, 3:] = rng.randn(located, num_tags)
    return person


# ---- (f), (g): the whole person against the host function -----------------------------------------------------------------------
@pytest.mark.parametrize("k,num_tags,tag_per_joint,h,w", [(5, 1, True, 6, 9), (5, 2, True, 7, 5), (4, 4, True, 5, 6), (5, 1, False, 6, 7)])
def test_restated_person_equals_the_host_functions(k, num_tags, tag_per_joint, h, w):
    rng = np.random.RandomState(k + num_tags + h)
    heat, tagging = _maps(rng, k, k if tag_per_joint else 1, h, w, num_tags)
    heat[1] = -np.abs(heat[1])            # joint 1: no value > 0 - found, never filled
    heat[2, 0, 0] = heat[2, h - 1, w - 1] = 1.5  # joint 2: two equal maxima in opposite corners (the tag term moves them apart or not)
    filled = 0
    for located in (1, 2, k - 1, k):
        person = _person(rng, k, h, w, num_tags, located)
        want_score = person[:, 2].mean()
        broadcast = tagging if tag_per_joint else np.broadcast_to(tagging, (k,) + tagging.shape[1:])
        want = refine_missing_joint(heat, broadcast, person.copy())
        got_score, got = finish_person_restated(person, heat, tagging, refine=True)
        assert _bits(got_score) == _bits(want_score)
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(got[:, 3:], person[:, 3:])  # the fill rule writes x, y, value only
        assert (got[1, 2] == 0) == (person[1, 2] == 0)
        filled += int(((got[:, 2] != 0) & (person[:, 2] == 0)).sum())
        plain_score, plain = finish_person_restated(person, heat, tagging, refine=False)
        assert _bits(plain_score) == _bits(want_score) and np.array_equal(_bits(plain), _bits(person))
    assert filled > 0
    nobody = np.zeros((k, 3 + num_tags), np.float32)  # no located joint: no mean tag, nothing filled
    assert located_tags(nobody, tagging) == [] and np.array_equal(finish_person_restated(nobody, heat, tagging, True)[1], nobody)


# ---- the entry refuses on the host ----------------------------------------------------------------------------------------------
K, M, H, W, L = 17, 30, 16, 16, 1


def _call(n=1, k=K, m=M, h=H, w=W, tag_per_joint=1, num_tags=L, refine=1, ws_bytes=None, **null):
    lib = _lib.load()
    ptr = {name: None if name in null else DUMMY for name in ("people", "counts", "status", "heatmap", "tagging", "scores", "workspace")}
    if ws_bytes is None:
        ws_bytes = 1 << 30
    return lib.mp_bottomup_finish_people(ptr["people"], ptr["counts"], ptr["status"], ptr["heatmap"], ptr["tagging"], n, k, m, h, w,
                                         tag_per_joint, num_tags, refine, ptr["scores"], ptr["workspace"], ws_bytes, None)


REFUSALS = {
    "null_people": (dict(people=True), MP_ERR_NULL),
    "null_counts": (dict(counts=True), MP_ERR_NULL),
    "null_status": (dict(status=True), MP_ERR_NULL),
    "null_heatmap": (dict(heatmap=True), MP_ERR_NULL),
    "null_tagging": (dict(tagging=True), MP_ERR_NULL),
    "null_scores": (dict(scores=True), MP_ERR_NULL),
    "negative_n": (dict(n=-1), MP_ERR_SHAPE),
    "n_beyond_the_grid": (dict(n=65536), MP_ERR_SHAPE),
    "k_zero": (dict(k=0), MP_ERR_SHAPE),
    "m_negative": (dict(m=-3), MP_ERR_SHAPE),
    "h_zero": (dict(h=0), MP_ERR_SHAPE),
    "w_negative": (dict(w=-1), MP_ERR_SHAPE),
    "no_tags": (dict(num_tags=0), MP_ERR_SHAPE),
    "map_of_2_31_pixels": (dict(h=1 << 16, w=1 << 15), MP_ERR_SHAPE),
    "k_65": (dict(k=65, m=1), MP_ERR_UNSUPPORTED),
    "m_65": (dict(k=1, m=65), MP_ERR_UNSUPPORTED),
    "five_tags": (dict(num_tags=5), MP_ERR_UNSUPPORTED),
    "groups_beyond_1024": (dict(k=64, m=64), MP_ERR_UNSUPPORTED),
    "null_workspace": (dict(workspace=True), MP_ERR_WORKSPACE),
    "short_workspace": (dict(ws_bytes=K * M * (L + 1) * 4 - 4), MP_ERR_WORKSPACE),
    "short_workspace_without_refine": (dict(ws_bytes=0, refine=0), MP_ERR_WORKSPACE),
    "no_image_is_no_launch": (dict(n=0), MP_OK),
    "no_image_reads_no_pointer": (dict(n=0, people=True, scores=True, workspace=True), MP_OK),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_finish_entry_refuses_on_the_host(name):
    kwargs, code = REFUSALS[name]
    assert _call(**kwargs) == code


def test_finish_workspace_bytes():
    lib = _lib.load()
    assert lib.mp_bottomup_finish_workspace_bytes(1, K, M, L) == K * M * (L + 1) * 4
    assert lib.mp_bottomup_finish_workspace_bytes(3, 5, 7, 4) == 3 * 5 * 7 * 5 * 4
    assert lib.mp_bottomup_finish_workspace_bytes(0, K, M, L) == 0 and lib.mp_bottomup_finish_workspace_bytes(1, 64, 64, 1) == 0
    assert "mp_bottomup_finish_people" in _lib.EXPORTED_SYMBOLS and "mp_bottomup_finish_workspace_bytes" in _lib.EXPORTED_SYMBOLS


# ---- the Python entries check before they touch the device ----------------------------------------------------------------------
def _cpu_args(n=2, k=5, m=3, h=8, w=8, num_tags=1, ktag=None):
    return dict(people=torch.zeros(n, k * m, k, 3 + num_tags), counts=torch.zeros(n, dtype=torch.int32), status=torch.zeros(n, dtype=torch.int32),
                heatmap=torch.zeros(n, k, h, w), tagging=torch.zeros(n, k if ktag is None else ktag, h, w, num_tags), refine=True,
                host_match=lambda i: pytest.fail("no image may be grouped"))


def test_finish_people_batch_refuses_cpu_tensors():
    with pytest.raises(_lib.MindposeHipError):
        finish_people_batch(**_cpu_args())


@pytest.mark.parametrize("change", [
    dict(people=torch.zeros(2, 15, 5, 3)),                  # no tag column
    dict(people=torch.zeros(2, 14, 5, 4)),                  # the capacity is no multiple of K
    dict(people=torch.zeros(2, 15, 20)),                    # three axes
    dict(counts=torch.zeros(3, dtype=torch.int32)),
    dict(status=torch.zeros(2, 1, dtype=torch.int32)),
    dict(heatmap=torch.zeros(2, 4, 8, 8)),                  # another K
    dict(heatmap=torch.zeros(1, 5, 8, 8)),                  # another N
    dict(tagging=torch.zeros(2, 5, 8, 9, 1)),               # another map
    dict(tagging=torch.zeros(2, 2, 8, 8, 1)),               # neither K nor one tag channel
    dict(tagging=torch.zeros(2, 5, 8, 8, 2)),               # another L
    dict(tagging=torch.zeros(2, 5, 8, 8)),
], ids=lambda c: next(iter(c)))
def test_finish_people_batch_refuses_wrong_shapes(change):
    with pytest.raises(ValueError):
        finish_people_batch(**dict(_cpu_args(), **change))


def test_finish_people_batch_refuses_what_is_no_tensor():
    with pytest.raises(TypeError):
        finish_people_batch(**dict(_cpu_args(), people=np.zeros((2, 15, 5, 4), np.float32)))


def test_match_by_tag_device_refuses_cpu_tensors():
    val, tag, ind = torch.zeros(1, 5, 3), torch.zeros(1, 5, 3, 1), torch.zeros(1, 5, 3, 2)
    with pytest.raises(_lib.MindposeHipError):
        match_by_tag_device(val, tag, ind, list(range(5)))
