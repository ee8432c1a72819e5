"""The device grouping (``mp_bottomup_match_by_tag`` / ``match_by_tag_batch``) on the MI355X: bit-equal to the reference's recorded
outputs and to the host ``match_by_tag`` on seeded cases that reach every branch of the kernel, nothing written beyond the counted
persons, the NaN hand-over to the host function, the entry's error codes, and the inferencer with the device path on and off."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.engine.inferencer import bottomup_inferencer  # noqa: E402
from mindpose_amd.utils.match import match_by_tag, match_by_tag_batch  # noqa: E402
from tests.golden_io import load_npz  # noqa: E402

DEV = torch.device("cuda:0")
COCO_ORDER = [0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16]
FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]


def _assert_same(got, want, what=""):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


def _host(val, tag, ind, order, **kwargs):
    return [match_by_tag(v, t, i, list(order), **kwargs) for v, t, i in zip(val, tag, ind)]


def _launch(val, tag, ind, order, vis_thr=0.1, tag_thr=1.0, ignore_too_much=False, use_rounded_norm=True):
    """The entry itself on numpy [N, ...] inputs with a NaN-prefilled ``people``: (persons per image, counts, status, people)."""
    lib = _lib.load()
    n, k, m = val.shape
    num_tags = tag.shape[3]
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in (val, tag, ind)]
    people = torch.full((n, k * m, k, 3 + num_tags), float("nan"), device=DEV)
    counts = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    ws_bytes = lib.mp_bottomup_match_workspace_bytes(n, k, m, num_tags)
    assert ws_bytes == n * k * k * m * num_tags * 4
    ws = torch.empty(ws_bytes // 4, device=DEV)
    order_c = (ctypes.c_int * k)(*[int(j) for j in order])
    rc = lib.mp_bottomup_match_by_tag(*[_lib.ptr(t) for t in dev], n, k, m, num_tags, order_c, vis_thr, tag_thr, int(ignore_too_much),
                                      int(use_rounded_norm), _lib.ptr(people), _lib.ptr(counts), _lib.ptr(status), _lib.ptr(ws), ws_bytes,
                                      _lib.stream())
    assert rc == 0
    counts, status, people = counts.cpu().numpy(), status.cpu().numpy(), people.cpu().numpy()
    persons = [people[i, :counts[i]].copy() if counts[i] else np.array([]).astype(np.float32) for i in range(n)]
    return persons, counts, status, people


def _check(val, tag, ind, order, **kwargs):
    """One launch against the host function image by image: bit-equal persons, no fall-back, nothing beyond the counted persons."""
    want = _host(val, tag, ind, order, **kwargs)
    got, counts, status, people = _launch(val, tag, ind, order, **kwargs)
    assert (status == 0).all(), status
    for i, (g, w) in enumerate(zip(got, want)):
        assert counts[i] == (w.shape[0] if w.ndim == 3 else 0)
        _assert_same(g, w, f"image {i}")
        assert not np.isnan(people[i, :counts[i]]).any() and np.isnan(people[i, counts[i]:]).all()
    return want


def _random(seed, n, k, m, num_tags, centres, scale=1.0, noise=(-0.5, 0.0, 0.5), p_visible=0.8):
    """Detections drawn around ``centres`` person tags per image: tag = scale * centre + a noise step (half-integers by default:
    ties in the rounded costs), value above 0.3 with probability ``p_visible``."""
    rng = np.random.RandomState(seed)
    centre = rng.randint(0, centres, (n, k, m, 1)) * np.ones((1, 1, 1, num_tags))
    tag = (scale * centre + rng.choice(noise, (n, k, m, num_tags))).astype(np.float32)
    val = np.where(rng.rand(n, k, m) < p_visible, 0.3 + 0.7 * rng.rand(n, k, m), 0.05 * rng.rand(n, k, m)).astype(np.float32)
    ind = (rng.randint(0, 256, (n, k, m, 2)) + rng.choice([-0.25, 0.0, 0.25], (n, k, m, 2))).astype(np.float32)
    return val, tag, ind


# ---- the reference's recorded outputs ------------------------------------------------------------------------------------------
def test_golden_cases_bit_equal_in_batches():
    z = load_npz("match_by_tag.npz")
    count = int(z["count"])
    assert count >= 60
    batches = {}
    for i in range(count):
        key = (z[f"c{i}_val"].shape, z[f"c{i}_tag"].shape[2], tuple(z[f"c{i}_args"].tolist()), tuple(int(j) for j in z[f"c{i}_order"]))
        batches.setdefault(key, []).append(i)
    assert any(len(cases) > 1 for cases in batches.values())
    for (_, _, (vis_thr, tag_thr, ignore, rounded), order), cases in batches.items():
        val, tag, ind = (torch.from_numpy(np.stack([z[f"c{i}_{name}"] for i in cases]).astype(np.float32)).to(DEV)
                         for name in ("val", "tag", "ind"))
        got = match_by_tag_batch(val, tag, ind, list(order), vis_thr=float(vis_thr), tag_thr=float(tag_thr), ignore_too_much=bool(ignore),
                                 use_rounded_norm=bool(rounded))
        assert len(got) == len(cases)
        for g, i in zip(got, cases):
            _assert_same(g, z[f"c{i}_out"], f"case {i}")


# ---- a batch of different images ----------------------------------------------------------------------------------------------------
def test_five_images_one_launch_writes_only_the_counted_persons():
    val, tag, ind = _random(1, 5, 17, 12, 1, centres=6)
    val[2] *= 0.1    # image 2: nothing above vis_thr
    val[3, :, 4:] = 0.0
    want = _check(val, tag, ind, COCO_ORDER, vis_thr=0.1)
    assert want[2].shape == (0,) and len({w.shape[0] for w in want}) >= 3  # the images differ
    got = match_by_tag_batch(*[torch.from_numpy(a).to(DEV) for a in (val, tag, ind)], COCO_ORDER, vis_thr=0.1)
    for i in range(5):
        _assert_same(got[i], want[i], f"image {i}")
    # the cached buffers of a shape serve a second, different batch
    val2, tag2, ind2 = _random(2, 5, 17, 12, 1, centres=3)
    for g, w in zip(match_by_tag_batch(*[torch.from_numpy(a).to(DEV) for a in (val2, tag2, ind2)], COCO_ORDER),
                    _host(val2, tag2, ind2, COCO_ORDER)):
        _assert_same(g, w)


# ---- seeded cases against the host function, at the smallest shapes that reach each branch -----------------------------------------
def test_recipe_shape_half_integer_tags_reaches_the_pairwise_mean():
    val, tag, ind = _random(3, 3, 17, 30, 1, centres=8, p_visible=0.6)
    want = _check(val, tag, ind, COCO_ORDER)
    # persons located at more than nine joints: tag lists of n >= 8 are likely here (test_pairwise_mean_decides_a_threshold is the
    # direct check of the eight-accumulator form)
    assert max(int((w[:, :, 2] > 0).sum(axis=1).max()) for w in want) > 9


def _pairwise_case(n, joins):
    """K = 17, M = 1, L = 1: joints 0 .. n - 1 carry tags near 300 that all join one group (its list grows to n), joint n carries a tag
    EXACTLY 1.0 above the smaller of the list's pairwise mean (numpy's, n >= 8) and its sequential mean, which differ in the last bit:
    with tag_thr = 1 the detection joins the group under one summation order and opens a second group under the other; ``joins``: which
    of the two numpy's order gives."""
    f = np.float32
    for seed in range(1000):
        tags = (300.0 + np.random.RandomState(seed).uniform(-0.3, 0.3, n)).astype(np.float32)
        pairwise = np.mean(np.stack([t[None] for t in tags]), axis=0)[0]
        total = tags[0]
        for t in tags[1:]:
            total = f(total + t)
        sequential = f(total / f(n))
        low, high = min(pairwise, sequential), max(pairwise, sequential)
        probe = f(low + f(1.0))
        if pairwise != sequential and f(probe - low) == f(1.0) and f(probe - high) < f(1.0) and (pairwise == high) == joins:
            break
    else:
        raise AssertionError("no seed separates the two sums")
    val, tag = np.zeros((17, 1), np.float32), np.zeros((17, 1, 1), np.float32)
    val[:n + 1], tag[:n, 0, 0], tag[n, 0, 0] = 0.9, tags, probe
    ind = np.arange(34, dtype=np.float32).reshape(17, 1, 2)
    assert bool(f(probe - pairwise) < f(1.0)) == joins != bool(f(probe - sequential) < f(1.0))  # numpy's order decides
    return val, tag, ind


def test_pairwise_mean_decides_a_threshold():
    shapes = ((8, False), (11, True), (16, False))  # one block of eight; a tail of three; two blocks
    cases = [_pairwise_case(n, joins) for n, joins in shapes]
    val, tag, ind = (np.stack([c[i] for c in cases]) for i in range(3))
    want = _check(val, tag, ind, list(range(17)))
    for w, (n, joins) in zip(want, shapes):
        assert w.shape[0] == (1 if joins else 2) and int((w[0, :, 2] > 0).sum()) == n + int(joins)  # the list did reach n tags


@pytest.mark.parametrize("num_tags", [2, 3, 4])
def test_more_tags(num_tags):
    val, tag, ind = _random(10 + num_tags, 3, 9, 8, num_tags, centres=5, noise=(-0.5, -0.25, 0.0, 0.25, 0.5))
    _check(val, tag, ind, list(range(9)))
    _check(val, tag, ind, list(range(9)), tag_thr=0.6, use_rounded_norm=False)


def test_spread_tags_more_groups_than_lanes():
    # 400 centres ten apart: most detections open a group of their own - beyond 64 columns (one pass of the lanes) after three
    # joints and beyond 256 after nine, with n_groups >> n_new - and some still meet their centre's group
    val, tag, ind = _random(5, 2, 17, 30, 1, centres=400, scale=10.0, p_visible=0.9)
    want = _check(val, tag, ind, COCO_ORDER)
    assert min(w.shape[0] for w in want) > 256 and max(int((w[:, :, 2] > 0).sum(axis=1).max()) for w in want) > 1
    val, tag, ind = _random(6, 2, 6, 30, 2, centres=60, scale=10.0, p_visible=0.9)
    want = _check(val, tag, ind, list(range(6)))
    assert min(w.shape[0] for w in want) > 64


def test_more_detections_than_groups_gives_dummy_columns():
    val, tag, ind = _random(7, 3, 17, 10, 1, centres=12)
    val[:, 0, 2:] = 0.0  # the first joint opens two groups, the next ones bring up to ten detections: n_new > n_groups
    val[:, 0, :2] = 0.9
    _check(val, tag, ind, list(range(17)))
    _check(val, tag, ind, list(range(17)), tag_thr=0.5)


def test_ignore_too_much():
    val, tag, ind = _random(8, 4, 17, 3, 1, centres=4, p_visible=0.7)
    want = _check(val, tag, ind, COCO_ORDER, ignore_too_much=True)
    other = _host(val, tag, ind, COCO_ORDER, ignore_too_much=False)
    assert any(w.shape != o.shape or not np.array_equal(w, o) for w, o in zip(want, other))  # the switch did skip steps


def test_unrounded_costs_permuted_order_single_joint_single_detection():
    val, tag, ind = _random(9, 3, 17, 10, 1, centres=6, noise=(-0.4, -0.15, 0.0, 0.3, 0.45))
    _check(val, tag, ind, COCO_ORDER, use_rounded_norm=False)
    order = np.random.RandomState(0).permutation(17).tolist()
    want = _check(val, tag, ind, order)
    assert any(w.shape != o.shape or not np.array_equal(w, o) for w, o in zip(want, _host(val, tag, ind, COCO_ORDER)))
    val, tag, ind = _random(10, 3, 1, 30, 2, centres=5)  # K = 1: only the opening step, with key collisions inside it
    _check(val, tag, ind, [0])
    val, tag, ind = _random(11, 4, 17, 1, 1, centres=2)  # M = 1: one row, one or more columns
    _check(val, tag, ind, COCO_ORDER)


# ---- NaN tags go to the host function ------------------------------------------------------------------------------------------
def test_nan_tag_sets_the_status_and_leaves_the_other_images_alone():
    val, tag, ind = _random(12, 3, 17, 8, 1, centres=4)
    clean = _host(val, tag, ind, COCO_ORDER)
    tag[1, 5, 2, 0] = np.nan
    val[1, 5, 2] = 0.9     # a visible detection
    tag[2, 3, 1, 0] = np.inf
    val[2, 3, 1] = 0.01    # an invisible one: no concern of anybody
    got, counts, status, _ = _launch(val, tag, ind, COCO_ORDER)
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    _assert_same(got[0], clean[0])
    _assert_same(got[2], clean[2])
    try:
        want = match_by_tag(val[1], tag[1], ind[1], COCO_ORDER)
    except Exception as e:  # whatever the host function raises for this image, the batch form raises too
        with pytest.raises(type(e)):
            match_by_tag_batch(*[torch.from_numpy(a).to(DEV) for a in (val, tag, ind)], COCO_ORDER)
    else:
        _assert_same(match_by_tag_batch(*[torch.from_numpy(a).to(DEV) for a in (val, tag, ind)], COCO_ORDER)[1], want)
    ok = match_by_tag_batch(*[torch.from_numpy(a[[0, 2]]).to(DEV) for a in (val, tag, ind)], COCO_ORDER)
    _assert_same(ok[0], clean[0])
    _assert_same(ok[1], clean[2])


@pytest.mark.filterwarnings("ignore:overflow encountered")  # numpy says so when the host function squares the difference
def test_overflowing_distance_hands_the_image_over():
    """Finite tags 3e19 apart: the squared difference overflows float32, the distance is inf - status 2, found in the scan after the
    first joint's persons were written; the batch form gives what the host function gives for that image."""
    val, tag, ind = _random(13, 3, 3, 2, 1, centres=3)
    clean = _host(val, tag, ind, [0, 1, 2])
    val[1], tag[1, :, 0, 0], tag[1, :, 1, 0] = 0.9, 0.0, 3e19
    got, counts, status, _ = _launch(val, tag, ind, [0, 1, 2])
    assert status.tolist() == [0, 2, 0] and counts[1] == 0
    _assert_same(got[0], clean[0])
    _assert_same(got[2], clean[2])
    batch = [torch.from_numpy(a).to(DEV) for a in (val, tag, ind)]
    try:
        want = match_by_tag(val[1], tag[1], ind[1], [0, 1, 2])
    except Exception as e:
        with pytest.raises(type(e)):
            match_by_tag_batch(*batch, [0, 1, 2])
    else:
        both = match_by_tag_batch(*batch, [0, 1, 2])
        _assert_same(both[1], want)
        _assert_same(both[0], clean[0])
        _assert_same(both[2], clean[2])


# ---- the entry refuses before any launch ----------------------------------------------------------------------------------------
def test_error_codes():
    lib = _lib.load()
    k, m, num_tags = 17, 30, 1
    val, tag, ind = (torch.zeros(1, k, m, *tail, device=DEV) for tail in ((), (num_tags,), (2,)))
    people = torch.full((1, k * m, k, 3 + num_tags), float("nan"), device=DEV)
    counts, status = torch.full((1,), -7, dtype=torch.int32, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws_bytes = lib.mp_bottomup_match_workspace_bytes(1, k, m, num_tags)
    ws = torch.empty(ws_bytes // 4, device=DEV)

    def call(n=1, k=k, m=m, num_tags=num_tags, order=None, ws_bytes=ws_bytes, **null):
        ptrs = {name: None if name in null else _lib.ptr(t) for name, t in
                dict(val=val, tag=tag, ind=ind, people=people, counts=counts, status=status, ws=ws).items()}
        order = list(range(k)) if order is None else order
        order_c = None if "joint_order" in null else (ctypes.c_int * len(order))(*order)
        return lib.mp_bottomup_match_by_tag(ptrs["val"], ptrs["tag"], ptrs["ind"], n, k, m, num_tags, order_c, 0.1, 1.0, 0, 1, ptrs["people"],
                                            ptrs["counts"], ptrs["status"], ptrs["ws"], ws_bytes, _lib.stream())

    for name in ("val", "tag", "ind", "people", "counts", "status", "joint_order"):
        assert call(**{name: True}) == -1, name
    assert call(k=0) == -2 and call(m=-1) == -2 and call(num_tags=0) == -2 and call(n=-1) == -2
    assert call(k=65) == -3 and call(m=65) == -3 and call(num_tags=5) == -3
    assert call(k=64, m=64) == -3  # inside each limit, beyond the group bound the LDS carries
    assert lib.mp_bottomup_match_supported(17, 30, 1) == 1 and lib.mp_bottomup_match_supported(17, 30, 4) == 1  # the recipe's 510 groups
    assert lib.mp_bottomup_match_supported(65, 1, 1) == 0 and lib.mp_bottomup_match_supported(64, 64, 1) == 0
    assert call(order=[0] * k) == -2 and call(order=list(range(1, k + 1))) == -2 and call(order=[-1] + list(range(1, k))) == -2
    assert call(ws_bytes=ws_bytes - 4) == -5 and call(ws=True) == -5
    assert call(n=0) == 0 and call(n=0, val=True, people=True, joint_order=True) == 0
    torch.cuda.synchronize()
    assert torch.isnan(people).all() and int(counts[0]) == -7 and int(status[0]) == -7  # none of the calls above launched
    assert call() == 0
    torch.cuda.synchronize()
    assert int(counts[0]) == 0 and int(status[0]) == 0 and torch.isnan(people).all()  # all values are 0: nothing visible
    assert match_by_tag_batch(val[:0], tag[:0], ind[:0], list(range(k))) == []
    with pytest.raises(ValueError):
        match_by_tag_batch(val, tag, ind, [0] * k)
    with pytest.raises(_lib.MindposeHipError):
        match_by_tag_batch(val.cpu(), tag.cpu(), ind.cpu(), list(range(k)))  # CPU tensors: the batch form has no fallback


# ---- the inferencer ------------------------------------------------------------------------------------------------------------
def test_inferencer_records_do_not_depend_on_the_switch(monkeypatch):
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")  # the library's own choice of kernel per layer: no candidate timing in this test
    h, w = 256, 192
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    eval_net = mp.create_eval_network(net, dec)
    base = dict(has_heatmap_output=True, hflip_tta=False, joint_order=COCO_ORDER, vis_thr=0.1, ignore_too_much=False, use_rounded_norm=True,
                tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=True, flip_pairs=FLIP_PAIRS)
    gen = torch.Generator().manual_seed(17)
    batch = dict(image=torch.randn(2, 3, h, w, generator=gen).to(DEV), mask=torch.ones(2, h, w, dtype=torch.bool, device=DEV),
                 center=np.array([[w / 2, h / 2]] * 2, np.float32), scale=np.array([[w / 200.0, h / 200.0]] * 2, np.float32),
                 image_shape=np.array([[h, w]] * 2, np.float32), image_file=np.array(["a.jpg", "b.jpg"]))
    calls = []
    original = bottomup_inferencer.match_by_tag_batch
    monkeypatch.setattr(bottomup_inferencer, "match_by_tag_batch", lambda *a, **k: (calls.append(1), original(*a, **k))[1])
    for cfg in (base, dict(base, refine_missing_joint=False), dict(base, hflip_tta=True)):
        inf = mp.create_inferencer(eval_net, "bottomup_heatmap_ae", config=cfg, decoder=dec)
        monkeypatch.setenv("MINDPOSE_MATCH_DEVICE", "1")
        device = inf.infer([batch])
        assert len(calls) == 1
        monkeypatch.setenv("MINDPOSE_MATCH_DEVICE", "0")
        host = inf.infer([batch])
        assert len(calls) == 1  # the switch keeps the batch on the host function
        calls.clear()
        assert len(device) == len(host) == 2 and len(device[0]["pred"]) > 0
        assert device[0]["pred"].shape[2] == (5 if cfg["hflip_tta"] else 4)  # the flip test doubles the tags: L = 2
        for d, q in zip(device, host):
            assert d["pred"].dtype == q["pred"].dtype and d["pred"].shape == q["pred"].shape
            assert np.array_equal(d["pred"], q["pred"])
            assert d["score"] == q["score"] and d["image_path"] == q["image_path"]
