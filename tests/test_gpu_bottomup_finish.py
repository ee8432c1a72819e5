"""The device tail of a bottom-up batch on the MI355X (``mp_bottomup_finish_people``, ``finish_people_batch``,
``match_by_tag_device``, ``MINDPOSE_FINISH_DEVICE``): bit for bit against the host path - ``match_by_tag``, the host score expression
``person[:, 2].mean()`` and ``refine_missing_joint`` on downloaded maps - on small maps that reach every rule of the refinement,
nothing read or written beyond the counted persons, the hand-over of an image to the host function, the inferencer's records with
the switch on and off, its downloads, and the old refinement entry unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.engine.inferencer import bottomup_inferencer  # noqa: E402
from mindpose_amd.engine.inferencer.bottomup_inferencer import refine_missing_joint  # noqa: E402
from mindpose_amd.utils import match as match_module  # noqa: E402
from mindpose_amd.utils.match import finish_people_batch, host_match_of, match_by_tag, match_by_tag_device  # noqa: E402
from tests.finish_restated import finish_person_restated  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 64          # words behind every buffer the entry writes
SENTINEL = 12345.0  # what they hold
CORNERS = ((0, 0), (0, -1), (-1, 0), (-1, -1))  # (row, column)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    assert np.array_equal(_bits(got), _bits(want)), what


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _maps(seed, kind, n, k, ktag, h, w, num_tags):
    """heat [n, k, h, w] and tagging [n, ktag, h, w, L] (numpy): multiples of 1 / 1024, or random normal.  With k >= 5 the maps carry
    the refinement's edge cases: joint 1 has no value > 0 (found, never filled), joints 2 and 3 of image i have their winner in
    corners 2i and 2i + 1 (mod 4; far above any tag distance: the clamped neighbours decide the shifts) and joint 4 has the same
    score at two pixels (equal values, equal tags: the lower flat index wins)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "dyadic":
        heat = torch.randint(-1024, 1024, (n, k, h, w), generator=gen).float() / 1024.0
        tagging = torch.randint(-4096, 4096, (n, ktag, h, w, num_tags), generator=gen).float() / 1024.0
    else:
        heat, tagging = torch.randn(n, k, h, w, generator=gen), 2.0 * torch.randn(n, ktag, h, w, num_tags, generator=gen)
    heat, tagging = heat.numpy(), tagging.numpy()
    ties = []
    if k >= 5:
        heat[:, 1] = -np.abs(heat[:, 1])
        for i in range(n):
            for joint, corner in ((2, CORNERS[(2 * i) % 4]), (3, CORNERS[(2 * i + 1) % 4])):
                heat[i, joint][corner] = 64.0
            first, second = (h // 3, w - 2), (h - 2, 1)
            heat[i, 4][first] = heat[i, 4][second] = 48.0
            tagging[i, 4 if ktag > 1 else 0][second] = tagging[i, 4 if ktag > 1 else 0][first]
            ties.append((first, second))
    return heat, tagging, ties


def _persons(seed, n, k, h, w, num_tags, per_image, located_counts):
    """[P_i, k, 3 + L] per image, as the grouping leaves them: ``located_counts`` (cycled) located joints - value > 0, coordinates off
    the integer grid as the decoder's +-0.25 shift leaves them, the detection's own tags - the others all zero."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        people = np.zeros((per_image[i], k, 3 + num_tags), np.float32)
        for p in range(per_image[i]):
            count = min(located_counts[(i * 7 + p) % len(located_counts)], k)
            joints = rng.permutation(k)[:count]
            people[p, joints, 0] = rng.randint(0, w, count) + rng.choice([-0.25, 0.25], count)
            people[p, joints, 1] = rng.randint(0, h, count) + rng.choice([-0.25, 0.25], count)
            people[p, joints, 2] = (0.125 + rng.rand(count) * np.exp2(rng.randint(-6, 3, count))).astype(np.float32)
            people[p, joints, 3:] = rng.randn(count, num_tags)
        out.append(people if per_image[i] else np.array([]).astype(np.float32))
    return out


def _host_path(persons, heat, tagging, refine):
    """(keypoints, scores) of the host path: the score expression, then refine_missing_joint person by person on host maps."""
    k = heat.shape[1]
    full = tagging if tagging.shape[1] == k else np.broadcast_to(tagging, (tagging.shape[0], k) + tagging.shape[2:])
    keypoints = [p.copy() for p in persons]
    scores = [[person[:, 2].mean() for person in people] for people in keypoints]
    if refine:
        for i in range(len(keypoints)):
            for p in range(len(keypoints[i])):
                keypoints[i][p] = refine_missing_joint(heat[i], full[i], keypoints[i][p])
    return keypoints, scores


def _guarded(words, dtype=torch.float32, fill=float("nan")):
    """(the buffer of ``words`` elements prefilled with ``fill``, the allocation it is the front of: GUARD sentinel words behind it)"""
    whole = torch.full((words + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    whole[:words] = fill
    return whole[:words], whole


def _guard_intact(whole):
    return bool((whole[-GUARD:] == SENTINEL).all())


def _run_entry(persons, heat, tagging, m, refine, status=None, finite=True):
    """The C entry on ``persons`` laid out as the grouping entry leaves them - NaN behind the counted rows of ``people``, NaN in all
    of ``scores`` - with sentinel words behind ``people``, ``scores`` and the workspace.  Checks what may not be touched; returns
    (keypoints, scores) of the counted persons."""
    lib = _lib.load()
    n, k, h, w = heat.shape
    ktag, num_tags = tagging.shape[1], tagging.shape[4]
    groups, width = k * m, 3 + num_tags
    counts = [len(p) for p in persons]
    assert max(counts) <= groups
    people, people_whole = _guarded(n * groups * k * width)
    people = people.view(n, groups, k, width)
    for i, p in enumerate(persons):
        if counts[i]:
            people[i, :counts[i]] = torch.from_numpy(p).to(DEV)
    before = people.cpu().numpy().copy()
    scores, scores_whole = _guarded(n * groups)
    ws_bytes = lib.mp_bottomup_finish_workspace_bytes(n, k, m, num_tags)
    assert ws_bytes == n * groups * (num_tags + 1) * 4
    ws, ws_whole = _guarded(ws_bytes // 4)
    counts_dev = torch.tensor(counts, dtype=torch.int32, device=DEV)
    status_dev = torch.tensor(status if status is not None else [0] * n, dtype=torch.int32, device=DEV)
    heat_dev, tagging_dev = torch.from_numpy(heat).to(DEV), torch.from_numpy(tagging).to(DEV)
    rc = lib.mp_bottomup_finish_people(_lib.ptr(people), _lib.ptr(counts_dev), _lib.ptr(status_dev), _lib.ptr(heat_dev), _lib.ptr(tagging_dev),
                                       n, k, m, h, w, int(ktag > 1 or k == 1), num_tags, int(refine), _lib.ptr(scores), _lib.ptr(ws), ws_bytes,
                                       _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _guard_intact(people_whole) and _guard_intact(scores_whole) and _guard_intact(ws_whole)
    after, got_scores = people.cpu().numpy(), scores.view(n, groups).cpu().numpy()
    keypoints, out_scores = [], []
    for i in range(n):
        live = counts[i] if status is None or status[i] == 0 else 0
        assert np.array_equal(_bits(after[i, live:]), _bits(before[i, live:]))  # rows that do not exist: as they were, bit for bit
        assert np.isnan(got_scores[i, live:]).all()
        assert not finite or (not np.isnan(after[i, :live]).any() and not np.isnan(got_scores[i, :live]).any())
        assert np.array_equal(_bits(after[i, :live, :, 3:]), _bits(before[i, :live, :, 3:]))  # the tags of a person are never written
        keypoints.append(after[i, :live].copy() if live else np.array([]).astype(np.float32))
        out_scores.append(list(got_scores[i, :live]))
    return keypoints, out_scores


def _device_batch(persons, heat, tagging, m, status=None):
    """CUDA (people, counts, status, heatmap, tagging) for finish_people_batch, people NaN behind the counted rows."""
    n, k = heat.shape[:2]
    people = torch.full((n, k * m, k, 3 + tagging.shape[4]), float("nan"), device=DEV)
    for i, p in enumerate(persons):
        if len(p):
            people[i, :len(p)] = torch.from_numpy(p).to(DEV)
    meta = torch.tensor([[len(p) for p in persons], status if status is not None else [0] * n], dtype=torch.int32, device=DEV)
    return people, meta[0], meta[1], torch.from_numpy(heat).to(DEV), torch.from_numpy(tagging).to(DEV)


def _no_host_match(i):
    raise AssertionError(f"image {i} went to the host function")


def _assert_records(got, want, what=""):
    (got_kp, got_scores), (want_kp, want_scores) = got, want
    assert len(got_kp) == len(want_kp) and len(got_scores) == len(want_scores)
    for i, (g, q) in enumerate(zip(got_kp, want_kp)):
        _same(g, q, f"{what} image {i}")
    assert [[type(s) for s in row] for row in got_scores] == [[np.float32] * len(row) for row in want_scores]
    assert [[_bits(s).item() for s in row] for row in got_scores] == [[_bits(s).item() for s in row] for row in want_scores], what


def _assert_case_is_meaningful(persons, want, ties, h, w):
    """What a parametrisation is there for, read from the host path's result: joints are filled, and where the maps carry the edge
    cases (k >= 5) each of them decides a joint."""
    n, k = len(persons), persons[0].shape[1]
    filled = [(i, p, j) for i in range(n) for p in range(len(persons[i])) for j in range(k)
              if persons[i][p][j, 2] == 0 and want[0][i][p][j, 2] != 0]
    if k == 1:  # a person is its one joint: located, or without a mean tag - nothing is ever filled
        assert filled == []
        return
    assert filled  # the case does refine something
    assert any((persons[i][p][:, 2] > 0).sum() == 1 for i, p, _ in filled)   # ... for a person with ONE located joint
    assert any((person[:, 2] > 0).all() for people in persons for person in people)      # ... beside persons with nothing to fill
    if k >= 5:
        missing = lambda j: [(i, p) for i in range(n) for p in range(len(persons[i])) if persons[i][p][j, 2] == 0]  # noqa: E731
        assert missing(1) and all(want[0][i][p][1, 2] == 0 and not want[0][i][p][1, :2].any() for i, p in missing(1))  # best pixel <= 0
        seen = set()
        for joint, offset in ((2, 0), (3, 1)):
            for i, p in missing(joint):
                row, col = CORNERS[(2 * i + offset) % 4]
                row, col = row % h, col % w
                x, y, value = want[0][i][p][joint, :3]
                assert value == 64.0 and (int(x), int(y)) == (col, row)
                assert x - col in (0.25, 0.75) and y - row in (0.25, 0.75)  # centre +- 0.25: inside the corner pixel
                seen.add((row, col))
        assert seen == {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}  # every corner's clamped neighbours were compared
        assert missing(4)
        for i, p in missing(4):
            (first, second), (x, y, value) = ties[i], want[0][i][p][4, :3]
            assert value == 48.0 and (int(y), int(x)) == first and first[0] * w + first[1] < second[0] * w + second[1]


# ---- 1. the entry against the host path ------------------------------------------------------------------------------------------
# (k, L, tag_per_joint, m, h, w): K * M < 128; a map per case of 16 x 16, 24 x 40 (several iterations per thread) and 20 x 33 (odd width,
# no multiple of the workgroup)
CASES = [(17, 1, True, 7, 16, 16), (17, 2, True, 5, 24, 40), (17, 4, True, 3, 20, 33), (5, 1, True, 20, 24, 40), (5, 2, True, 9, 20, 33),
         (5, 4, True, 6, 16, 16), (17, 1, False, 6, 20, 33), (5, 1, False, 25, 16, 16), (1, 1, True, 30, 16, 16), (1, 2, True, 9, 24, 40),
         (1, 4, True, 5, 20, 33)]


@pytest.mark.parametrize("kind", ["dyadic", "normal"])
@pytest.mark.parametrize("k,num_tags,tag_per_joint,m,h,w", CASES)
def test_entry_bit_equal_to_the_host_path(k, num_tags, tag_per_joint, m, h, w, kind):
    seed = 1000 * k + 100 * num_tags + h + (kind == "normal")
    n = 2
    heat, tagging, ties = _maps(seed, kind, n, k, k if tag_per_joint else 1, h, w, num_tags)
    # every joint located (nothing to fill), one located joint, a few, most
    persons = _persons(seed, n, k, h, w, num_tags, per_image=(min(9, k * m), min(6, k * m)), located_counts=(k, 1, 3, 9, 1, k - 1, 2) if k > 1 else (1,))
    want = _host_path(persons, heat, tagging, refine=True)
    _assert_case_is_meaningful(persons, want, ties, h, w)
    got = _run_entry(persons, heat, tagging, m, refine=True)
    _assert_records(got, want, "entry")
    got_python = finish_people_batch(*_device_batch(persons, heat, tagging, m), refine=True, host_match=_no_host_match)
    _assert_records(got_python, want, "finish_people_batch")
    assert all(g.flags["C_CONTIGUOUS"] and g.flags["WRITEABLE"] for g in got_python[0])
    plain = _run_entry(persons, heat, tagging, m, refine=False)
    _assert_records(plain, _host_path(persons, heat, tagging, refine=False), "refine off")



# ---- 2. counts, rows that do not exist, guard words -------------------------------------------------------------------------------
def test_counts_decide_what_is_read_and_written():
    k, num_tags, m, h, w = 17, 1, 7, 20, 33
    heat, tagging, _ = _maps(3, "normal", 4, k, k, h, w, num_tags)
    # an image without persons between two with, and an image that fills its capacity K * M
    persons = _persons(3, 4, k, h, w, num_tags, per_image=(5, 0, 2, k * m), located_counts=(3, 1, k, 9))
    want = _host_path(persons, heat, tagging, refine=True)
    got = _run_entry(persons, heat, tagging, m, refine=True)  # (checks the NaN rows, the NaN scores and the guard words)
    _assert_records(got, want)
    assert got[0][1].shape == (0,) and got[1][1] == [] and len(got[0][3]) == k * m
    # a status word != 0 takes the image out: nothing of it is read or written, whatever its count says
    handed = _run_entry(persons, heat, tagging, m, refine=True, status=[0, 0, 1, 0])
    _assert_records((handed[0][:2] + handed[0][3:], handed[1][:2] + handed[1][3:]), (want[0][:2] + want[0][3:], want[1][:2] + want[1][3:]))
    assert handed[0][2].shape == (0,)


def test_counts_outside_the_capacity_are_clamped():
    """counts[i] below 0 or above K * M (no grouping launch leaves one): clamped, so the grid's last person is the last one read."""
    lib = _lib.load()
    k, num_tags, m, h, w = 5, 1, 3, 16, 16
    heat, tagging, _ = _maps(5, "dyadic", 2, k, k, h, w, num_tags)
    persons = _persons(5, 2, k, h, w, num_tags, per_image=(k * m, k * m), located_counts=(2, 1, k))
    people, _, _, heat_dev, tagging_dev = _device_batch(persons, heat, tagging, m)
    counts = torch.tensor([-4, 1 << 20], dtype=torch.int32, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    scores, scores_whole = _guarded(2 * k * m)
    ws_bytes = lib.mp_bottomup_finish_workspace_bytes(2, k, m, num_tags)
    ws, ws_whole = _guarded(ws_bytes // 4)
    assert lib.mp_bottomup_finish_people(_lib.ptr(people), _lib.ptr(counts), _lib.ptr(status), _lib.ptr(heat_dev), _lib.ptr(tagging_dev), 2, k,
                                         m, h, w, 1, num_tags, 1, _lib.ptr(scores), _lib.ptr(ws), ws_bytes, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert _guard_intact(scores_whole) and _guard_intact(ws_whole)
    want = _host_path(persons, heat, tagging, refine=True)
    got = people.cpu().numpy()
    _same(got[0], persons[0])  # a negative count: no person
    _same(got[1], want[0][1])  # a count beyond the capacity: the capacity
    assert np.isnan(scores.view(2, -1)[0].cpu().numpy()).all()
    assert [_bits(s).item() for s in scores.view(2, -1)[1].cpu().numpy()] == [_bits(s).item() for s in want[1][1]]


def test_coordinates_outside_the_map_read_inside_it():
    """NaN, infinite and far coordinates on located joints (outside the bit-equality contract of the host path, inside the memory
    safety contract): the tag is read at the clamped pixel, as the restatement says."""
    k, num_tags, m, h, w = 5, 2, 3, 16, 16
    heat, tagging, _ = _maps(9, "dyadic", 1, k, k, h, w, num_tags)
    persons = _persons(9, 1, k, h, w, num_tags, per_image=(4,), located_counts=(2, 3, 1, 2))
    bad = [float("nan"), float("inf"), -float("inf"), 3e9, -3e9, -0.75, w + 0.25, 1e5]
    slot = 0
    for person in persons[0]:
        for j in np.flatnonzero(person[:, 2] > 0):
            person[j, 0], person[j, 1] = bad[slot % len(bad)], bad[(slot + 3) % len(bad)]
            slot += 1
    got = _run_entry(persons, heat, tagging, m, refine=True, finite=False)
    for p, person in enumerate(persons[0]):
        want_score, want = finish_person_restated(person, heat[0], tagging[0], refine=True)
        assert np.array_equal(_bits(got[0][0][p]), _bits(want)) and _bits(got[1][0][p]) == _bits(want_score)


# ---- 3. an image handed to the host function --------------------------------------------------------------------------------------
def _detections(seed, n, k, m, num_tags, h, w, centres=3):
    rng = np.random.RandomState(seed)
    tag = (rng.randint(0, centres, (n, k, m, 1)) * 4.0 + 0.25 * rng.randn(n, k, m, num_tags)).astype(np.float32)
    val = np.where(rng.rand(n, k, m) < 0.6, 0.3 + 0.7 * rng.rand(n, k, m), 0.05 * rng.rand(n, k, m)).astype(np.float32)
    ind = np.stack([rng.randint(0, w, (n, k, m)), rng.randint(0, h, (n, k, m))], axis=3) + rng.choice([-0.25, 0.25], (n, k, m, 2))
    return val, tag, ind.astype(np.float32)


def test_nan_tag_hands_one_image_of_three_to_the_host_function(monkeypatch):
    k, m, num_tags, h, w = 17, 6, 1, 24, 40
    order = [0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16]
    val, tag, ind = _detections(11, 3, k, m, num_tags, h, w)
    # the middle image: detections of ONE joint only, so the host function opens a group per detection and never builds a cost
    # matrix from the NaN tag (scipy would raise); the kernel hands the image over all the same (status 1)
    val[1] = 0.0
    val[1, 3, :4] = (0.9, 0.8, 0.7, 0.6)
    tag[1, 3, 1, 0] = np.nan
    heat, tagging, _ = _maps(11, "normal", 3, k, k, h, w, num_tags)
    groups = [match_by_tag(val[i], tag[i], ind[i], order) for i in range(3)]
    assert all(len(g) > 0 for g in groups) and groups[1].shape == (4, k, 4)
    want = _host_path(groups, heat, tagging, refine=True)
    assert any(not np.array_equal(a[:, :, :3], b[:, :, :3]) for a, b in zip(want[0], groups))  # the refinement fills joints

    calls = []
    original = match_module.match_by_tag
    monkeypatch.setattr(match_module, "match_by_tag", lambda *a, **kw: (calls.append(1), original(*a, **kw))[1])
    dev = [torch.from_numpy(a).to(DEV) for a in (val, tag, ind)]
    people, counts, status = match_by_tag_device(*dev, order)
    assert people.is_cuda and counts.is_cuda and status.is_cuda and calls == []
    got = finish_people_batch(people, counts, status, torch.from_numpy(heat).to(DEV), torch.from_numpy(tagging).to(DEV), refine=True,
                              host_match=host_match_of(*dev, order))
    assert len(calls) == 1  # exactly the one image, by construction of the input
    assert status.cpu().tolist() == [0, 1, 0]
    for g, q in zip(got[0], want[0]):  # (the host rows carry the NaN tag: compare bits, not values)
        _same(g, q)
    assert [[_bits(s).item() for s in row] for row in got[1]] == [[_bits(s).item() for s in row] for row in want[1]]
    # refinement off: the same image goes over, nothing is filled
    calls.clear()
    people, counts, status = match_by_tag_device(*dev, order)
    plain = finish_people_batch(people, counts, status, torch.from_numpy(heat).to(DEV), torch.from_numpy(tagging).to(DEV), refine=False,
                                host_match=host_match_of(*dev, order))
    assert len(calls) == 1
    for g, q in zip(plain[0], groups):
        _same(g, q)


# ---- 4., 5. the inferencer ------------------------------------------------------------------------------------------------------
K = 17
FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
FLIP_INDEX = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
INFER_CFG = dict(has_heatmap_output=True, hflip_tta=False, joint_order=[0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16], vis_thr=0.1,
                 ignore_too_much=False, use_rounded_norm=True, tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=True,
                 flip_pairs=FLIP_PAIRS)
MAP_H, MAP_W = 48, 40


def _fake_net(n, flip, seed=5):
    """A network that is its decoder on fixed random stage outputs (spread tags: grouping leaves persons with empty joints), with
    the flip test's doubled tags (L = 2) on request; and one batch for it."""
    gen = torch.Generator().manual_seed(seed)

    def outputs():
        low = torch.rand(n, 2 * K, MAP_H // 2, MAP_W // 2, generator=gen)
        low[:, K:] *= 8.0
        return [low.to(DEV), torch.rand(n, K, MAP_H, MAP_W, generator=gen).to(DEV)]

    outs, mirrored = outputs(), outputs()
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)

    def net(image, mask):
        return (dec.decode_flip_aggregated(outs, mirrored, FLIP_INDEX, mask) if flip else dec(outs, mask)), outs

    batch = dict(image=torch.zeros(n, 3, 2 * MAP_H, 2 * MAP_W, device=DEV), mask=torch.ones(n, 2 * MAP_H, 2 * MAP_W, dtype=torch.uint8, device=DEV),
                 center=np.array([[MAP_W, MAP_H]] * n, np.float32), scale=np.array([[2 * MAP_W / 200.0, 2 * MAP_H / 200.0]] * n, np.float32),
                 image_shape=np.array([[2 * MAP_W, 2 * MAP_H]] * n), image_file=[f"{i}.jpg" for i in range(n)])
    return net, batch


def _assert_same_records(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["pred"].dtype == y["pred"].dtype and x["pred"].shape == y["pred"].shape
        assert np.array_equal(x["pred"], y["pred"])
        assert x["score"] == y["score"] and [type(s) for s in x["score"]] == [type(s) for s in y["score"]]
        assert x["image_path"] == y["image_path"]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip_tta_tags"])
def test_inferencer_records_do_not_depend_on_the_finish_switch(monkeypatch, n, flip):
    net, batch = _fake_net(n, flip)
    records = {}
    for refine in (True, False):
        inf = mp.BottomUpHeatMapAEInferencer(net, config=dict(INFER_CFG, refine_missing_joint=refine))
        finished = []
        original = bottomup_inferencer.finish_people_batch
        monkeypatch.setattr(bottomup_inferencer, "finish_people_batch", lambda *a, **kw: (finished.append(1), original(*a, **kw))[1])
        monkeypatch.setenv("MINDPOSE_FINISH_DEVICE", "1")
        on = inf.infer([batch])
        assert finished == [1]
        monkeypatch.setenv("MINDPOSE_FINISH_DEVICE", "0")
        off = inf.infer([batch])
        assert finished == [1]  # the switch keeps the tail on the host
        monkeypatch.setenv("MINDPOSE_FINISH_DEVICE", "1")
        monkeypatch.setenv("MINDPOSE_MATCH_DEVICE", "0")
        host_grouping = inf.infer([batch])
        assert finished == [1]  # no device grouping, no device tail
        monkeypatch.undo()
        assert len(on) == n and all(len(r["pred"]) > 0 for r in on) and on[0]["pred"].shape[2] == (5 if flip else 4)
        _assert_same_records(on, off)
        _assert_same_records(on, host_grouping)
        records[refine] = on
    assert any(not np.array_equal(a["pred"], b["pred"]) for a, b in zip(records[True], records[False]))  # the refinement filled joints


def test_inferencer_makes_two_downloads_and_no_upload(monkeypatch):
    n = 2
    net, batch = _fake_net(n, flip=False)
    inf = mp.BottomUpHeatMapAEInferencer(net, config=INFER_CFG)
    inside = []
    parse = inf._parse
    monkeypatch.setattr(inf, "_parse", lambda *a: (inside.append(1), parse(*a), inside.pop())[1])
    downloads, uploads = [], []
    cpu, from_numpy = torch.Tensor.cpu, torch.from_numpy
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **kw: (downloads.append(t.numel()) if inside and t.is_cuda else None, cpu(t, *a, **kw))[1])
    monkeypatch.setattr(torch, "from_numpy", lambda a: (uploads.append(a.shape) if inside and a.dtype == np.float32 else None, from_numpy(a))[1])
    monkeypatch.setenv("MINDPOSE_FINISH_DEVICE", "1")
    on = inf.infer([batch])
    on_downloads, on_uploads = list(downloads), list(uploads)
    downloads.clear()
    uploads.clear()
    monkeypatch.setenv("MINDPOSE_FINISH_DEVICE", "0")
    off = inf.infer([batch])
    off_downloads, off_uploads = list(downloads), list(uploads)
    monkeypatch.undo()
    _assert_same_records(on, off)
    assert all(len(r["pred"]) > 0 for r in on)
    assert len(on_downloads) == 2 and on_downloads[0] == 2 * n            # counts with status, then the packed persons and scores
    assert max(on_downloads) < K * MAP_H * MAP_W and on_uploads == []    # no map came down, no mean tag went up
    assert len(off_downloads) == 4 and len(off_uploads) == 1             # (the probe sees the host tail's four copies and its upload)


# ---- 6. the old refinement entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_tags,tag_per_joint", [(1, True), (2, True), (1, False)])
def test_refine_missing_entry_keeps_its_bits(num_tags, tag_per_joint):
    k, h, w = 17, 20, 33
    heat, tagging, _ = _maps(21 + num_tags, "normal", 2, k, k if tag_per_joint else 1, h, w, num_tags)
    persons = _persons(21, 2, k, h, w, num_tags, per_image=(5, 4), located_counts=(1, 3, 9, 16, k))
    want, _ = _host_path(persons, heat, tagging, refine=True)
    got = [p.copy() for p in persons]
    mp.BottomUpHeatMapAEInferencer._refine_on_device(got, torch.from_numpy(heat).to(DEV), torch.from_numpy(tagging).to(DEV))
    for g, q in zip(got, want):
        _same(g, q)
    assert any(not np.array_equal(g, p) for g, p in zip(got, persons))


# ---- the Python entries -----------------------------------------------------------------------------------------------------------
def test_python_entries_check_their_arguments():
    k, m, num_tags, h, w = 5, 3, 1, 16, 16
    heat, tagging, _ = _maps(1, "dyadic", 2, k, k, h, w, num_tags)
    persons = _persons(1, 2, k, h, w, num_tags, per_image=(2, 1), located_counts=(2,))
    people, counts, status, heat_dev, tagging_dev = _device_batch(persons, heat, tagging, m)
    good = dict(people=people, counts=counts, status=status, heatmap=heat_dev, tagging=tagging_dev, refine=True, host_match=_no_host_match)
    for change in (dict(people=people[:, :, :, :3]), dict(people=people.transpose(1, 2)), dict(counts=counts.float()), dict(status=status[:1]),
                   dict(heatmap=heat_dev[:, :4]), dict(tagging=tagging_dev[:, :2]), dict(tagging=tagging_dev[:, :, :, :8])):
        with pytest.raises(ValueError):
            finish_people_batch(**dict(good, **change))
    with pytest.raises(_lib.MindposeHipError):
        finish_people_batch(**dict(good, heatmap=heat_dev.cpu()))
    assert finish_people_batch(**dict(good, people=people[:0], counts=counts[:0], status=status[:0], heatmap=heat_dev[:0],
                                      tagging=tagging_dev[:0])) == ([], [])
    _assert_records(finish_people_batch(**good), _host_path(persons, heat, tagging, refine=True))

    val, tag, ind = (torch.zeros(2, k, m, *tail, device=DEV) for tail in ((), (num_tags,), (2,)))
    with pytest.raises(ValueError):
        match_by_tag_device(val, tag, ind, [0] * k)
    with pytest.raises(ValueError):
        match_by_tag_device(val, tag[:, :, :2], ind, list(range(k)))
    with pytest.raises(_lib.MindposeHipError):
        match_by_tag_device(val.cpu(), tag, ind, list(range(k)))
    people, counts, status = match_by_tag_device(val, tag, ind, list(range(k)))
    assert people.shape == (2, k * m, k, 3 + num_tags) and counts.cpu().tolist() == [0, 0] and status.cpu().tolist() == [0, 0]
    empty = match_by_tag_device(val[:0], tag[:0], ind[:0], list(range(k)))
    assert empty[0].shape == (0, k * m, k, 3 + num_tags) and empty[1].shape == (0,) and empty[2].shape == (0,)
