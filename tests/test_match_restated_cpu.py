"""The restated grouping (``tests/match_restated.py``, the specification of the device kernel) against the libraries it restates:
the solver against scipy's ``linear_sum_assignment`` on tie-heavy matrices, the group mean against ``np.mean``, the distance against
``np.linalg.norm``, and the whole function against the recorded outputs of the reference and the host ``match_by_tag``.  If the
numpy or scipy of a machine orders its sums or breaks its ties differently, it shows here, without a GPU."""
import numpy as np
import pytest
import scipy.optimize

from mindpose_amd.utils.match import match_by_tag
from tests.golden_io import load_npz
from tests.match_restated import DUMMY_COST, distance, match_by_tag_restated, mean_tags, solve

F = np.float32


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_solver(cost):
    rows, cols = scipy.optimize.linear_sum_assignment(cost)
    assert rows.tolist() == list(range(cost.shape[0]))
    assert solve([[float(c) for c in row] for row in cost]) == cols.tolist()


@pytest.mark.parametrize("kind", ["integers", "rounded_normals", "uniform"])
def test_solver_matches_scipy_on_tie_heavy_matrices(kind):
    rng = np.random.RandomState(dict(integers=0, rounded_normals=1, uniform=2)[kind])
    for _ in range(250):
        nr = rng.randint(1, 13)
        nc = nr + rng.randint(0, 14)
        if kind == "integers":
            cost = rng.randint(0, 3, (nr, nc)).astype(np.float32)
        elif kind == "rounded_normals":
            cost = np.round(rng.randn(nr, nc).astype(np.float32) ** 2)
        else:
            cost = rng.rand(nr, nc).astype(np.float32)
        _check_solver(cost)


def test_solver_matches_scipy_with_dummy_columns_square_and_single_row():
    rng = np.random.RandomState(3)
    for _ in range(200):  # more rows than real columns: the rest are 1e10 dummies, as match_by_tag pads them
        nr = rng.randint(2, 13)
        real = rng.randint(1, nr)
        cost = np.concatenate((rng.randint(0, 3, (nr, real)).astype(np.float32), np.zeros((nr, nr - real), np.float32) + 1e10), axis=1)
        assert float(cost[0, -1]) == DUMMY_COST
        _check_solver(cost)
    for _ in range(100):
        n = rng.randint(1, 13)
        _check_solver(rng.randint(0, 2, (n, n)).astype(np.float32))  # nr == nc
        _check_solver(rng.randint(0, 2, (1, rng.randint(1, 40))).astype(np.float32))  # nr == 1
    _check_solver(np.zeros((6, 70), np.float32))  # all ties, more columns than one pass of 64


@pytest.mark.parametrize("num_tags", [1, 2, 3, 4])
def test_mean_matches_numpy(num_tags):
    rng = np.random.RandomState(num_tags)
    for n in range(1, 65):
        for _ in range(4):
            tags = (rng.randn(n, num_tags) * 10.0 ** rng.randint(-3, 4, (n, num_tags))).astype(np.float32)
            want = np.mean(np.stack(list(tags)), axis=0)
            got = np.array(mean_tags(list(tags)), np.float32)
            assert _bits_equal(got, want), (num_tags, n)


@pytest.mark.parametrize("num_tags", [1, 2, 3, 4])
def test_distance_matches_numpy_norm(num_tags):
    rng = np.random.RandomState(10 + num_tags)
    rows = (rng.randn(40, num_tags) * 10.0 ** rng.randint(-2, 3, (40, 1))).astype(np.float32)
    means = rng.randn(9, num_tags).astype(np.float32)
    want = np.linalg.norm(rows[:, None, :] - means[None, :, :], ord=2, axis=2)
    got = np.array([[distance(r, list(m)) for m in means] for r in rows], np.float32)
    assert _bits_equal(got, want)
    assert np.array_equal(np.round(want), np.rint(want))  # np.round is round-half-to-even
    assert np.round(F(0.5)) == 0 and np.round(F(1.5)) == 2 and np.round(F(2.5)) == 2


def test_restated_match_bit_equal_to_reference_fixtures():
    z = load_npz("match_by_tag.npz")
    count = int(z["count"])
    assert count >= 60
    for i in range(count):
        vis_thr, tag_thr, ignore, rounded = z[f"c{i}_args"]
        got = match_by_tag_restated(z[f"c{i}_val"], z[f"c{i}_tag"], z[f"c{i}_ind"], [int(j) for j in z[f"c{i}_order"]],
                                    vis_thr=float(vis_thr), tag_thr=float(tag_thr), ignore_too_much=bool(ignore),
                                    use_rounded_norm=bool(rounded))
        assert _bits_equal(got, z[f"c{i}_out"]), f"case {i}"


def _both(val, tag, ind, order, **kwargs):
    """The restated and the host function on one case; they must agree bit for bit."""
    got = match_by_tag_restated(val, tag, ind, order, **kwargs)
    want = match_by_tag(val, tag, ind, order, **kwargs)
    assert _bits_equal(got, want)
    return got


def _case(values, tags):
    """val_k [K, M], tag_k [K, M, L], ind_k [K, M, 2] from nested lists; x = 10 * joint + candidate, y = 100 + x."""
    val = np.array(values, np.float32)
    tag = np.array(tags, np.float32)
    k, m = val.shape
    x = (10 * np.arange(k)[:, None] + np.arange(m)[None, :]).astype(np.float32)
    return val, tag.reshape(k, m, -1), np.stack((x, x + 100), axis=2)


def test_thresholds_are_float32_comparisons():
    # tag_thr: a distance of exactly float32(0.1) is not below tag_thr = 0.1 - the second joint opens a group of its own
    val, tag, ind = _case([[0.9], [0.9]], [[0.0], [F(0.1)]])
    out = _both(val, tag, ind, [0, 1], tag_thr=0.1, use_rounded_norm=False)
    assert out.shape == (2, 2, 4) and out[0, 1, 2] == 0 and out[1, 0, 2] == 0
    out = _both(val, tag, ind, [0, 1], tag_thr=0.1)  # the rounded cost is 0, the test still reads the unrounded distance
    assert out.shape == (2, 2, 4)
    # float32(0.7) < 0.7 in double: as a double comparison this distance would be below the threshold and join the group
    val, tag, ind = _case([[0.9], [0.9]], [[0.0], [F(0.7)]])
    assert float(F(0.7)) < 0.7
    assert _both(val, tag, ind, [0, 1], tag_thr=0.7).shape == (2, 2, 4)
    # one float32 step closer joins it
    tag[1, 0, 0] = np.nextafter(F(0.7), F(0))
    assert _both(val, tag, ind, [0, 1], tag_thr=0.7).shape == (1, 2, 4)
    # vis_thr: a value of exactly float32(0.1) is not above vis_thr = 0.1 (as doubles it would be)
    assert float(F(0.1)) > 0.1
    val, tag, ind = _case([[F(0.1), 0.9]], [[1.0, 5.0]])
    out = _both(val, tag, ind, [0], vis_thr=0.1)
    assert out.shape == (1, 1, 4) and out[0, 0].tolist() == [1.0, 101.0, F(0.9), 5.0]
    val[0, 0] = np.nextafter(F(0.1), F(1))
    assert _both(val, tag, ind, [0], vis_thr=0.1).shape == (2, 1, 4)


def test_key_collision_keeps_the_other_joints_and_resets_the_tag_list():
    # L = 2.  Joint 0 opens A (key 1) and B (key 9).  Joint 1: a detection with A's first tag value but a far second one is no match
    # (distance 6 >= tag_thr), so it "opens" key 1 again: A keeps joint 0, takes this row for joint 1, and its tag list becomes
    # [(1, 6)] alone.  Within the same step a second detection with the key 1 as well overwrites joint 1 again: list [(1, 7)].
    # Joint 2 then measures against mean (1, 7): (1, 7.25) joins A; against the unreset mean ((1,0)+(1,6)+(1,7))/3 it would not.
    values = [[0.9, 0.8, 0.0], [0.7, 0.6, 0.0], [0.5, 0.0, 0.0]]
    tags = [[[1.0, 0.0], [9.0, 0.0], [0.0, 0.0]],
            [[1.0, 6.0], [-1.0, 7.0], [0.0, 0.0]],
            [[1.0, 7.25], [0.0, 0.0], [0.0, 0.0]]]
    val, tag, ind = _case(values, tags)
    tag[1, 1, 0] = 1.0  # the within-step collision: both detections of joint 1 carry key 1
    out = _both(val, tag, ind, [0, 1, 2], use_rounded_norm=False)
    assert out.shape == (2, 3, 5)
    a, b = out
    assert a[0].tolist() == [0.0, 100.0, F(0.9), 1.0, 0.0]    # joint 0 of the earlier holder is kept
    assert a[1].tolist() == [11.0, 111.0, F(0.6), 1.0, 7.0]   # the later detection of the step overwrote the earlier one
    assert a[2].tolist() == [20.0, 120.0, F(0.5), 1.0, 7.25]  # joined through the reset list
    assert b[0, 2] == F(0.8) and not b[1:].any()
    # -0.0 and 0.0 are one key
    val, tag, ind = _case([[0.9, 0.8]], [[0.0, -0.0]])
    out = _both(val, tag, ind, [0])
    assert out.shape == (1, 1, 4) and out[0, 0, 2] == F(0.8) and np.signbit(out[0, 0, 3])


def test_random_cases_bit_equal_to_the_host_function():
    rng = np.random.RandomState(7)
    for case in range(30):
        k, m, num_tags = rng.randint(1, 7), rng.randint(1, 9), rng.randint(1, 5)
        val = rng.rand(k, m).astype(np.float32)
        tag = (rng.randint(0, 8, (k, m, num_tags)) * 0.5).astype(np.float32)  # half-integers: ties in the rounded costs
        ind = rng.randint(0, 64, (k, m, 2)).astype(np.float32)
        order = rng.permutation(k).tolist()
        _both(val, tag, ind, order, vis_thr=0.3, tag_thr=1.0, ignore_too_much=bool(case % 2), use_rounded_norm=bool(case % 3))
