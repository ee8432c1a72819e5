"""tests/pose_matrix.py checked without a GPU: the lists keep the maps, row counts, refine / flip forms, peak positions, tie kinds,
window classes and loss sizes that tests/test_gpu_pose_edges.py is written to reach (the floors below fail when a later edit thins a
list), the quoted source lines exist in the files of csrc/ they name, and every builder does what it says ON THE ORACLE ALONE: the designed
arg-max is the oracle's, a plateau does not move, every designed key point falls into its window class, the DARK blobs give a
regular Hessian, and the float64 loss references agree with oracle.loss."""
import os
import re

import numpy as np
import pytest

from oracle import decoder as od
from oracle import loss as ol
from oracle import target as ot
from tests import pose_matrix as pm
from tests.golden import recipes

CASES_BY_MAP = {}
for _c in pm.DECODE_CASES:
    CASES_BY_MAP.setdefault((_c.h, _c.w), []).append(_c)


def test_decoder_lists_keep_their_floors():
    assert set(pm.DECODE_MAPS) >= {(1, 1), (1, 5), (5, 1), (2, 2), (7, 9), (6, 10), (3, 67), (8, 4), (4, 68), (20, 52), (64, 48)}
    assert {n * k for n, k in pm.ROW_SHAPES} == {1, 5, 7, 8}
    assert set(pm.REFINE_FORMS) >= {("none", 0), ("shift", 0)} | {("dark", ks) for ks in (1, 3, 11, 17, 19, 21, 63)}
    assert set(pm.FLIP_FORMS) == {(0, 0), (1, 0), (1, 1)} and set(pm.AVG_FORMS) == {True, False}
    assert pm.FLIP_INDEX[5] == [0, 2, 1, 4, 3] and sorted(pm.FLIP_INDEX[7]) == list(range(7))
    for k, fi in pm.FLIP_INDEX.items():
        assert sorted(fi) == list(range(k))
        if k >= 4:
            assert any(fi[j] == j for j in range(k)) and any(fi[j] != j for j in range(k)), "a permutation with fixed points and swaps"
    cases = pm.DECODE_CASES
    # every map with every row count, refine form and flip form
    assert {(c.h, c.w, c.n * c.k, c.refine, c.ks, c.flip, c.shift_heatmap) for c in cases} == \
        {(h, w, n * k, r, ks, f, s) for h, w in pm.DECODE_MAPS for n, k in pm.ROW_SHAPES for r, ks in pm.REFINE_FORMS for f, s in pm.FLIP_FORMS}
    # every (decode_path, refine form, flip) triple, with both column shifts under the flip test
    assert {(pm.decode_path(c.h, c.w, c.flip), c.refine, c.ks, c.flip, c.shift_heatmap) for c in cases} == \
        {(p, r, ks, f, s) for p in ("quad", "scalar") for r, ks in pm.REFINE_FORMS for f, s in pm.FLIP_FORMS}
    # both DARK paths, with and without the flip test, on both decode paths
    assert {(pm.dark_path(c.ks), c.flip, pm.decode_path(c.h, c.w, c.flip)) for c in cases if c.refine == "dark"} == \
        {(d, f, p) for d in ("patch", "loop") for f in (0, 1) for p in ("quad", "scalar")}
    assert {pm.dark_path(ks) for ks in (1, 3, 11, 17)} == {"patch"} and {pm.dark_path(ks) for ks in (19, 21, 63)} == {"loop"}
    assert 21 * 21 > 6 * 64 and sum(63 > 2 * max(h, w) for h, w in pm.DECODE_MAPS) >= 6  # larger than every small map
    # the maps reach what their comments say
    assert pm.decode_path(2, 2, 0) == "quad" and pm.decode_path(2, 2, 1) == "scalar"
    assert pm.decode_path(6, 10, 0) == "quad" and pm.decode_path(6, 10, 1) == "scalar"
    assert pm.decode_path(20, 52, 1) == "quad" and 256 < 20 * 52 // 4 < 512 and (20 * 52 // 4) % 64
    assert pm.decode_path(7, 9, 0) == pm.decode_path(3, 67, 0) == "scalar" and pm.decode_path(4, 68, 1) == "quad" and 8 * 4 // 4 < 64
    # the flip forms run on the smallest maps too; to_original and UDP vary under every refine form, UDP only where it is defined
    for hw in ((1, 5), (5, 1), (2, 2)):
        assert {(c.flip, c.shift_heatmap) for c in CASES_BY_MAP[hw]} == set(pm.FLIP_FORMS)
    for r, ks in pm.REFINE_FORMS:
        for f in (0, 1):
            assert {(c.to_original, c.use_udp) for c in cases if (c.refine, c.ks, c.flip) == (r, ks, f)} == set(pm.ORIGINAL_FORMS)
    assert all(c.h >= 2 and c.w >= 2 for c in cases if c.use_udp)


@pytest.mark.parametrize("h,w", list(pm.DECODE_MAPS), ids=[f"{h}x{w}" for h, w in pm.DECODE_MAPS])
def test_every_map_reaches_its_positions_and_ties(h, w):
    admitted = pm.peak_positions(h, w)
    assert set(admitted) <= set(pm.PEAK_NAMES) and set(pm.peak_positions(64, 48)) == set(pm.PEAK_NAMES) and len(pm.PEAK_NAMES) == 11
    assert set(admitted) >= {"corner_tl", "corner_tr", "corner_bl", "corner_br", "flat_first", "flat_last"}
    assert ("edge_top" in admitted) == ("edge_bottom" in admitted) == (w >= 3) and ("edge_left" in admitted) == ("edge_right" in admitted) == (h >= 3)
    assert ("interior" in admitted) == (h >= 3 and w >= 3)
    assert admitted["flat_first"] == (0, 0) and admitted["flat_last"] == (h - 1, w - 1)
    if "interior" in admitted:
        y, x = admitted["interior"]
        assert 1 <= y <= h - 2 and 1 <= x <= w - 2
    ties = pm.tie_indices(h, w)
    for kind, idx in ties.items():
        assert len(set(idx)) == len(idx) >= 2 and max(idx) < h * w, kind
    assert len(pm.plane_specs(h, w)) <= sum(n * k for n, k in pm.ROW_SHAPES), "more designed planes than the row shapes hold"
    for r, ks in pm.REFINE_FORMS:
        for f, s in pm.FLIP_FORMS:
            mine = [c for c in CASES_BY_MAP[(h, w)] if (c.refine, c.ks, c.flip, c.shift_heatmap) == (r, ks, f, s)]
            specs = [sp for c in mine for sp in pm.row_specs(h, w, c.n, c.k, r == "dark")]
            names = {(sp.kind, nm) for sp in specs for nm in sp.names}
            assert names >= {("peak_at", nm) for nm in admitted}, (r, ks, f, s)
            if r != "dark":
                assert names >= {("ties", kind) for kind in ties} | {("negative", "negative"), ("empty", "inf"), ("empty", "nan")}
                assert (("plateau", "plateau") in names) == (h >= 3 or w >= 3)


def test_tie_kinds_sit_where_the_kernel_separates_them():
    by_kind = {}
    for h, w in pm.DECODE_MAPS:
        for kind, idx in pm.tie_indices(h, w).items():
            by_kind.setdefault(kind, []).append((h, w, idx))
    assert set(by_kind) == set(pm.TIE_KINDS)
    quad = lambda i: i // 4  # noqa: E731
    # on a quad-path map: one lane's float4; two lanes of one round; one lane's next step; one lane's next round
    assert any(pm.decode_path(h, w, 0) == "quad" and quad(i[0]) == quad(i[1]) for h, w, i in by_kind["same_quad"])
    assert any(pm.decode_path(h, w, 0) == "quad" and quad(i[0]) % 64 != quad(i[1]) % 64 and quad(i[1]) < 64 for h, w, i in by_kind["same_round"])
    assert any(pm.decode_path(h, w, 1) == "quad" and quad(i[1]) - quad(i[0]) == 64 for h, w, i in by_kind["lane_steps"])
    assert any(pm.decode_path(h, w, 1) == "quad" and quad(i[1]) - quad(i[0]) == 256 for h, w, i in by_kind["two_rounds"])
    # on a scalar-path map: one lane's columns x and x + 64 of one row
    assert any(pm.decode_path(h, w, 0) == "scalar" and i[1] - i[0] == 64 and i[0] // w == i[1] // w for h, w, i in by_kind["scalar_i_i64"])
    assert any(len(i) == 3 for _, _, i in by_kind["three"]) and all(len(i) == h * w for h, w, i in by_kind["constant"])


def test_quoted_lines_exist_in_the_source():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mindpose_amd", "csrc")
    text = {}
    for name, (source, line) in pm.SOURCE_LINES.items():
        if source not in text:
            with open(os.path.join(csrc, source)) as f:
                text[source] = f.read()
        assert line in text[source], (name, source, line)
    # ONE host predicate picks the path of the joint MSE and the OHKM loss, forward and backward: one definition, and every launch
    # of the row and backward kernels takes its `vec` from it
    loss = text["joints_loss.hip"]
    assert len(re.findall(r"\bint vec16\(", loss)) == 1 and pm.SOURCE_LINES["mse_path"][1] in loss
    assert len(re.findall(r"& *3\b", loss)) == 1  # nothing else in the file decides a path by hw % 4
    # the row kernel and the backward kernel are each launched from one place, with vec16's answer
    for kernel in ("joints_sq_row_kernel", "joints_bwd_kernel"):
        launches = re.findall(r"hipLaunchKernelGGL\(\s*" + kernel + r"\b[^;]*;", loss)
        assert len(launches) == 1 and "vec16(" in launches[0], kernel
    assert f"kDarkFastKs = {pm.DARK_FAST_KS};" in pm.SOURCE_LINES["dark_path"][1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("h,w", list(pm.DECODE_MAPS), ids=[f"{h}x{w}" for h, w in pm.DECODE_MAPS])
def test_decoder_builders_on_the_oracle(h, w):
    """the designed arg-max is the oracle's on every plane (peaks, ties, negative, empty); all values are dyadic and below 4; under
    the flip test the oracle's aggregation of the two inputs is the designed map to the bit; a plateau does not move under shift"""
    seen_done = set()
    for c in CASES_BY_MAP[(h, w)]:
        key = (c.n, c.k, c.refine == "dark", c.flip, c.shift_heatmap)
        if key in seen_done:
            continue  # the data depend on nothing else
        seen_done.add(key)
        d = pm.decode_inputs(c)
        seen = d["seen"]
        _, vals, idx = od.get_max_preds(seen)
        assert np.array_equal(idx, d["index"]), (c, idx, d["index"])
        grid = pm.Q12 if c.refine == "dark" else pm.Q6
        for name in ("hm", "hf"):
            if name in d:
                v = d[name][np.isfinite(d[name])].astype(np.float64)
                assert np.all(v / grid == np.round(v / grid)) and np.all(np.abs(v) < 4), (c, name)
        if c.flip:
            with np.errstate(invalid="ignore"):
                avg = od.flip_aggregate(d["hm"], d["hf"], d["flip_index"], shift_heatmap=bool(c.shift_heatmap))
            same = (_bits(avg) == _bits(seen)) | (np.isnan(avg) & np.isnan(seen))
            assert same.all(), c
            assert np.array_equal(pm.flip_back(d["hf"], d["flip_index"], c.shift_heatmap), od.flip_back(d["hf"], d["flip_index"], bool(c.shift_heatmap)))
        flat = seen.reshape(c.n * c.k, -1)
        for row, sp in enumerate(d["specs"]):
            if sp.kind == "peak_at":
                assert (flat[row] == flat[row, sp.index]).sum() == 1, "the designed maximum is unique"
            elif sp.kind == "ties" and sp.names[0] != "constant":
                where = np.nonzero(flat[row] == flat[row].max())[0]
                assert tuple(where) == tuple(sorted(pm.tie_indices(h, w)[sp.names[0]])) and sp.index == where[0]
            elif sp.kind == "negative":
                assert flat[row].max() < 0
            elif sp.kind == "empty":
                assert np.isnan(flat[row]).all() if sp.names[0] == "nan" else (flat[row] == -np.inf).all()
                v0 = vals.reshape(-1)[row]
                assert np.isnan(v0) if sp.names[0] == "nan" else v0 == -np.inf  # the value of pixel (0, 0)
        if c.refine != "dark":
            coords, _, idx = od.get_max_preds(seen)
            with np.errstate(invalid="ignore"):
                moved = od.shift_coordinate(coords, seen, idx).reshape(-1, 2)
            for row, sp in enumerate(d["specs"]):
                if sp.kind == "plateau":
                    assert np.array_equal(moved[row], coords.reshape(-1, 2)[row]), c


@pytest.mark.parametrize("h,w", [hw for hw in pm.DECODE_MAPS if "interior" in pm.peak_positions(*hw)], ids=lambda v: str(v))
def test_dark_blobs_give_a_regular_hessian(h, w):
    """DARK blob planes with the peak in the interior: the oracle's determinant of H + 1e-7 I is not zero, for every blur size; the
    clip [1e-3, 50] is inactive at the centre and, on a map larger than the blob, active far from it"""
    spec = [s for s in pm.plane_specs(h, w, dark=True) if "interior" in s.names][0]
    plane = pm.build_plane(h, w, spec, np.random.default_rng([5, h, w]), dark=True)[None, None]
    coords, _, idx = od.get_max_preds(plane)
    assert int(idx[0, 0]) == spec.index
    for _, ks in [f for f in pm.REFINE_FORMS if f[0] == "dark"]:
        t = {}
        od.dark_udp_refine_coords(coords, plane, ks, terms=t)
        ha, hd = np.float32(t["dxx"][0, 0]) + np.float32(1e-7), np.float32(t["dyy"][0, 0]) + np.float32(1e-7)
        det = ha * hd - np.float32(t["dxy"][0, 0]) ** 2
        assert np.isfinite(det) and det != 0, (ks, det)
        assert np.log(np.float32(0.001)) < t["neighbourhood"][0, 0, 4] < np.log(np.float32(50)), ks
    if (h, w) == (64, 48):
        blur = od._depthwise_blur_same(plane, od.create_gaussian_kernel(11))
        assert blur.min() < 0.001 < blur.max()


# ---- targets -------------------------------------------------------------------------------------------------------------------------

def test_target_lists_keep_their_floors():
    cases = pm.TARGET_CASES
    assert {(c.h, c.w) for c in cases} >= {(7, 9), (10, 6), (5, 5), (1, 8), (8, 1), (16, 12), (64, 48)}
    assert {c.sigma for c in cases} == {1, 2, 3} and all(float(3 * c.sigma).is_integer() for c in cases)
    assert any((c.h, c.w, c.sigma) == (5, 5, 2) for c in cases) and 6 * 2 + 1 > 5  # the stamp is clipped on all four sides
    for udp in (0, 1):
        mine = [c for c in cases if c.use_udp == udp]
        assert {pm.target_zero_path(c.w) for c in mine} == {"quad", "scalar"} and {c.joint_weights for c in mine} == {0, 1}
        assert any(c.stride == 1 for c in mine) and {c.sigma for c in mine} == {1, 2, 3}
        assert any(min(c.h, c.w) < 6 * c.sigma + 1 for c in mine) and any(min(c.h, c.w) > 6 * c.sigma + 1 for c in mine)
    assert {(c.h, c.w) for c in cases if not c.use_udp} >= {(1, 8), (8, 1)} and all(min(c.h, c.w) >= 2 for c in cases if c.use_udp)
    assert len(pm.JOINT_WEIGHTS) == pm.TARGET_K and len(set(pm.JOINT_WEIGHTS)) >= 4 and 0.0 in pm.JOINT_WEIGHTS
    assert set(pm.VISIBILITIES) == {0.0, 0.5, 1.0, 2.0} and pm.HUGE == 3.0e9
    assert {m % 2 for m in pm.HALVES} == {0, 1} and any(m > 0 for m in pm.HALVES) and any(m < 0 for m in pm.HALVES)
    assert set(pm.AXIS_CLASSES) == {"br0", "br-1", "ul_last", "ul_end", "centre", "border_lo", "border_hi"}


def _mu(v, stride, use_udp):
    fx = np.float32(v) / np.float64(stride)
    return (int(fx + 0.5) if use_udp else round(fx)), fx


@pytest.mark.parametrize("case", pm.TARGET_CASES, ids=str)
def test_target_points_fall_into_their_window_classes(case):
    """every designed key point, through the oracle's own rounding and `_window`, lies in the class it was designed for - for x, for y
    and for both together, per encoding - and the classes give the weights and supports the reference's bounds test implies"""
    h, w, tmp = case.h, case.w, 3 * case.sigma
    pts = pm.target_points(case)
    labels = {(lx, ly) for lx, ly, *_ in pts}
    for cls in pm.AXIS_CLASSES:
        assert {(cls, "centre"), ("centre", cls), (cls, cls)} <= labels, cls
    for m in pm.HALVES:
        assert {(f"half{m}", "centre"), ("centre", f"half{m}")} <= labels
    assert {"udp_trunc", "huge+", "huge-"} <= {lx for lx, *_ in pts} and {"udp_trunc", "huge+", "huge-"} <= {ly for _, ly, *_ in pts}
    assert {v for lx, ly, _, _, v in pts if (lx, ly) == ("centre", "centre")} == set(pm.VISIBILITIES)
    kp = pm.target_keypoints(case)
    assert kp.dtype == np.float32 and kp.shape[1:] == (pm.TARGET_K, 3) and kp.shape[0] * pm.TARGET_K >= len(pts)
    flat = kp.reshape(-1, 3)
    img = pm.target_image_size(case)
    stride = (np.array(img) - 1.0) / (np.array([w, h]) - 1.0) if case.use_udp else np.array(img) / np.array([w, h])
    assert stride[0] == stride[1] == case.stride  # the oracle's own feat_stride is the case's stride, exactly
    target, weight = ot.generate_target(kp, img, [w, h], float(case.sigma), use_udp=bool(case.use_udp))
    target, weight = target.reshape(-1, h, w), weight.reshape(-1)
    for i, (lx, ly, kx, ky, vis) in enumerate(pts):
        assert tuple(flat[i]) == (np.float32(kx), np.float32(ky), np.float32(vis))
        (mx, fx), (my, fy) = _mu(kx, case.stride, case.use_udp), _mu(ky, case.stride, case.use_udp)
        ulx, brx, *_ = ot._window(mx, tmp, w)
        uly, bry, *_ = ot._window(my, tmp, h)
        assert pm.axis_class_holds(lx, mx, ulx, brx, w) and pm.axis_class_holds(ly, my, uly, bry, h), (lx, ly, mx, my)
        for lab, f, mu in ((lx, fx, mx), (ly, fy, my)):
            if lab.startswith("half"):
                m = int(lab[4:])
                assert f == m + 0.5 and mu == (m + 1 if case.use_udp else (m if m % 2 == 0 else m + 1))
            if lab == "udp_trunc":
                assert -1 < f + 0.5 < 0 and mu == (0 if case.use_udp else -1)
            if lab.startswith("huge"):
                assert abs(f) == pm.HUGE / case.stride and (abs(f) > 1.0e9) == (case.stride == 1)
        oob = {"br-1", "ul_end", "huge+", "huge-"}
        empty = lx == "br0" or ly == "br0"
        if lx in oob or ly in oob:
            assert weight[i] == 0 and not target[i].any()
        elif not (lx.startswith("half") or ly.startswith("half") or "udp_trunc" in (lx, ly)):
            assert weight[i] == np.float32(vis)
            assert target[i].any() == (vis > 0.5 and not empty), (lx, ly)
            if vis > 0.5 and not empty and "ul_last" in (lx, ly):
                assert (target[i] != 0).sum() <= max(min(h, 2 * tmp + 1), min(w, 2 * tmp + 1))  # one column or one row of the stamp


def test_window_edges_known_answers():
    """map 7 x 9, stride 4, sigma 1 and 2: br == 0 is in bounds (weight 1, an all-zero plane), br == -1 is not; ul == w - 1 stamps
    one column (7 pixels), ul == w is out of bounds"""
    for sigma in (1, 2):
        tmp = 3 * sigma
        for udp in (False, True):
            img = [33, 25] if udp else [36, 28]
            low = 2.0 if udp else 0.0  # UDP truncates toward zero: a negative mu takes fx = mu - 0.5
            kp = np.array([[[(-tmp - 1) * 4.0 - low, 12.0, 1.0], [(-tmp - 2) * 4.0 - low, 12.0, 1.0], [(8 + tmp) * 4.0, 12.0, 1.0],
                            [(9 + tmp) * 4.0, 12.0, 1.0]]], dtype=np.float32)
            target, weight = ot.generate_target(kp, img, [9, 7], float(sigma), use_udp=udp)
            assert weight.tolist() == [[1.0, 0.0, 1.0, 0.0]]
            assert [int((t != 0).sum()) for t in target[0]] == [0, 0, 7, 0]
    assert round(2.5) == 2 and round(3.5) == 4 and round(-2.5) == -2 and round(-3.5) == -4 and int(-0.25) == 0


# ---- JointsMSELoss -------------------------------------------------------------------------------------------------------------------

def test_mse_lists_keep_their_floors():
    assert set(pm.MSE_HW_SCALAR) >= {1, 3, 63, 255, 257, 1023} and {pm.mse_path(v) for v in pm.MSE_HW_SCALAR} == {"scalar"}
    assert set(pm.MSE_HW_QUAD) >= {4, 252, 1028, 3072} and {pm.mse_path(v) for v in pm.MSE_HW_QUAD} == {"quad"}
    assert set(pm.MSE_ROWS) >= {1, 5, 257, 600} and all(n * k == r for r, (n, k) in pm.MSE_ROWS.items())
    assert any(256 < r <= 512 and r % 256 for r in pm.MSE_ROWS) and any(512 < r and r % 256 for r in pm.MSE_ROWS)
    assert set(pm.MSE_CASES) == {(hw, r, wk) for hw in pm.MSE_HW_SCALAR + pm.MSE_HW_QUAD for r in pm.MSE_ROWS for wk in ("none", "ones", "mix")}
    assert None in pm.MSE_GRADS and any(g is not None and g != 1 for g in pm.MSE_GRADS)
    _, _, w = pm.mse_inputs(63, 600, "mix")
    assert set(np.unique(w)) == {0.0, 0.5, 2.0}
    # the additions of one thread: a stride of 256 scalars or 256 float4
    assert [pm.mse_additions(v) for v in (1, 255, 257, 1023)] == [1, 1, 2, 4] and [pm.mse_additions(v) for v in (4, 1028, 3072)] == [4, 8, 12]
    assert pm.mse_fwd_tolerance(3072) == 24 * 2.0 ** -24 and pm.MSE_BWD_TOLERANCE == 4 * 2.0 ** -24


@pytest.mark.parametrize("name", list(recipes.LOSS_CASES))
def test_mse_references_agree_with_the_oracle(name):
    """The float64 references of pose_matrix against oracle.loss on the existing loss cases.  The oracle squares and weights in fp32
    before its float64 mean: three roundings per (non-negative) term, 3 * 2^-24 of the value, and one more for its fp32 result; its
    gradient differs from the fp32 restatement by the order of three multiplies."""
    shape, seed = recipes.LOSS_CASES[name]
    pred, target, w = recipes.loss_inputs(shape, seed)
    rows = shape[0] * shape[1]
    p2, t2, w1 = pred.reshape(rows, -1), target.reshape(rows, -1), w.reshape(rows)
    for weights in (None, w1):
        ref, mag = pm.mse_fwd_ref(p2, t2, weights)
        want = float(ol.joints_mse(pred, target, w, use_target_weight=weights is not None))
        assert ref == mag and abs(ref - want) <= 4 * pm.U24 * ref
        for g in pm.MSE_GRADS:
            g64 = pm.mse_bwd_ref(p2, t2, weights, g)
            got = pm.mse_bwd_restated(p2, t2, weights, g)
            assert got.dtype == np.float32 and np.all(np.abs(got - g64) <= pm.MSE_BWD_TOLERANCE * np.abs(g64))
            theirs = ol.joints_mse_grad(pred, target, w, use_target_weight=weights is not None, grad_out=1.0 if g is None else g)
            np.testing.assert_allclose(theirs.reshape(rows, -1), g64, rtol=4 * pm.U24, atol=0)
    # a weight of -1 shows in the magnitude only
    ref, mag = pm.mse_fwd_ref(p2[:2], t2[:2], np.array([-1.0, 1.0], dtype=np.float32))
    assert mag > abs(ref)


@pytest.mark.parametrize("hw", [1, 63, 257, 1023, 252, 1028, 3072])
@pytest.mark.parametrize("weights", ["none", "mix"])
def test_mse_restatement_of_the_row_pass(hw, weights):
    """mse_rows_restated / mse_fwd_restated (the fp32 row pass, thread by thread) against float64 within the bound the GPU test allows,
    on both paths where the size admits both.  The two paths associate differently: on the unweighted inputs some row differs in its
    bits.  The value-only mutant of the four-wave sum, a dropped ws[2] + ws[3], is outside the bound wherever threads 128 ... 255 hold
    elements."""
    pred, target, w = pm.mse_inputs(hw, 5, weights)
    ref, mag = pm.mse_fwd_ref(pred, target, w)
    terms64 = (pred.astype(np.float64) - target.astype(np.float64)) ** 2 * (1.0 if w is None else w.astype(np.float64)[:, None])
    rows64 = terms64.sum(axis=1)
    got = {}
    for path in ["scalar"] + (["quad"] if hw % 4 == 0 else []):
        got[path] = pm.mse_rows_restated(pred, target, w, path)
        assert got[path].dtype == np.float32
        # the path's own additions: the scalar loop on a quad size makes ceil(hw / 256) of them
        bound = ((pm.ceil_div(hw, 256) if path == "scalar" else pm.mse_additions(hw)) + 12) * pm.U24
        assert np.all(np.abs(got[path] - rows64) <= bound * np.abs(rows64)), (path, got[path], rows64)
        assert abs(float(pm.mse_fwd_restated(pred, target, w, path)) - ref) <= bound * mag
        unit = 1 if path == "scalar" else 4
        upper = (np.arange(hw) // unit) % 256 >= 128  # the elements of waves 2 and 3
        if upper.any():
            assert abs(terms64[:, ~upper].sum() / pred.size - ref) > bound * mag
    if len(got) == 2 and weights == "none" and hw >= 252:
        assert (got["scalar"].view(np.uint32) != got["quad"].view(np.uint32)).any()
