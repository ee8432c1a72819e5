"""Every case of tests/pose_matrix.py on the device: decode_kernel<FLIP> (quad and scalar streaming, the register-patch and the
per-tap DARK paths, the all -inf / NaN branch), flip_aggregate_kernel, gaussian_target_kernel (both zeroing paths, every window edge)
and the three JointsMSELoss kernels (both paths, a second and a third stride of the final sum).  Each case goes through the C ABI and
through the Python wrapper that accepts it (create_decoder, decode_flip_aggregated, TopDownGenerateTarget, create_loss).

What is compared:
  * decoder without refinement and with the shift: arg-max, max values, boxes, coordinates and the materialised average, bit for bit
    with oracle.decoder (a NaN equals a NaN); with and without avg_out; the stand-alone aggregation bit for bit;
  * DARK: the kernel's intermediates against the oracle term by term and the solve as a solve (check_dark_intermediates of
    tests/test_gpu_pose_ops.py); under the flip test on the averaged map of mp_flip_aggregate, and the fused entry must then return
    the bits mp_decode_topdown returns on that map; the back-projection is the oracle's fp32 expression on the kernel's coordinates;
  * targets: weights, support and plain values bit for bit, UDP values within 1 fp32 ulp of the oracle; outputs start as NaN;
  * loss: forward within (A + 12) 2^-24 of the float64 value (pose_matrix.mse_fwd_tolerance), two runs bit-identical; backward bit for
    bit with the fp32 restatement and within 4 * 2^-24 of float64; outputs start as NaN.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from oracle import decoder as od  # noqa: E402
from oracle import target as ot  # noqa: E402
from tests import pose_matrix as pm  # noqa: E402
from tests.test_gpu_pose_ops import check_dark_intermediates  # noqa: E402

DEV = "cuda:0"
LIB = _lib.load()
REFINE_CODE = {"none": _lib.MP_REFINE_NONE, "shift": _lib.MP_REFINE_SHIFT, "dark": _lib.MP_REFINE_DARK}
PIXEL_STD = 200.0


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    """bit for bit; a NaN equals a NaN (no reference pins a NaN's payload)"""
    got = np.ascontiguousarray(got.cpu().numpy() if torch.is_tensor(got) else got)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    else:
        diff = got != want
    if diff.any():
        at = tuple(int(v[0]) for v in np.nonzero(diff))
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits, first at {at}: got {got[at]!r}, want {want[at]!r}")


def _decoder(case):
    return mp.create_decoder("topdown_heatmap", pixel_std=PIXEL_STD, to_original=bool(case.to_original), shift_coordinate=case.refine == "shift",
                             use_udp=bool(case.use_udp), dark_udp_refine=case.refine == "dark", kernel_size=case.ks or 11).to(DEV)


class _Launch:
    """device operands of one decoder case and the two C entry points on them; outputs start as a sentinel no result equals"""

    def __init__(self, case, d, dec):
        self.case, self.dec = case, dec
        self.hm, self.center, self.scale, self.score = (_cuda(d[key]) for key in ("hm", "center", "scale", "score"))
        self.blur = dec._blur_on(torch.device(DEV))
        if case.flip:
            self.hf, self.fi = _cuda(d["hf"]), torch.tensor(d["flip_index"], dtype=torch.int32, device=DEV)

    def _outs(self):
        c = self.case
        return (torch.full((c.n, c.k, 3), -777.0, device=DEV), torch.full((c.n, 6), -777.0, device=DEV),
                torch.full((c.n, c.k), -777, dtype=torch.int32, device=DEV))

    def decode(self, hm, to_original=None):
        c = self.case
        preds, boxes, idx = self._outs()
        _lib.check(LIB.mp_decode_topdown(hm.data_ptr(), self.center.data_ptr(), self.scale.data_ptr(), self.score.data_ptr(), preds.data_ptr(),
                                         boxes.data_ptr(), idx.data_ptr(), c.n, c.k, c.h, c.w, REFINE_CODE[c.refine], c.use_udp,
                                         c.to_original if to_original is None else to_original, PIXEL_STD, _lib.ptr(self.blur), c.ks or 11,
                                         _lib.stream()), "mp_decode_topdown")
        return preds, boxes, idx

    def flip_decode(self, with_avg, to_original=None):
        c = self.case
        preds, boxes, idx = self._outs()
        avg = torch.full_like(self.hm, float("nan")) if with_avg else None
        _lib.check(LIB.mp_flip_aggregate_decode(self.hm.data_ptr(), self.hf.data_ptr(), self.fi.data_ptr(), c.shift_heatmap, _lib.ptr(avg),
                                                self.center.data_ptr(), self.scale.data_ptr(), self.score.data_ptr(), preds.data_ptr(),
                                                boxes.data_ptr(), idx.data_ptr(), c.n, c.k, c.h, c.w, REFINE_CODE[c.refine], c.use_udp,
                                                c.to_original if to_original is None else to_original, PIXEL_STD, _lib.ptr(self.blur),
                                                c.ks or 11, _lib.stream()), "mp_flip_aggregate_decode")
        return preds, boxes, idx, avg

    def aggregate(self):
        c = self.case
        out = torch.full_like(self.hm, float("nan"))
        _lib.check(LIB.mp_flip_aggregate(self.hm.data_ptr(), self.hf.data_ptr(), self.fi.data_ptr(), out.data_ptr(), c.n, c.k, c.h, c.w,
                                         c.shift_heatmap, _lib.stream()), "mp_flip_aggregate")
        return out


def _check_aggregate(case, d, la, what):
    """the stand-alone aggregation against the oracle's, which is the designed map (tests/test_pose_matrix_cpu.py)"""
    with np.errstate(invalid="ignore"):
        ref_avg = od.flip_aggregate(d["hm"], d["hf"], d["flip_index"], shift_heatmap=bool(case.shift_heatmap))
    avg = la.aggregate()
    _same(avg, ref_avg, f"{what}: mp_flip_aggregate")
    return avg, ref_avg


def _check_plain(case):
    """refine none / shift: everything bit for bit with the oracle"""
    what = str(case)
    d = pm.decode_inputs(case)
    dec = _decoder(case)
    la = _Launch(case, d, dec)
    seen = d["hm"]
    if case.flip:
        _, seen = _check_aggregate(case, d, la, what)
    with np.errstate(invalid="ignore"):
        ref_preds, ref_boxes, ref_idx = od.decode(seen, d["center"], d["scale"], d["score"], pixel_std=PIXEL_STD, to_original=bool(case.to_original),
                                                  shift_coord=case.refine == "shift", use_udp=bool(case.use_udp))
    ref_idx = ref_idx.astype(np.int32)
    assert np.array_equal(ref_idx, d["index"]), what  # the oracle finds the designed arg-max
    runs = []
    if case.flip:
        for with_avg in pm.AVG_FORMS:
            preds, boxes, idx, avg = la.flip_decode(with_avg)
            runs.append((f"C ABI, avg_out {'given' if with_avg else 'NULL'}", preds, boxes, idx))
            if with_avg:
                _same(avg, seen, f"{what}: the materialised average")
        (preds, boxes), avg = dec.decode_flip_aggregated(la.hm, la.hf, la.fi, bool(case.shift_heatmap), la.center, la.scale, la.score,
                                                         return_heatmap=True)
        _same(avg, seen, f"{what}: the wrapper's average")
        runs.append(("wrapper with the average", preds, boxes, dec.last_argmax))
        preds, boxes = dec.decode_flip_aggregated(la.hm, la.hf, la.fi, bool(case.shift_heatmap), la.center, la.scale, la.score)
        runs.append(("wrapper", preds, boxes, dec.last_argmax))
    else:
        runs.append(("C ABI",) + la.decode(la.hm))
        preds, boxes = dec(la.hm, la.center, la.scale, la.score)
        runs.append(("wrapper", preds, boxes, dec.last_argmax))
    for name, preds, boxes, idx in runs:
        _same(idx, ref_idx, f"{what}, {name}: arg-max")
        _same(preds[..., 2], ref_preds[..., 2], f"{what}, {name}: max values")
        _same(boxes, ref_boxes, f"{what}, {name}: boxes")
        _same(preds[..., :2], ref_preds[..., :2], f"{what}, {name}: coordinates")


def _check_dark(case):
    """DARK: intermediates and solve on the map the decoder sees; the entry points agree to the bit; the back-projection is the
    oracle's expression on the kernel's own heat-map coordinates"""
    what = str(case)
    d = pm.decode_inputs(case)
    dec = _decoder(case)
    la = _Launch(case, d, dec)
    seen_t, seen = la.hm, d["hm"]
    if case.flip:
        seen_t, seen = _check_aggregate(case, d, la, what)
    pix = check_dark_intermediates(seen, d["center"], d["scale"], d["score"], dec)  # [n,k,3] in heat-map pixels, arg-max checked inside
    _, ref_boxes, ref_idx = od.decode(seen, d["center"], d["scale"], d["score"], pixel_std=PIXEL_STD, to_original=False)
    ref_idx = ref_idx.astype(np.int32)
    assert np.array_equal(ref_idx, d["index"]), what
    _same(pix[..., 2], np.take_along_axis(seen.reshape(case.n, case.k, -1), ref_idx[..., None].astype(np.int64), axis=2)[..., 0], f"{what}: max values")
    want = pix.copy()
    if case.to_original:
        with np.errstate(invalid="ignore"):
            want[..., :2] = od.transform_preds(pix[..., :2], d["center"], d["scale"], (case.h, case.w), PIXEL_STD, bool(case.use_udp))
    runs = []
    if case.flip:
        # same expression on equal inputs: the fused entry on (hm, hf) and mp_decode_topdown on their average
        plain = la.decode(seen_t, to_original=0)
        _same(plain[0], pix, f"{what}: mp_decode_topdown on the average")
        for with_avg in pm.AVG_FORMS:
            preds, boxes, idx, avg = la.flip_decode(with_avg, to_original=0)
            _same(preds, pix, f"{what}: fused DARK in heat-map pixels, avg_out {'given' if with_avg else 'NULL'}")
            if with_avg:
                _same(avg, seen, f"{what}: the materialised average")
            preds, boxes, idx, _ = la.flip_decode(with_avg)
            runs.append((f"C ABI, avg_out {'given' if with_avg else 'NULL'}", preds, boxes, idx))
        preds, boxes = dec.decode_flip_aggregated(la.hm, la.hf, la.fi, bool(case.shift_heatmap), la.center, la.scale, la.score)
        runs.append(("wrapper", preds, boxes, dec.last_argmax))
    else:
        runs.append(("C ABI",) + la.decode(la.hm))
        preds, boxes = dec(la.hm, la.center, la.scale, la.score)
        runs.append(("wrapper", preds, boxes, dec.last_argmax))
    for name, preds, boxes, idx in runs:
        _same(idx, ref_idx, f"{what}, {name}: arg-max")
        _same(boxes, ref_boxes, f"{what}, {name}: boxes")
        _same(preds, want, f"{what}, {name}: predictions")


_MAP_FORMS = [(h, w, r, ks) for h, w in pm.DECODE_MAPS for r, ks in pm.REFINE_FORMS]


@pytest.mark.parametrize("h,w,refine,ks", _MAP_FORMS, ids=[f"{h}x{w}-{pm.refine_id(r, ks)}" for h, w, r, ks in _MAP_FORMS])
def test_decoder_edges(h, w, refine, ks):
    """one map under one refine form: every row count, without the flip test and with it under both column shifts"""
    mine = [c for c in pm.DECODE_CASES if (c.h, c.w, c.refine, c.ks) == (h, w, refine, ks)]
    assert len(mine) == len(pm.ROW_SHAPES) * len(pm.FLIP_FORMS)
    for case in mine:
        (_check_dark if refine == "dark" else _check_plain)(case)


def test_decoder_refuses_what_it_does_not_serve():
    la = _Launch(pm.DECODE_CASES[0], pm.decode_inputs(pm.DECODE_CASES[0]), _decoder(pm.DECODE_CASES[0]))
    p, b, i = la._outs()
    blur = torch.ones(65 * 65, device=DEV)
    for ks, rc in ((0, -3), (2, -3), (65, -3)):
        assert LIB.mp_decode_topdown(la.hm.data_ptr(), la.center.data_ptr(), la.scale.data_ptr(), la.score.data_ptr(), p.data_ptr(), b.data_ptr(),
                                     i.data_ptr(), 1, 1, 1, 1, _lib.MP_REFINE_DARK, 0, 0, PIXEL_STD, blur.data_ptr(), ks, _lib.stream()) == rc
    assert float(p.max()) == -777.0  # nothing was launched


# ---- targets -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", pm.TARGET_CASES, ids=str)
def test_target_edges(case):
    h, w, sigma = case.h, case.w, float(case.sigma)
    kp = pm.target_keypoints(case)
    n, k, _ = kp.shape
    img = pm.target_image_size(case)
    jw = pm.JOINT_WEIGHTS if case.joint_weights else None
    ref_t, ref_w = ot.generate_target(kp, img, [w, h], sigma, use_udp=bool(case.use_udp), joint_weights=jw)
    tkp = _cuda(kp)
    # the C ABI, on outputs that start as NaN
    patch = None if case.use_udp else _cuda(ot.gaussian_patch(sigma).astype(np.float32))
    tjw = None if jw is None else _cuda(np.asarray(jw, dtype=np.float64))
    target = torch.full((n, k, h, w), float("nan"), device=DEV)
    weight = torch.full((n, k), float("nan"), device=DEV)
    _lib.check(LIB.mp_gaussian_target(tkp.data_ptr(), _lib.ptr(patch), 0 if patch is None else patch.shape[0], _lib.ptr(tjw), target.data_ptr(),
                                      weight.data_ptr(), n, k, h, w, float(case.stride), float(case.stride), sigma, case.use_udp,
                                      _lib.stream()), "mp_gaussian_target")
    cfg = dict(image_size=img, heatmap_size=[w, h])
    if jw is not None:
        cfg["joint_weights"] = jw
    gen = mp.TopDownGenerateTarget(is_train=True, config=cfg, sigma=sigma, use_udp=bool(case.use_udp), use_different_joint_weights=jw is not None)
    assert gen._feat_stride() == (float(case.stride), float(case.stride))
    for name, (t, wt) in (("C ABI", (target, weight)), ("wrapper", gen(tkp))):
        t, wt = t.cpu().numpy(), wt.cpu().numpy()
        _same(wt, ref_w, f"{case}, {name}: weights")
        assert not np.isnan(t).any(), f"{case}, {name}: {int(np.isnan(t).sum())} pixels were never written"
        assert np.array_equal(t != 0, ref_t != 0), f"{case}, {name}: support"
        if not case.use_udp:
            _same(t, ref_t, f"{case}, {name}: values")
        else:
            # exp() in fp64 on the device, rounded to fp32: <= 1 fp32 ulp from numpy's
            ulp = np.abs(t.view(np.int32).astype(np.int64) - ref_t.view(np.int32).astype(np.int64))
            share = float((ulp > 0).sum()) / max(int((ref_t != 0).sum()), 1)
            print(f"{case}, {name}: {int((ulp > 0).sum())} of {int((ref_t != 0).sum())} stamped pixels differ by one ulp (share {share:.2e})")
            assert ulp.max() <= 1, f"{case}, {name}: {int(ulp.max())} ulp"


# ---- JointsMSELoss -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", pm.MSE_HW_SCALAR + pm.MSE_HW_QUAD)
def test_mse_edges(hw):
    worst = 0.0
    for rows, (n, k) in pm.MSE_ROWS.items():
        for weights in pm.MSE_WEIGHTS:
            what = f"hw {hw}, rows {rows}, weights {weights}"
            pred, target, w = pm.mse_inputs(hw, rows, weights)
            tp, tt = _cuda(pred), _cuda(target)
            tw = None if w is None else _cuda(w)
            ref, mag = pm.mse_fwd_ref(pred, target, w)
            tol = pm.mse_fwd_tolerance(hw) * mag
            # forward through the C ABI, twice
            ws_bytes = LIB.mp_joints_mse_workspace_bytes(n, k)
            got = []
            for _ in range(2):
                ws = torch.full((ws_bytes // 4,), float("nan"), device=DEV)
                loss = torch.full((1,), float("nan"), device=DEV)
                _lib.check(LIB.mp_joints_mse_fwd(tp.data_ptr(), tt.data_ptr(), _lib.ptr(tw), loss.data_ptr(), ws.data_ptr(), ws_bytes, n, k, hw,
                                                 _lib.stream()), "mp_joints_mse_fwd")
                got.append(loss.cpu().numpy())
            _same(got[1], got[0], f"{what}: two runs")
            # and through the wrapper, with its autograd backward
            p4 = tp.view(n, k, 1, hw).clone().requires_grad_(True)
            fn = mp.create_loss("joint_mse", use_target_weight=w is not None)
            out = fn(p4, tt.view(n, k, 1, hw), tw.view(n, k) if w is not None else None)
            _same(out.detach().reshape(1), got[0], f"{what}: wrapper forward")
            err = abs(float(got[0][0]) - ref)
            worst = max(worst, err / tol if tol else 0.0)
            assert err <= tol, f"{what}: |{float(got[0][0])!r} - {ref!r}| = {err:.3e} > {tol:.3e}"
            for g in pm.MSE_GRADS:
                want = pm.mse_bwd_restated(pred, target, w, g)
                g64 = pm.mse_bwd_ref(pred, target, w, g)
                assert np.all(np.abs(want.astype(np.float64) - g64) <= pm.MSE_BWD_TOLERANCE * np.abs(g64))
                grad = torch.full((rows, hw), float("nan"), device=DEV)
                tg = None if g is None else torch.tensor([g], dtype=torch.float32, device=DEV)
                _lib.check(LIB.mp_joints_mse_bwd(tp.data_ptr(), tt.data_ptr(), _lib.ptr(tw), _lib.ptr(tg), grad.data_ptr(), n, k, hw,
                                                 _lib.stream()), "mp_joints_mse_bwd")
                _same(grad, want, f"{what}, grad_out {g}: backward")
                gn = grad.cpu().numpy().astype(np.float64)
                assert np.all(np.abs(gn - g64) <= pm.MSE_BWD_TOLERANCE * np.abs(g64)), f"{what}, grad_out {g}: backward against float64"
            p4.grad = None
            (out * 0.375).backward()
            _same(p4.grad.view(rows, hw), pm.mse_bwd_restated(pred, target, w, 0.375), f"{what}: wrapper backward")
    print(f"hw {hw}: worst forward error / bound {worst:.3f}")
