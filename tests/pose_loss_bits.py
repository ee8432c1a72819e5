"""The output bits of the top-down decode, target and loss entries, as digests: what tests/golden/gen_pose_loss_bits.py records from the
library of the commit a change to those kernels starts from, and what tests/test_gpu_pose_loss_bits.py recomputes and compares.

Groups (one record each, the SHA-256 per output name over the group's cases in their listed order):
  decode/<h>x<w>/<refine>   every case of pose_matrix.DECODE_CASES of that map and refine form.  Per case: mp_decode_topdown on the
                            given map; under DARK mp_decode_topdown_debug with its 16 terms per row; under the flip test
                            mp_flip_aggregate_decode with avg_out given and with avg_out NULL.  logf runs on the device, so only a
                            recorded digest pins the DARK terms to the bit.
  target/<case>             mp_gaussian_target on pose_matrix.target_keypoints, plain and UDP.
  loss/hw<hw>               mp_joints_mse_fwd / _bwd and mp_joints_ohkm_fwd / _bwd on pose_matrix.mse_inputs for every row count and
                            weight kind, grad_out NULL and given, all on 16-byte aligned bases.  The OHKM row sums of a case must BE the
                            MSE row partials of that case (asserted while recording and while comparing).
  masked/<view>             JointsMSELossWithMask forward and backward on the three views of tests/test_gpu_bottomup_loss.py with fp32,
                            uint8 and bool masks, and with an fp32 mask of non-binary values: the kernels multiply by the mask under
                            fp contraction, so a change of the contraction setting shows there.
  ae                        AELoss forward and backward on the inputs of test_ae_random_cases.

An output with NaNs is recorded as the digest of its other values and the index runs [start, stop) of the NaNs, so that a NaN's payload
cannot matter.
"""
import hashlib

import numpy as np
import torch

import mindpose_amd as mp
from mindpose_amd import _lib
from oracle import target as ot
from tests import pose_matrix as pm

DEV = "cuda:0"
PIXEL_STD = 200.0
REFINE_CODE = {"none": _lib.MP_REFINE_NONE, "shift": _lib.MP_REFINE_SHIFT, "dark": _lib.MP_REFINE_DARK}
MASK_VIEWS = ("contiguous", "strided", "odd")
MASK_KINDS = ("float32", "uint8", "bool", "fraction")

GROUPS = [f"decode/{h}x{w}/{pm.refine_id(r, ks)}" for h, w in pm.DECODE_MAPS for r, ks in pm.REFINE_FORMS] + \
         [f"target/{'-'.join(str(v) for v in c)}" for c in pm.TARGET_CASES] + \
         [f"loss/hw{hw}" for hw in pm.MSE_HW_SCALAR + pm.MSE_HW_QUAD] + [f"masked/{v}" for v in MASK_VIEWS] + ["ae"]


def ohkm_topk(k):
    return (k + 1) // 2


class _Record:
    """name -> the bytes of every output recorded under it, in order"""

    def __init__(self):
        self.parts = {}

    def add(self, name, t):
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        self.parts.setdefault(name, []).append(np.ascontiguousarray(a).reshape(-1))

    def digests(self):
        out = {}
        for name, parts in self.parts.items():
            kinds = {p.dtype for p in parts}
            assert len(kinds) == 1, (name, kinds)
            a = np.concatenate(parts)
            nan = np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, dtype=bool)
            if nan.any():
                edges = np.flatnonzero(np.diff(np.concatenate(([0], nan.view(np.int8), [0]))))
                out[name] = {"finite": hashlib.sha256(a[~nan].tobytes()).hexdigest(), "nan": edges.reshape(-1, 2).tolist()}
            else:
                out[name] = hashlib.sha256(a.tobytes()).hexdigest()
        return out


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _decode(rec, lib, h, w, refine, ks):
    for case in pm.DECODE_CASES:
        if (case.h, case.w, case.refine, case.ks) != (h, w, refine, ks):
            continue
        d = pm.decode_inputs(case)
        dec = mp.create_decoder("topdown_heatmap", pixel_std=PIXEL_STD, dark_udp_refine=refine == "dark", kernel_size=ks or 11).to(DEV)
        blur = dec._blur_on(torch.device(DEV))
        hm, center, scale, score = (_cuda(d[key]) for key in ("hm", "center", "scale", "score"))
        n, k = case.n, case.k

        def outs():
            return (torch.full((n, k, 3), -777.0, device=DEV), torch.full((n, 6), -777.0, device=DEV),
                    torch.full((n, k), -777, dtype=torch.int32, device=DEV))

        tail = (n, k, h, w, REFINE_CODE[refine], case.use_udp, case.to_original, PIXEL_STD, _lib.ptr(blur), ks or 11)
        preds, boxes, idx = outs()
        _lib.check(lib.mp_decode_topdown(hm.data_ptr(), center.data_ptr(), scale.data_ptr(), score.data_ptr(), preds.data_ptr(), boxes.data_ptr(),
                                         idx.data_ptr(), *tail, _lib.stream()), "mp_decode_topdown")
        for name, t in (("preds", preds), ("boxes", boxes), ("argmax", idx)):
            rec.add(name, t)
        if refine == "dark":
            preds, boxes, idx = outs()
            terms = torch.full((n * k, 16), -777.0, device=DEV)
            _lib.check(lib.mp_decode_topdown_debug(hm.data_ptr(), center.data_ptr(), scale.data_ptr(), score.data_ptr(), preds.data_ptr(),
                                                   boxes.data_ptr(), idx.data_ptr(), *tail, terms.data_ptr(), _lib.stream()), "mp_decode_topdown_debug")
            for name, t in (("preds", preds), ("boxes", boxes), ("argmax", idx), ("dark_terms", terms)):
                rec.add(name, t)
        if case.flip:
            hf, fi = _cuda(d["hf"]), torch.tensor(d["flip_index"], dtype=torch.int32, device=DEV)
            for with_avg in pm.AVG_FORMS:
                preds, boxes, idx = outs()
                avg = torch.full_like(hm, -777.0) if with_avg else None
                _lib.check(lib.mp_flip_aggregate_decode(hm.data_ptr(), hf.data_ptr(), fi.data_ptr(), case.shift_heatmap, _lib.ptr(avg), center.data_ptr(),
                                                        scale.data_ptr(), score.data_ptr(), preds.data_ptr(), boxes.data_ptr(), idx.data_ptr(), *tail,
                                                        _lib.stream()), "mp_flip_aggregate_decode")
                for name, t in (("preds", preds), ("boxes", boxes), ("argmax", idx)) + ((("avg_out", avg),) if with_avg else ()):
                    rec.add(name, t)


def _target(rec, lib, case):
    kp = pm.target_keypoints(case)
    n, k, _ = kp.shape
    sigma = float(case.sigma)
    patch = None if case.use_udp else _cuda(ot.gaussian_patch(sigma).astype(np.float32))
    jw = _cuda(np.asarray(pm.JOINT_WEIGHTS, dtype=np.float64)) if case.joint_weights else None
    target = torch.full((n, k, case.h, case.w), -777.0, device=DEV)
    weight = torch.full((n, k), -777.0, device=DEV)
    _lib.check(lib.mp_gaussian_target(_cuda(kp).data_ptr(), _lib.ptr(patch), 0 if patch is None else patch.shape[0], _lib.ptr(jw), target.data_ptr(),
                                      weight.data_ptr(), n, k, case.h, case.w, float(case.stride), float(case.stride), sigma, case.use_udp,
                                      _lib.stream()), "mp_gaussian_target")
    rec.add("target", target)
    rec.add("weight", weight)


def _loss(rec, lib, hw):
    for rows, (n, k) in pm.MSE_ROWS.items():
        for weights in pm.MSE_WEIGHTS:
            pred, target, w = pm.mse_inputs(hw, rows, weights)
            tp, tt = _cuda(pred), _cuda(target)
            tw = None if w is None else _cuda(w)
            assert tp.data_ptr() % 16 == 0 and tt.data_ptr() % 16 == 0
            ws_bytes = lib.mp_joints_mse_workspace_bytes(n, k)
            ws = torch.full((ws_bytes // 4,), -777.0, device=DEV)
            loss = torch.full((1,), -777.0, device=DEV)
            _lib.check(lib.mp_joints_mse_fwd(tp.data_ptr(), tt.data_ptr(), _lib.ptr(tw), loss.data_ptr(), ws.data_ptr(), ws_bytes, n, k, hw, _lib.stream()),
                       "mp_joints_mse_fwd")
            rec.add("mse_loss", loss)
            rec.add("mse_partial", ws[:rows])
            topk = ohkm_topk(k)
            ows_bytes = lib.mp_joints_ohkm_workspace_bytes(n, k)
            ows = torch.zeros(ows_bytes // 8, dtype=torch.float64, device=DEV)
            row_sum = torch.full((rows,), -777.0, device=DEV)
            sel = torch.full((rows,), 77, dtype=torch.uint8, device=DEV)
            _lib.check(lib.mp_joints_ohkm_fwd(tp.data_ptr(), tt.data_ptr(), _lib.ptr(tw), loss.data_ptr(), row_sum.data_ptr(), sel.data_ptr(), ows.data_ptr(),
                                              ows_bytes, n, k, hw, topk, _lib.stream()), "mp_joints_ohkm_fwd")
            rec.add("ohkm_loss", loss)
            rec.add("ohkm_row_sum", row_sum)
            rec.add("ohkm_sel", sel)
            assert torch.equal(row_sum.view(torch.int32), ws[:rows].view(torch.int32)), f"hw {hw}, rows {rows}, weights {weights}: OHKM row sums differ from the MSE row partials"
            for g in pm.MSE_GRADS:
                tg = None if g is None else torch.tensor([g], dtype=torch.float32, device=DEV)
                grad = torch.full((rows, hw), -777.0, device=DEV)
                assert grad.data_ptr() % 16 == 0
                _lib.check(lib.mp_joints_mse_bwd(tp.data_ptr(), tt.data_ptr(), _lib.ptr(tw), _lib.ptr(tg), grad.data_ptr(), n, k, hw, _lib.stream()),
                           "mp_joints_mse_bwd")
                rec.add("mse_grad", grad)
                grad = torch.full((rows, hw), -777.0, device=DEV)
                _lib.check(lib.mp_joints_ohkm_bwd(tp.data_ptr(), tt.data_ptr(), _lib.ptr(tw), sel.data_ptr(), _lib.ptr(tg), grad.data_ptr(), n, k, hw, topk,
                                                  _lib.stream()), "mp_joints_ohkm_bwd")
                rec.add("ohkm_grad", grad)


def _masked(rec, view):
    from tests.test_gpu_bottomup_loss import _mse_case  # the views of test_masked_mse_fwd_bwd; that module needs a GPU to import

    stage, target_full, mask_full, si, k, h, w = _mse_case(view)
    for kind in MASK_KINDS:
        if kind == "fraction":  # multiples of 0.1 in [0, 1]: most are no dyadic fraction, so (d * d) * m rounds
            m = (torch.randint(0, 11, mask_full.shape, generator=torch.Generator().manual_seed(7)).float() * 0.1).to(DEV)
        else:
            m = mask_full.to(DEV).to(getattr(torch, kind))
        s = stage.to(DEV).requires_grad_(True)
        t = target_full.to(DEV)
        loss = mp.JointsMSELossWithMask()(s[:, :k], t[:, si, :, :h, :w], m[:, si, :h, :w])
        (loss * 1.7).backward()
        rec.add("loss", loss.reshape(1))
        rec.add("grad", s.grad)


def _ae(rec):
    from tests.test_gpu_bottomup_loss import ae_random_inputs

    for _, pred, ind, weights, tag_per_joint in ae_random_inputs():
        p = pred.to(DEV).requires_grad_(True)
        out = mp.AELoss(tag_per_joint=tag_per_joint)(p, torch.as_tensor(ind).to(DEV))
        (out * torch.tensor(weights, device=DEV)).sum().backward()
        rec.add("out", out)
        rec.add("grad", p.grad)


def digest(group):
    """{output name: record} of one group of GROUPS"""
    lib = _lib.load()
    rec = _Record()
    kind, _, rest = group.partition("/")
    if kind == "decode":
        hw, _, form = rest.partition("/")
        h, w = (int(v) for v in hw.split("x"))
        refine, ks = next(f for f in pm.REFINE_FORMS if pm.refine_id(*f) == form)
        _decode(rec, lib, h, w, refine, ks)
    elif kind == "target":
        _target(rec, lib, next(c for c in pm.TARGET_CASES if "-".join(str(v) for v in c) == rest))
    elif kind == "loss":
        _loss(rec, lib, int(rest[2:]))
    elif kind == "masked":
        _masked(rec, rest)
    else:
        assert group == "ae"
        _ae(rec)
    torch.cuda.synchronize()
    return rec.digests()
