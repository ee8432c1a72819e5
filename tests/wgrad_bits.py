"""The output bits of the weight-gradient kernels (csrc/conv_wgrad.hip, csrc/wgrad_f16.hip), as digests: what
tests/golden/gen_wgrad_bits.py records on the GPU from the library of the commit a change to those kernels starts from, and what
tests/test_gpu_wgrad_bits.py recomputes.

Cases: every row of the three tables of tests/wgrad_matrix.py under its knobs, on the operands of `wgrad_matrix.operands` (fp16 rows:
half-rounded operands, scale 0.5, as tests/test_gpu_wgrad_tiles.py runs them; grouped rows: every job).  Per row and job two SHA-256:
of dw after accumulate = 0 into a NaN-filled destination, and of dw after accumulate = 1 into the seeded dw0 of that test's
accumulate step.  The kernels sum in a fixed order (the tile test asserts a bit-identical repeat), so a digest is a fair pin: a changed
tile order, split partition, reduce association or an element that is no longer written changes it.
"""
import ctypes
import hashlib

import torch

from mindpose_amd import _lib
from mindpose_amd.models.act_c8 import ActC8
from tests import f16_matrix as fm
from tests import wgrad_matrix as wm

TABLES = {"f32": [(c, k, 1) for c, k, _ in wm.F32_CASES], "f16": [(c, wm.env16(k), 1) for c, k, _ in wm.F16_CASES],
          "f16_grouped": [(c, wm.env16(k), j) for c, k, j in wm.F16_GROUPED_CASES]}


def run_id(table, i):
    case, env, _ = TABLES[table][i]
    return wm.case_id(case, {k.replace("MP_WGRAD16_", ""): v for k, v in env.items()})


def _to_c8(x, dev):
    n, c, h, w = x.shape
    a = ActC8(n, c, h, w, dev)
    _lib.check(_lib.load().mp_f16_to_c8(_lib.ptr(x.to(dev).contiguous()), _lib.ptr(a), n, c, h, w, _lib.stream()), "to_c8")
    return a


def _sha(t):
    return hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def digests(table, i):
    """{"job<j>": [SHA-256 of dw after accumulate = 0, after accumulate = 1 on dw0]} of one row"""
    lib, dev = _lib.load(), torch.device("cuda:0")
    case, env, jobs = TABLES[table][i]
    n, cin, cout, k, s, h, w = case
    count = cout * cin * k * k
    d = wm.desc(case)
    half = table != "f32"
    ops = [wm.operands(case, half, j) for j in range(jobs)]
    xs, dzs = ([_to_c8(o[0], dev) for o in ops], [_to_c8(o[1], dev) for o in ops]) if half else ([o[0].to(dev) for o in ops], [o[1].to(dev) for o in ops])
    arr = ctypes.c_void_p * jobs
    g = torch.Generator().manual_seed(count)
    dw0 = [torch.randn(count, generator=g).to(dev) for _ in range(jobs)]
    out = {f"job{j}": [] for j in range(jobs)}
    with fm.knobs(**env):
        nb = (lib.mp_conv_wgrad_workspace_bytes(ctypes.byref(d)) if table == "f32" else lib.mp_f16_conv_wgrad_workspace_bytes(ctypes.byref(d))
              if table == "f16" else lib.mp_f16_conv_wgrad_grouped_workspace_bytes(ctypes.byref(d), jobs))
        assert nb > 0
        for accumulate in (0, 1):
            ws = torch.full((nb // 4,), float("nan"), device=dev)
            dws = [t.clone() for t in dw0] if accumulate else [torch.full((count,), float("nan"), device=dev) for _ in range(jobs)]
            if table == "f32":
                rc = lib.mp_conv_wgrad(ctypes.byref(d), _lib.ptr(xs[0]), _lib.ptr(dzs[0]), _lib.ptr(dws[0]), accumulate, _lib.ptr(ws), nb, _lib.stream())
            elif table == "f16":
                rc = lib.mp_f16_conv_wgrad(ctypes.byref(d), _lib.ptr(xs[0]), _lib.ptr(dzs[0]), _lib.ptr(dws[0]), 0.5, accumulate, _lib.ptr(ws), nb,
                                           _lib.stream())
            else:
                rc = lib.mp_f16_conv_wgrad_grouped(ctypes.byref(d), arr(*[_lib.ptr(t) for t in xs]), arr(*[_lib.ptr(t) for t in dzs]),
                                                   arr(*[_lib.ptr(t) for t in dws]), jobs, 0.5, accumulate, _lib.ptr(ws), nb, _lib.stream())
            _lib.check(rc, f"{table} {run_id(table, i)} accumulate {accumulate}")
            torch.cuda.synchronize()
            for j, t in enumerate(dws):
                out[f"job{j}"].append(_sha(t))
    return out
