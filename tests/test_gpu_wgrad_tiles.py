"""The weight-gradient kernels on workgroups that walk MANY pixel tiles, per kernel instantiation, form and reduce kernel, through the
raw C ABI against the float64 weight gradient (tests/wgrad_matrix.py holds the tables and says what each row reaches).

Per row: the library's split count equals the restated geometry's; workspace and destination start as NaN with 256 sentinel floats
behind each; accumulate = 0 is within the bound of the float64 reference - fp32 5e-5 of its scale (the bound of
test_conv_fwd_dgrad_wgrad_vs_torch), fp16 1e-4 on half-rounded operands with scale = 0.5 (the bound of test_wgrad_f16_vs_torch); a
second launch into fresh buffers is bit-identical; accumulate = 1 adds into what the destination held.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models.act_c8 import ActC8  # noqa: E402
from tests import wgrad_matrix as wm  # noqa: E402

DEV = torch.device("cuda:0")
LIB = _lib.load()
SENTINEL = -7654.5
GUARD = 256
NAN = float("nan")


def _guarded(count, init):
    """[count floats of `init` (a value or a tensor) | GUARD sentinels] on the device."""
    buf = torch.full((count + GUARD,), SENTINEL, device=DEV)
    buf[:count] = init
    return buf


def _intact(buf, count):
    return bool((buf[count:] == SENTINEL).all())


def _to_c8(x):
    n, c, h, w = x.shape
    a = ActC8(n, c, h, w, DEV)
    _lib.check(LIB.mp_f16_to_c8(_lib.ptr(x.to(DEV).contiguous()), _lib.ptr(a), n, c, h, w, _lib.stream()), "to_c8")
    return a


def _five_steps(what, launch, n_slab_floats, count, refs, bound):
    """Steps 2 - 5 of a row.  launch(ws, dws, accumulate) runs the entry point on guarded buffers; refs: one float64 reference per
    destination."""
    def run(accumulate, init):
        ws = _guarded(n_slab_floats, NAN)
        dws = [_guarded(count, i) for i in init]
        launch(ws, dws, accumulate)
        torch.cuda.synchronize()
        assert _intact(ws, n_slab_floats), "wrote behind the workspace"
        assert all(_intact(d, count) for d in dws), "wrote behind the weight gradient"
        return [d[:count].clone() for d in dws]

    first = run(0, [NAN] * len(refs))
    for j, (got, ref) in enumerate(zip(first, refs)):
        err = float((got.cpu().double() - ref.flatten()).abs().max() / ref.abs().max())
        print(f"WGRAD_ERR {what} job{j} {err:.3e} of bound {bound:.0e}")
        assert err <= bound, (j, err)  # (a NaN left in the destination fails this too)
    again = run(0, [NAN] * len(refs))
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "second launch differs"
    g = torch.Generator().manual_seed(count)
    dw0 = [torch.randn(count, generator=g).to(DEV) for _ in refs]
    summed = run(1, dw0)
    assert all(torch.equal(s, d0 + d) for s, d0, d in zip(summed, dw0, first)), "accumulate = 1 is not dw0 + dw"


@pytest.mark.parametrize("case,knobs", [pytest.param(c, k, id=wm.case_id(c, k)) for c, k, _ in wm.F32_CASES])
def test_wgrad_f32_many_tiles_vs_float64(case, knobs, monkeypatch):
    for key, val in knobs.items():
        monkeypatch.setenv(key, val)
    n, cin, cout, k, s, h, w = case
    count = cout * cin * k * k
    d = wm.desc(case)
    nb = LIB.mp_conv_wgrad_workspace_bytes(ctypes.byref(d))
    assert nb // (count * 4) == wm.geometry32(*case, simple=bool(knobs)).splits and nb % (count * 4) == 0
    x, dz, ref = wm.operands(case, False)
    xd, dzd = x.to(DEV), dz.to(DEV)

    def launch(ws, dws, accumulate):
        _lib.check(LIB.mp_conv_wgrad(ctypes.byref(d), _lib.ptr(xd), _lib.ptr(dzd), _lib.ptr(dws[0]), accumulate, _lib.ptr(ws), nb,
                                     _lib.stream()), "wgrad")

    _five_steps(wm.case_id(case, knobs), launch, nb // 4, count, [ref], 5e-5)


@pytest.mark.parametrize("case,knobs", [pytest.param(c, k, id=wm.case_id(c, k)) for c, k, _ in wm.F16_CASES])
def test_wgrad_f16_many_tiles_vs_float64(case, knobs, monkeypatch):
    for key, val in wm.env16(knobs).items():
        monkeypatch.setenv(key, val)
    n, cin, cout, k, s, h, w = case
    count = cout * cin * k * k
    d = wm.desc(case)
    nb = LIB.mp_f16_conv_wgrad_workspace_bytes(ctypes.byref(d))
    assert nb // (count * 4) == wm.geometry16(*case, **wm.geo16_kwargs(knobs)).splits and nb % (count * 4) == 0
    x, dz, ref = wm.operands(case, True)
    xa, dza = _to_c8(x), _to_c8(dz)  # kept alive here: the ABI only sees raw pointers

    def launch(ws, dws, accumulate):
        _lib.check(LIB.mp_f16_conv_wgrad(ctypes.byref(d), _lib.ptr(xa), _lib.ptr(dza), _lib.ptr(dws[0]), 0.5, accumulate, _lib.ptr(ws), nb,
                                         _lib.stream()), "wgrad")

    _five_steps(wm.case_id(case, knobs), launch, nb // 4, count, [ref * 0.5], 1e-4)


@pytest.mark.parametrize("case,knobs,jobs", [pytest.param(c, k, j, id=wm.case_id(c, k)) for c, k, j in wm.F16_GROUPED_CASES])
def test_wgrad_f16_grouped_many_tiles_every_job_vs_float64(case, knobs, jobs, monkeypatch):
    for key, val in wm.env16(knobs).items():
        monkeypatch.setenv(key, val)
    n, cin, cout, k, s, h, w = case
    count = cout * cin * k * k
    d = wm.desc(case)
    nb = LIB.mp_f16_conv_wgrad_grouped_workspace_bytes(ctypes.byref(d), jobs)
    assert nb // (jobs * count * 4) == wm.geometry16(*case, n_jobs=jobs, **wm.geo16_kwargs(knobs)).splits and nb % (jobs * count * 4) == 0
    ops = [wm.operands(case, True, j) for j in range(jobs)]
    xa, dza = [_to_c8(o[0]) for o in ops], [_to_c8(o[1]) for o in ops]
    arr = ctypes.c_void_p * jobs

    def launch(ws, dws, accumulate):
        _lib.check(LIB.mp_f16_conv_wgrad_grouped(ctypes.byref(d), arr(*[_lib.ptr(t) for t in xa]), arr(*[_lib.ptr(t) for t in dza]),
                                                 arr(*[_lib.ptr(t) for t in dws]), jobs, 0.5, accumulate, _lib.ptr(ws), nb, _lib.stream()),
                   "grouped wgrad")

    _five_steps(wm.case_id(case, knobs) + "-grouped", launch, nb // 4, count, [o[2] * 0.5 for o in ops], 1e-4)
