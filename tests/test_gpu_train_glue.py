"""Every case of tests/glue_matrix.py on the device, through the C ABI: the kernels a training step runs between its convolutions
and BatchNorms - the exchange-unit sums and their backward (fp32 and channel-blocked fp16), the fan-in gradient sum, max-pool
forward / backward, the stem weight gradient, the sub-pixel phase gathers, AdamW, scaled AdamW, the four other optimizers and the
overflow check.  Each list has sizes below one block, ragged against the block and the vector width, and just over the launch's grid
cap, where the grid-stride loop takes a second pass with a ragged end.

Every operand and output sits between NaN guard bands (`Guarded` of tests/test_gpu_conv_variants.py) and outputs start as the NaN
sentinel.  After each launch the guards are intact, the inputs are bit-unchanged and every output element was written; a read
outside a tensor shows up as a NaN (or a raised overflow flag) in the result.  What is compared, per entry:

  * exchange-unit sums, fan-in sum, max-pool, gathers: bit for bit, against the kernels' arithmetic restated in IEEE fp32 by torch
    CPU (term order ((base + t1) + t2) + t3, one rounding for fp16), the window loops of glue_matrix, the slice;
  * the sums' backward and the stem weight gradient: against float64 with bounds from the accumulation lengths (stated at each test);
  * optimizers: against the update rules in float64 on fp32 hyper-parameters, at the bars the suite already holds for them.

Max-pool inputs are finite: the references do not pin which element a NaN or two infinities of one window select.  The output
gradients of the max-pool backward lie on a 2^-10 grid, so every fp32 sum of up to four of them is exact and the per-plane sums of
dx and dy agree to the bit.
"""
import ctypes
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from mindpose_amd import _lib  # noqa: E402
from tests import glue_matrix as gm  # noqa: E402
from tests.test_gpu_conv_variants import Guarded  # noqa: E402

DEV = torch.device("cuda:0")
LIB = _lib.load()
F16, F32 = torch.float16, torch.float32
MP_ERR_NULL, MP_ERR_SHAPE, MP_ERR_UNSUPPORTED = -1, -2, -3


def _in(x):
    return Guarded(tuple(x.shape), x, x.dtype)


def _out(shape, dtype=F32):
    return Guarded(tuple(shape), None, dtype)


def _settle(what, ins=(), outs=(), inout=()):
    """after a launch: guards intact everywhere, inputs bit-unchanged, every output element written"""
    torch.cuda.synchronize()
    for i, t in enumerate(ins):
        if t is not None:
            t.assert_guards(f"{what}: input {i}")
            t.assert_unchanged(f"{what}: input {i}")
    for i, t in enumerate(outs):
        t.assert_guards(f"{what}: output {i}")
        t.assert_written(f"{what}: output {i}")
    for i, t in enumerate(inout):
        t.assert_guards(f"{what}: updated tensor {i}")


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _assert_bits(got, want, what):
    """got (device or host) == want (host), bit for bit"""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = _bits(got) != _bits(want)
    if bool(diff.any()):
        at = tuple(int(v) for v in torch.nonzero(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ in their bits, first at {at}: got {got[at].item()!r}, "
                             f"want {want[at].item()!r}")


def _assert_bound(got, ref, bound, what):
    """|got - ref| <= bound element-wise (float64); returns the worst error / bound over the elements whose bound is not 0"""
    err = (got.cpu().double() - ref).abs()
    assert bool(torch.isfinite(err).all()), f"{what}: non-finite values in the result"
    over = err > bound
    ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    print(f"{what}: worst error / bound {ratio:.3f}, max error {float(err.max()):.3e}")
    if bool(over.any()):
        at = tuple(int(v) for v in torch.nonzero(over)[0])
        raise AssertionError(f"{what}: {int(over.sum())} elements over their bound, first at {at}: error {float(err[at]):.3e}, bound "
                             f"{float(bound[at]):.3e}; worst error / bound {ratio:.3f}")
    return ratio


def _case_id(case):
    return "-".join("x".join(str(u) for u in v) if isinstance(v, tuple) else str(v) for v in (case if isinstance(case, tuple) else (case,)))


def _over_cap(entry, case):
    e = gm.ENTRIES[entry]
    return e.units(case) > e.cap


def _subsets(k, everything):
    """which of the 1 + k outputs (dbase, dt_1 ... dt_k) a backward launch gets: every non-empty subset, or (large cases) dbase alone
    and all of them"""
    idx = list(range(k + 1))
    if not everything:
        return [(0,), tuple(idx)]
    return [s for r in range(1, k + 2) for s in itertools.combinations(idx, r)]


# ---- the exchange-unit sum, fp32 and channel-blocked fp16 ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def _fuse_data(case, half):
    """operands of a case on the host: base, terms, dy, and an `out` for the backward's mask that holds exact +0, -0 and negatives"""
    n, c, h, w, scales, _ = case
    g = torch.Generator().manual_seed(gm.seed_of(case, half))
    rnd = gm.randn_h if half else gm.randn
    base, terms = rnd(g, n, c, h, w), [rnd(g, n, c, h // s, w // s) for s in scales]
    return base, terms, rnd(g, n, c, h, w), gm.plant_zeros(rnd(g, n, c, h, w), g)


def _term_args(tensors, scales):
    args = []
    for i in range(3):
        args += [_lib.ptr(tensors[i].t), scales[i]] if i < len(tensors) else [None, 1]
    return args


@pytest.mark.parametrize("case", gm.FUSE32_CASES, ids=_case_id)
def test_fuse_sum_f32(case):
    n, c, h, w, scales, relu = case
    base, terms, _, _ = _fuse_data(case, 0)
    want = gm.fuse_sum_restated(base, terms, scales, relu)
    b, ts, out = _in(base), [_in(t) for t in terms], _out(base.shape)
    what = f"mp_fuse_upsample_sum {case} ({'vector' if w % 4 == 0 else 'scalar'} path)"
    _lib.check(LIB.mp_fuse_upsample_sum(_lib.ptr(b.t), *_term_args(ts, scales), _lib.ptr(out.t), n, c, h, w, relu, _lib.stream()), what)
    _settle(what, [b] + ts, [out])
    _assert_bits(out.t, want, what)


@pytest.mark.parametrize("case", gm.FUSE32_CASES, ids=_case_id)
def test_fuse_sum_f32_bwd(case):
    """float64 block sums of g = dy * (out > 0); an s x s block is summed by one thread in fp32, s^2 additions from 0, each off by at
    most 2^-24 of a partial sum that never exceeds sum |g| of the block: bound s^2 * 2^-24 * sum |g|.  dbase (s = 1) is g itself,
    bit for bit.  relu = 0 runs with out = NULL."""
    n, c, h, w, scales, relu = case
    _, _, dy, outv = _fuse_data(case, 0)
    refs, mags = gm.fuse_sum_bwd_ref(dy, outv, scales, relu)
    g32 = torch.where(outv > 0, dy, torch.zeros_like(dy)) if relu else dy
    d, o = _in(dy), (_in(outv) if relu else None)
    ss = (1,) + tuple(scales)
    worst = 0.0
    for subset in _subsets(len(scales), not _over_cap("mp_fuse_upsample_sum_bwd", case)):
        outs = {k: _out(refs[k].shape) for k in subset}
        ptrs = [_lib.ptr(outs[k].t) if k in outs else None for k in range(4)]
        args = [ptrs[0]]
        for k in range(1, 4):
            args += [ptrs[k], ss[k] if k < len(ss) else 1]
        what = f"mp_fuse_upsample_sum_bwd {case} outputs {subset}"
        _lib.check(LIB.mp_fuse_upsample_sum_bwd(_lib.ptr(d.t), _lib.ptr(o.t) if o else None, *args, n, c, h, w, relu, _lib.stream()), what)
        _settle(what, [d, o], list(outs.values()))
        for k, t in outs.items():
            if ss[k] == 1:
                _assert_bits(t.t, g32, f"{what}: output {k} (scale 1)")
            worst = max(worst, _assert_bound(t.t, refs[k], ss[k] ** 2 * gm.U24 * mags[k], f"{what}: output {k} (scale {ss[k]})"))
    print(f"worst error / bound of the case {worst:.3f}")


def _c8_in(x):
    return _in(gm.to_c8(x))


@pytest.mark.parametrize("case", gm.FUSE16_CASES, ids=_case_id)
def test_fuse_sum_f16(case):
    """bit for bit against fp32 sums in the term order, one rounding; the padding lanes of the last channel block stay +0"""
    n, c, h, w, scales, relu = case
    base, terms, _, _ = _fuse_data(case, 1)
    want = gm.to_c8(gm.fuse_sum_restated(base, terms, scales, relu, half=True))
    b, ts, out = _c8_in(base), [_c8_in(t) for t in terms], _out(want.shape, F16)
    # which kernel serves the case follows from the documented condition alone (glue_matrix.f16_fuse_fast)
    what = f"mp_f16_fuse_upsample_sum {case} ({'fast' if gm.f16_fuse_fast(case) else 'generic'} form)"
    _lib.check(LIB.mp_f16_fuse_upsample_sum(_lib.ptr(b.t), *_term_args(ts, scales), _lib.ptr(out.t), n, c, h, w, relu, _lib.stream()), what)
    _settle(what, [b] + ts, [out])
    _assert_bits(out.t, want, what)
    if c % 8:
        assert not bool(_bits(out.t[:, -1, :, :, c % 8:]).any()), f"{what}: padding lanes are not +0"


@pytest.mark.parametrize("case", gm.fuse16_bwd_cases(), ids=_case_id)
def test_fuse_sum_f16_bwd(case):
    """float64 block sums of the masked fp16 dy; fp32 accumulation of s^2 terms, then ONE rounding to fp16:
    bound 2^-11 * |ref| + s^2 * 2^-24 * sum |g|.  (Every fp16 value is a multiple of 2^-24, so is every exact block sum: a sum in
    fp16's denormal range is held exactly and the relative term needs no absolute floor.)"""
    n, c, h, w, scales, relu = case
    _, _, dy, outv = _fuse_data(case, 1)
    refs, mags = gm.fuse_sum_bwd_ref(dy, outv, scales, relu)
    d, o = _c8_in(dy), (_c8_in(outv) if relu else None)
    ss = (1,) + tuple(scales)
    worst = 0.0
    for subset in _subsets(len(scales), not _over_cap("mp_f16_fuse_upsample_sum_bwd", case)):
        outs = {k: _out((n, gm.c8_of(c)) + tuple(refs[k].shape[2:]) + (8,), F16) for k in subset}
        ptrs = [_lib.ptr(outs[k].t) if k in outs else None for k in range(4)]
        args = [ptrs[0]]
        for k in range(1, 4):
            args += [ptrs[k], ss[k] if k < len(ss) else 1]
        what = f"mp_f16_fuse_upsample_sum_bwd {case} outputs {subset}"
        _lib.check(LIB.mp_f16_fuse_upsample_sum_bwd(_lib.ptr(d.t), _lib.ptr(o.t) if o else None, *args, n, c, h, w, relu, _lib.stream()), what)
        _settle(what, [d, o], list(outs.values()))
        for k, t in outs.items():
            got = t.t.cpu()
            if c % 8:
                assert not bool(_bits(got[:, -1, :, :, c % 8:]).any()), f"{what}: output {k}: padding lanes are not +0"
            bound = gm.U16 * refs[k].abs() + ss[k] ** 2 * gm.U24 * mags[k]
            worst = max(worst, _assert_bound(gm.from_c8(got, c), refs[k], bound, f"{what}: output {k} (scale {ss[k]})"))
    print(f"worst error / bound of the case {worst:.3f}")


# ---- the fan-in sum of gradients -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("half,k,units", gm.SUM_CASES, ids=[f"{'f16' if h else 'f32'}-{k}ops-{u}units" for h, k, u in gm.SUM_CASES])
def test_sum_tensors(half, k, units):
    """fp32: the bits of ((a + b) + c) + d; fp16: that sum formed in fp32 and rounded once.  `out` aliasing an operand (the running sum
    accumulated in place) gives the bits of the out-of-place call."""
    g = torch.Generator().manual_seed(gm.seed_of(half, k, units))
    numel = units * (8 if half else 4)
    ops = [(gm.randn_h(g, numel).half() if half else gm.randn(g, numel)) for _ in range(k)]
    acc = ops[0].float()
    for t in ops[1:]:
        acc = acc + t.float()
    want = acc.half() if half else acc
    dev = [_in(t) for t in ops]
    ptrs = lambda ts: [_lib.ptr(t.t) for t in ts] + [None] * (4 - k)  # noqa: E731
    out = _out((numel,), F16 if half else F32)
    what = f"mp_sum_tensors half {half}, {k} operands, {units} units"
    _lib.check(LIB.mp_sum_tensors(*ptrs(dev), _lib.ptr(out.t), units * 16, half, _lib.stream()), what)
    _settle(what, dev, [out])
    _assert_bits(out.t, want, what)
    for j in sorted({0, k - 1}):  # out aliases the first, then the last operand
        mine = [_in(t) for t in ops]
        _lib.check(LIB.mp_sum_tensors(*ptrs(mine), _lib.ptr(mine[j].t), units * 16, half, _lib.stream()), f"{what}, out aliases operand {j}")
        _settle(what, [t for i, t in enumerate(mine) if i != j], [], [mine[j]])
        _assert_bits(mine[j].t, out.t.cpu(), f"{what}: out aliasing operand {j} against the out-of-place call")


def test_sum_tensors_refusals():
    a, b, d = (_in(torch.ones(64)) for _ in range(3))
    out = _out((64,))
    assert LIB.mp_sum_tensors(_lib.ptr(a.t), _lib.ptr(b.t), None, None, _lib.ptr(out.t), 250, 0, _lib.stream()) == MP_ERR_SHAPE  # bytes % 16
    assert LIB.mp_sum_tensors(_lib.ptr(a.t), _lib.ptr(b.t), None, _lib.ptr(d.t), _lib.ptr(out.t), 256, 0, _lib.stream()) == MP_ERR_NULL  # d, no c
    torch.cuda.synchronize()
    out.assert_unchanged("a refused mp_sum_tensors: out")


# ---- max-pool ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _pool_data(case, kind):
    n, c, h, w = case
    g = torch.Generator().manual_seed(gm.seed_of(case, len(kind)))
    # "ties": small integers, as behind the stem's ReLU, where about half of the pool's inputs are exactly 0 - almost every window ties
    x = gm.randn(g, n, c, h, w) if kind == "randn" else torch.randint(0, 3, (n, c, h, w), generator=g).float()
    oh, ow, _, _ = gm.pool_geometry(h, w)
    dy = (gm.randn(g, n, c, oh, ow) * 1024).round() / 1024
    return x, dy


@pytest.mark.parametrize("kind", gm.POOL_KINDS)
@pytest.mark.parametrize("case", gm.POOL_FWD_CASES, ids=_case_id)
def test_maxpool_fwd(case, kind):
    n, c, h, w = case
    x, _ = _pool_data(case, kind)
    want = gm.maxpool_ref(x)
    xd, out = _in(x), _out(want.shape)
    what = f"mp_maxpool3x3s2_same {case} {kind}"
    _lib.check(LIB.mp_maxpool3x3s2_same(_lib.ptr(xd.t), _lib.ptr(out.t), n, c, h, w, _lib.stream()), what)
    _settle(what, [xd], [out])
    _assert_bits(out.t, want, what)


@pytest.mark.parametrize("kind", gm.POOL_KINDS)
@pytest.mark.parametrize("case", gm.POOL_BWD_CASES, ids=_case_id)
def test_maxpool_bwd(case, kind):
    """the gradient of every window at its FIRST maximum in scan order, bit for bit; it lands exactly once: per plane, sum dx == sum dy"""
    n, c, h, w = case
    x, dy = _pool_data(case, kind)
    want = gm.maxpool_bwd_ref(x, dy)
    xd, dyd, dx = _in(x), _in(dy), _out(x.shape)
    what = f"mp_maxpool3x3s2_same_bwd {case} {kind}"
    _lib.check(LIB.mp_maxpool3x3s2_same_bwd(_lib.ptr(xd.t), _lib.ptr(dyd.t), _lib.ptr(dx.t), n, c, h, w, _lib.stream()), what)
    _settle(what, [xd, dyd], [dx])
    _assert_bits(dx.t, want, what)
    assert torch.equal(dx.t.cpu().double().sum(dim=(2, 3)), dy.double().sum(dim=(2, 3))), f"{what}: a window's gradient is lost or lands twice"


# ---- stem weight gradient ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", gm.STEM_CASES, ids=_case_id)
def test_stem_wgrad(case):
    """A thread adds its ceil(n ho wo / 256) products in fp32 (each product and each addition off by at most 2^-24 of a running sum
    that stays under the thread's sum |dz x|), the block sums the threads in float64, the result is rounded to fp32 once:
    bound (ceil(n ho wo / 256) + 2) * 2^-24 * sum |dz x| per weight.  The reduction order is fixed: two runs agree to the bit."""
    k, cin, cout, n, h, w = case
    g = torch.Generator().manual_seed(gm.seed_of(case))
    ho, wo = (h + 2 * (k // 2) - k) // 2 + 1, (w + 2 * (k // 2) - k) // 2 + 1
    x, dz = gm.randn(g, n, cin, h, w), gm.randn(g, n, cout, ho, wo)
    ref, mag = gm.stem_wgrad_ref(x, dz, k)
    xd, dzd = _in(x), _in(dz)
    runs = [_out(ref.shape), _out(ref.shape)]
    what = f"mp_stem_conv_wgrad {case}"
    for dw in runs:
        _lib.check(LIB.mp_stem_conv_wgrad(_lib.ptr(xd.t), _lib.ptr(dzd.t), _lib.ptr(dw.t), n, cin, h, w, cout, k, _lib.stream()), what)
    _settle(what, [xd, dzd], runs)
    _assert_bound(runs[0].t, ref, (gm.ceil_div(n * ho * wo, 256) + 2) * gm.U24 * mag, what)
    _assert_bits(runs[1].t, runs[0].t.cpu(), f"{what}: second run against the first")


def test_stem_wgrad_refusals():
    x, dz, dw = _in(torch.ones(1, 5, 8, 8)), _in(torch.ones(1, 4, 4, 4)), _out((4, 5, 7, 7))
    assert LIB.mp_stem_conv_wgrad(_lib.ptr(x.t), _lib.ptr(dz.t), _lib.ptr(dw.t), 1, 5, 8, 8, 4, 7, _lib.stream()) == MP_ERR_SHAPE        # cin = 5
    assert LIB.mp_stem_conv_wgrad(_lib.ptr(x.t), _lib.ptr(dz.t), _lib.ptr(dw.t), 1, 4, 8, 8, 4, 5, _lib.stream()) == MP_ERR_UNSUPPORTED  # k = 5
    torch.cuda.synchronize()
    dw.assert_unchanged("a refused mp_stem_conv_wgrad: dw")


# ---- sub-pixel phase gathers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", gm.GATHER_CASES, ids=_case_id)
def test_gather_phase(case):
    """out[n, c, m, k] = x[n, c, 2m + py, 2k + px], a copy: the bits of the slice, on values of every magnitude (denormals, -0)"""
    half, n, c, h, w, py, px = case
    shape = (n, gm.c8_of(c), 2 * h, 2 * w, 8) if half else (n, c, 2 * h, 2 * w)
    numel = 1
    for v in shape:
        numel *= v
    x = gm.pattern_bits(numel, F16 if half else F32).view(shape)
    want = gm.gather_phase_ref(x, py, px, c8=bool(half))
    xd, out = _in(x), _out(want.shape, x.dtype)
    fn, what = (LIB.mp_f16_gather_phase, f"mp_f16_gather_phase {case}") if half else (LIB.mp_gather_phase, f"mp_gather_phase {case}")
    _lib.check(fn(_lib.ptr(xd.t), _lib.ptr(out.t), n, c, h, w, py, px, _lib.stream()), what)
    _settle(what, [xd], [out])
    _assert_bits(out.t, want, what)


def test_gather_phase_refusals():
    for fn, dtype, shape in ((LIB.mp_gather_phase, F32, (1, 3, 4, 4)), (LIB.mp_f16_gather_phase, F16, (1, 1, 4, 4, 8))):
        x, out = _in(torch.ones(shape, dtype=dtype)), _out((1, shape[1], 2, 2) + shape[4:], dtype)
        assert fn(_lib.ptr(x.t), _lib.ptr(out.t), 1, 3, 2, 2, 2, 0, _lib.stream()) == MP_ERR_SHAPE  # phase 2
        assert fn(_lib.ptr(x.t), _lib.ptr(out.t), 1, 3, 2, 2, 0, 2, _lib.stream()) == MP_ERR_SHAPE
        torch.cuda.synchronize()
        out.assert_unchanged("a refused gather: out")


# ---- optimizers ----------------------------------------------------------------------------------------------------------------------

def _rel(got, ref):
    return float((got.cpu().double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=2)
def _adamw_data(count):
    g = torch.Generator().manual_seed(gm.seed_of(count))
    return gm.randn(g, count), gm.randn(g, count), gm.randn(g, count) * 0.1, torch.rand(count, generator=g) * 0.01


def _adamw_args():
    hp = gm.ADAMW_HYPER
    return hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"]


def _assert_adamw(got, ref, what):
    """the bar the suite holds for AdamWeightDecay: 1e-6 of the reference's max abs, on the parameters and both moments"""
    for name, t, r in zip(("param", "exp_avg", "exp_avg_sq"), got, ref):
        err = _rel(t.t, r)
        print(f"{what}: {name} error / max abs {err:.3e} (bar 1e-6)")
        assert err < 1e-6, f"{what}: {name} {err:.3e}"


@pytest.mark.parametrize("count", gm.OPT_COUNTS)
def test_adamw_step(count):
    p, gr, m, v = _adamw_data(count)
    hp = gm.ADAMW_HYPER
    ref = gm.optimizer_ref(0, p, gr, m, v, hp["lr"], 1.0, hp["wd"], (hp["b1"], hp["b2"], hp["eps"]))
    pd, gd, md, vd = (_in(t) for t in (p, gr, m, v))
    what = f"mp_adamw_step count {count}"
    _lib.check(LIB.mp_adamw_step(_lib.ptr(pd.t), _lib.ptr(gd.t), _lib.ptr(md.t), _lib.ptr(vd.t), count, *_adamw_args(), _lib.stream()), what)
    _settle(what, [gd], [], [pd, md, vd])
    _assert_adamw((pd, md, vd), ref, what)


@pytest.mark.parametrize("count", gm.OPT_COUNTS)
def test_adamw_step_scaled(count):
    """against the rule with a gradient scale that is no power of two (skip flag present and 0); with the skip flag set nothing
    changes; with a power-of-two scale the bits of mp_adamw_step on the pre-scaled gradient"""
    p, gr, m, v = _adamw_data(count)
    hp = gm.ADAMW_HYPER
    what = f"mp_adamw_step_scaled count {count}"
    scale = 1.0 / 3.0
    ref = gm.optimizer_ref(0, p, gr, m, v, hp["lr"], scale, hp["wd"], (hp["b1"], hp["b2"], hp["eps"]))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    pd, gd, md, vd = (_in(t) for t in (p, gr, m, v))
    _lib.check(LIB.mp_adamw_step_scaled(_lib.ptr(pd.t), _lib.ptr(gd.t), _lib.ptr(md.t), _lib.ptr(vd.t), count, *_adamw_args(), scale, _lib.ptr(flag),
                                        _lib.stream()), what)
    _settle(what, [gd], [], [pd, md, vd])
    _assert_adamw((pd, md, vd), ref, what)
    # overflow step: the flag is set, parameters and moments keep their bits
    flag.fill_(1)
    pd, md, vd = (_in(t) for t in (p, m, v))
    _lib.check(LIB.mp_adamw_step_scaled(_lib.ptr(pd.t), _lib.ptr(gd.t), _lib.ptr(md.t), _lib.ptr(vd.t), count, *_adamw_args(), scale, _lib.ptr(flag),
                                        _lib.stream()), what)
    _settle(f"{what}, skip flag set", [gd, pd, md, vd])
    assert int(flag) == 1
    # power-of-two scale: g * scale is exact, so the two entries run the same arithmetic
    scale = 2.0 ** -7
    one = [_in(t) for t in (p, gr * scale, m, v)]
    two = [_in(t) for t in (p, gr, m, v)]
    _lib.check(LIB.mp_adamw_step(*[_lib.ptr(t.t) for t in one], count, *_adamw_args(), _lib.stream()), "mp_adamw_step")
    _lib.check(LIB.mp_adamw_step_scaled(*[_lib.ptr(t.t) for t in two], count, *_adamw_args(), scale, None, _lib.stream()), what)
    _settle(what, [one[1], two[1]], [], [one[0], one[2], one[3], two[0], two[2], two[3]])
    for name, a, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), one, two):
        if name != "grad":
            _assert_bits(b.t, a.t.cpu(), f"{what}, scale 2^-7: {name} against mp_adamw_step on the pre-scaled gradient")


@pytest.mark.parametrize("count", gm.OPT_COUNTS)
@pytest.mark.parametrize("name", list(gm.OPT_VARIANTS))
def test_optimizer_step(name, count):
    """kinds 1 ... 4 of mp_optimizer_step against their documented rules, element by element, parameters and states, at the bar of
    tests/test_gpu_train.py for these rules: rtol 2e-5, atol 2e-6"""
    kind, hyper = gm.OPT_VARIANTS[name]
    g = torch.Generator().manual_seed(gm.seed_of(kind, count, len(name)))
    p, gr = gm.randn(g, count), gm.randn(g, count)
    s1 = None if name == "sgd-plain" else (torch.rand(count, generator=g) + 0.1 if kind == 4 else gm.randn(g, count) * 0.1)
    s2 = torch.rand(count, generator=g) * 0.01 if kind == 1 else None
    ref = gm.optimizer_ref(kind, p, gr, s1, s2, gm.OPT_LR, gm.OPT_GRAD_SCALE, gm.OPT_WD, hyper)
    pd, gd = _in(p), _in(gr)
    s1d, s2d = (None if s1 is None else _in(s1)), (None if s2 is None else _in(s2))
    h = (ctypes.c_float * 5)(*hyper)
    what = f"mp_optimizer_step {name} count {count}"
    _lib.check(LIB.mp_optimizer_step(kind, _lib.ptr(pd.t), _lib.ptr(gd.t), _lib.ptr(s1d.t) if s1d else None, _lib.ptr(s2d.t) if s2d else None, count,
                                     gm.OPT_LR, gm.OPT_GRAD_SCALE, gm.OPT_WD, ctypes.byref(h), _lib.stream()), what)
    _settle(what, [gd], [], [t for t in (pd, s1d, s2d) if t is not None])
    for label, t, r in (("param", pd, ref[0]), ("state1", s1d, ref[1]), ("state2", s2d, ref[2])):
        if t is None:
            continue
        got = t.t.cpu().double()
        err = (got - r).abs()
        print(f"{what}: {label} worst error / (2e-6 + 2e-5 |ref|) {float((err / (2e-6 + 2e-5 * r.abs())).max()):.3e}")
        assert torch.allclose(got, r, rtol=2e-5, atol=2e-6), f"{what}: {label} max error {float(err.max()):.3e}"


# ---- the overflow check --------------------------------------------------------------------------------------------------------------

CLEAN = [3.4028234663852886e38, -3.4028234663852886e38, 1e-45, -1e-40, -0.0, 0.0, 1.0, -2.5, 1.17549435e-38]  # FLT_MAX, denormals, -0


def _flag(value=0):
    """the flag between two sentinel words"""
    t = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    t[1] = value
    return t


def _finite(ptr, count, flag):
    rc = LIB.mp_grad_finite_check(ptr, count, flag[1:].data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert int(flag[0]) == 0x5A5A5A5A and int(flag[2]) == 0x5A5A5A5A, "the words next to the flag were written"
    return rc, int(flag[1])


@pytest.mark.parametrize("count", gm.FINITE_COUNTS)
def test_grad_finite_check(count):
    """The gradients lie between NaN guard bands, so a read outside [0, count) raises the flag on clean data.  One inf, -inf or NaN at
    index 0, the last index, every lane of a float4, the scalar tail and (the large count) the second grid pass raises it; FLT_MAX,
    -FLT_MAX, denormals and -0 do not; a flag that is already 1 stays 1."""
    clean = torch.tensor(CLEAN, dtype=F32).repeat(gm.ceil_div(count, len(CLEAN)))[:count]
    gd = _in(clean)
    assert gd.t.data_ptr() % 16 == 0
    what = f"mp_grad_finite_check count {count}"
    assert _finite(_lib.ptr(gd.t), count, _flag(0)) == (0, 0), f"{what}: clean data raised the flag"
    assert _finite(_lib.ptr(gd.t), count, _flag(1)) == (0, 1), f"{what}: a flag that was set did not stay set"
    gd.assert_unchanged(what)
    n4 = count // 4
    spots = {0, count - 1}
    spots.update(range(n4 * 4, count))                                     # the scalar tail
    spots.update(4 * (n4 // 2) + lane for lane in range(4) if n4)         # the four lanes of a float4 in the middle
    spots.update(4 * (n4 - 1) + lane for lane in range(4) if n4)          # ... and of the last one
    if count > gm.FINITE_CAP:
        spots.update({gm.FINITE_CAP - 1, gm.FINITE_CAP, gm.FINITE_CAP + 1, gm.FINITE_CAP + 2, gm.FINITE_CAP + 3})  # around the second pass
    bad = [float("inf"), float("-inf"), float("nan")]
    for j, at in enumerate(sorted(spots)):
        keep = float(gd.t[at])
        gd.t[at] = bad[j % 3]
        got = _finite(_lib.ptr(gd.t), count, _flag(0))
        gd.t[at] = keep
        assert got == (0, 1), f"{what}: {bad[j % 3]} at index {at} (lane {at % 4}, {'tail' if at >= n4 * 4 else 'float4 part'}) was not seen"
    gd.assert_guards(what)


def test_grad_finite_check_arena_slices():
    """a 16-byte-aligned slice in the middle of an arena is checked alone - the non-finite values right before and behind it are not
    read; a pointer that is only 4-byte aligned is refused"""
    count = 1027
    arena = _in(torch.ones(count + 8))
    arena.t[:4] = float("nan")
    arena.t[4 + count:] = float("inf")
    base = arena.t.data_ptr()
    assert _finite(base + 16, count, _flag(0)) == (0, 0)
    assert _finite(base + 16, count + 1, _flag(0)) == (0, 1)  # ... and one element more reaches the inf behind it
    assert _finite(base + 4, count, _flag(0)) == (MP_ERR_UNSUPPORTED, 0)
    assert _finite(base + 16, 0, _flag(0)) == (0, 0)
