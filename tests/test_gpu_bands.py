"""Column bands: every (band case, kernel variant) pair the library serves, against the UNBANDED layer.

A layer no kernel takes at its full width runs as output-column bands: `mp_col_slice` copies a band's input columns out and the
band's conv writes a column window of the full output (`out_off_x`, `pad_left = 0` on every band but the first).  For each pair of
tests/band_matrix.py, through the C ABI with the variant forced:
  * the output starts as NaN in every element (every fp16 lane of the channel-blocked layout); after EACH band launch everything
    outside the band's window is bit-unchanged, after the last band no NaN remains and the pad channels of the last fp16 block are 0;
  * the assembled output is compared with the whole layer computed by torch on the CPU - fp32: in fp64, normalised max error < 2e-5
    (the bound of test_conv_bn_act_vs_torch); fp16: the fp16-operand / fp32-accumulate oracle, |got - ref| <= 2^-9 |ref| + 1e-4 max|ref|
    per element (the bound of test_conv_f16_vs_oracle);
  * the error is reduced per output column and a failure names the worst column and whether it is the first / last of a band.
Plan level: `Plan.conv` / `Plan.deconv4x4s2` on the map widths of the bottom-up recipe, fp32 and amp O2, tuner on and off.
`mp_col_slice` / `mp_concat_channels` are also tested directly, bit for bit, on both of their code paths.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models import layers as L  # noqa: E402
from mindpose_amd.models.layers import ActC8, BatchNorm2d, Conv2d, Conv2dTranspose, Plan  # noqa: E402
from tests import band_matrix as bm  # noqa: E402

DEV = torch.device("cuda:0")
LIB = _lib.load()
NAN16 = 0x7E00  # fp16 quiet NaN


def _h(x):
    return x.half().float()


def _to_c8(x):
    n, c, h, w = x.shape
    a = ActC8(n, c, h, w, DEV)
    _lib.check(LIB.mp_f16_to_c8(_lib.ptr(x.to(DEV).contiguous()), _lib.ptr(a), n, c, h, w, _lib.stream()), "to_c8")
    return a


@functools.lru_cache(maxsize=4)
def _case_data(kind, case):
    """Operands of a band case (CPU fp32) and the two references of the UNBANDED layer: fp64, and the fp16 oracle (fp16 operands,
    fp32 accumulation and epilogue, one rounding)."""
    g = torch.Generator().manual_seed(sum(int(v) for v in case) + (7 if kind == "conv" else 11))
    if kind == "conv":
        n, cin, cout, k, s, h, w, relu, n_res, _ = case
        wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        layer = lambda x_, w_: F.conv2d(x_, w_, None, stride=s, padding=k // 2)  # noqa: E731
    else:
        n, cin, cout, h, w, relu, _ = case
        n_res = 0
        wt = torch.randn(cin, cout, 4, 4, generator=g) / (cin * 4) ** 0.5
        layer = lambda x_, w_: F.conv_transpose2d(x_, w_, None, stride=2, padding=1)  # noqa: E731
    x = torch.randn(n, cin, h, w, generator=g)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    y = layer(x.double(), wt.double())
    res = [torch.randn(y.shape, generator=g) for _ in range(n_res)]
    ref64 = y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref16 = layer(_h(x), _h(wt)) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    for r in res:
        ref64 = ref64 + r.double()
        ref16 = ref16 + _h(r)
    if relu:
        ref64, ref16 = F.relu(ref64), F.relu(ref16)
    return x, wt, scale, shift, res, ref64, _h(ref16)


def _launches(kind, case):
    """[(py, px, transposed, [(start, width_in, desc)])]: the band launches of a case, one weight packing per group."""
    if kind == "conv":
        return [(0, 0, 0, bm.conv_case_bands(case))]
    return [(py, px, 1, bands) for (py, px), bands in bm.deconv_case_bands(case).items()]


def _window(d, shape):
    """Boolean [H, W] mask of the output pixels a band descriptor writes."""
    m = torch.zeros(shape, dtype=torch.bool, device=DEV)
    m[d.out_off_y::d.out_mul, d.out_off_x:d.out_off_x + (d.conv_w - 1) * d.out_mul + 1:d.out_mul] = True
    return m


def _edges(kind, case):
    """{output column: 'first' / 'last' / 'first and last'} over the bands of a case."""
    out = {}
    for _, _, _, bands in _launches(kind, case):
        for _, _, d in bands:
            first, last = d.out_off_x, d.out_off_x + (d.conv_w - 1) * d.out_mul
            for col, what in ((first, "first"), (last, "last")):
                out[col] = what if out.get(col, what) == what else "first and last"
    return out


def _column_report(err, tol, kind, case):
    """err / tol: [n, c, H, W] - the worst output column, and where it sits in its band."""
    excess = (err - tol).amax(dim=(0, 1, 2))
    col = int(excess.argmax())
    edge = _edges(kind, case).get(col)
    where = f"the {edge} column of a band" if edge else "inside a band"
    bad_cols = [int(c) for c in torch.nonzero(excess > 0).flatten()[:12]]
    return f"worst output column {col} ({where}): error {float(err[..., col].max()):.3e}; columns beyond the bound: {bad_cols}"


def _assert_untouched(before, after, window, what):
    changed = (before != after)  # integer views: bit comparison
    while changed.dim() > 2:
        changed = changed.any(dim=0)
    stray = changed & ~window
    if stray.any():
        ys, xs = torch.nonzero(stray, as_tuple=True)
        raise AssertionError(f"{what}: wrote outside its window at (row, column) {list(zip(ys[:8].tolist(), xs[:8].tolist()))}"
                             f" - {int(stray.sum())} pixels")


def _run_f32(kind, case, variant):
    """``variant``: one forced variant for every band, or {(py, px, band index): variant}."""
    per_band = variant if isinstance(variant, dict) else None
    x, wt, scale, shift, res, ref64, _ = _case_data(kind, case)
    n, cin, h, w = x.shape
    cout, (oh, ow) = ref64.shape[1], ref64.shape[2:]
    xd, wd, sc, sh = x.to(DEV), wt.to(DEV), scale.to(DEV), shift.to(DEV)
    rd = [r.to(DEV) for r in res] + [None, None]
    out = torch.full((n, cout, oh, ow), float("nan"), device=DEV)
    for py, px, transposed, bands in _launches(kind, case):
        d0 = bands[0][2]
        packed = torch.empty(LIB.mp_conv_packed_weight_bytes(cout, cin, d0.kh, d0.kw) // 4, device=DEV)
        _lib.check(LIB.mp_conv_pack_weight(_lib.ptr(wd), _lib.ptr(packed), cout, cin, d0.kh, d0.kw, transposed, py, px, _lib.stream()), "pack")
        for bi, (start, wb, d) in enumerate(bands):
            xb = torch.full((n, cin, h, wb), float("nan"), device=DEV)
            _lib.check(LIB.mp_col_slice(_lib.ptr(xd), _lib.ptr(xb), n * cin * h, w, start, wb, 0, _lib.stream()), "mp_col_slice")
            assert torch.equal(xb, xd[..., start:start + wb]), f"mp_col_slice(start {start}, width {wb}) is not the input's columns"
            before = out.view(torch.int32).clone()
            if per_band is not None:
                variant = per_band[(py, px, bi)]
            rc = LIB.mp_conv2d_fwd_variant(ctypes.byref(d), variant, _lib.ptr(xb), _lib.ptr(packed), _lib.ptr(sc), _lib.ptr(sh),
                                           _lib.ptr(rd[0]), _lib.ptr(rd[1]), _lib.ptr(out), _lib.stream())
            _lib.check(rc, f"mp_conv2d_fwd_variant, variant {variant}, phase ({py}, {px}) band {bi}")
            _assert_untouched(before.view(-1, oh, ow), out.view(torch.int32).view(-1, oh, ow), _window(d, (oh, ow)),
                              f"phase ({py}, {px}) band {bi} (columns {d.out_off_x} + {d.conv_w} x {d.out_mul})")
    got = out.cpu().double()
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} output elements were never written: columns " \
                                       f"{torch.nonzero(torch.isnan(got).any(dim=0).any(dim=0).any(dim=0)).flatten()[:12].tolist()}"
    err = (got - ref64).abs()
    bound = 2e-5 * float(ref64.abs().max())
    assert float(err.max()) < bound, f"normalised max error {float(err.max()) / float(ref64.abs().max()):.3e} >= 2e-5; " + \
        _column_report(err, torch.full_like(err, bound), kind, case)


def _run_f16(kind, case, variant):
    x, wt, scale, shift, res, _, ref16 = _case_data(kind, case)
    n, cin, h, w = x.shape
    cout, (oh, ow) = ref16.shape[1], ref16.shape[2:]
    xa = _to_c8(x)
    ra = [_to_c8(r) for r in res] + [None, None]
    wd = wt.to(DEV)
    padc = (-cout) % 16
    sc, sh = torch.cat([scale, torch.zeros(padc)]).to(DEV), torch.cat([shift, torch.zeros(padc)]).to(DEV)
    out = ActC8(n, cout, oh, ow, DEV)
    out.c8_tensor.view(torch.int16).fill_(NAN16)

    def bits(t):  # [n * c8, H, W, 8] -> [n * c8 * 8, H, W]
        return t.view(torch.int16).view(-1, oh, ow, 8).permute(0, 3, 1, 2).reshape(-1, oh, ow)

    for py, px, transposed, bands in _launches(kind, case):
        d0 = bands[0][2]
        packed = torch.empty(LIB.mp_f16_packed_weight_bytes(cout, cin, d0.kh, d0.kw) // 2, device=DEV, dtype=torch.float16)
        _lib.check(LIB.mp_f16_pack_weight(_lib.ptr(wd), _lib.ptr(packed), cout, cin, d0.kh, d0.kw, transposed, py, px, _lib.stream()), "pack")
        for bi, (start, wb, d) in enumerate(bands):
            xb = ActC8(n, cin, h, wb, DEV)
            xb.c8_tensor.view(torch.int16).fill_(NAN16)
            _lib.check(LIB.mp_col_slice(_lib.ptr(xa), _lib.ptr(xb), n * ((cin + 7) // 8) * h, w, start, wb, 1, _lib.stream()), "mp_col_slice")
            assert torch.equal(xb.c8_tensor.view(torch.int16), xa.c8_tensor[:, :, :, start:start + wb].contiguous().view(torch.int16)), \
                f"mp_col_slice(start {start}, width {wb}, c8) is not the input's columns"
            before = out.c8_tensor.clone()
            rc = LIB.mp_f16_conv2d_fwd(ctypes.byref(d), variant, _lib.ptr(xb), _lib.ptr(packed), _lib.ptr(sc), _lib.ptr(sh),
                                       _lib.ptr(ra[0]), _lib.ptr(ra[1]), _lib.ptr(out), _lib.stream())
            _lib.check(rc, f"mp_f16_conv2d_fwd, variant {variant}, phase ({py}, {px}) band {bi}")
            _assert_untouched(bits(before), bits(out.c8_tensor), _window(d, (oh, ow)),
                              f"phase ({py}, {px}) band {bi} (columns {d.out_off_x} + {d.conv_w} x {d.out_mul})")
    blk = out.c8_tensor.cpu().permute(0, 1, 4, 2, 3).reshape(n, -1, oh, ow).float()
    got = blk[:, :cout]
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} output elements were never written: columns " \
                                       f"{torch.nonzero(torch.isnan(got).any(dim=0).any(dim=0).any(dim=0)).flatten()[:12].tolist()}"
    assert torch.all(blk[:, cout:] == 0), "pad channels of the last 8-channel block are not zero"
    err = (got - ref16).abs()
    tol = ref16.abs() * 2.0 ** -9 + 1e-4 * ref16.abs().max()
    assert not (err > tol).any(), f"{int((err > tol).sum())} of {err.numel()} beyond one fp16 ulp; " + _column_report(err, tol, kind, case)


@pytest.mark.parametrize("kind,case,variant", bm.f32_pairs())
def test_band_case_f32_vs_unbanded_layer(kind, case, variant):
    _run_f32(kind, case, variant)


@pytest.mark.parametrize("kind,case,variant", bm.f16_tile_pairs())
def test_band_case_f16_vs_unbanded_layer(kind, case, variant):
    _run_f16(kind, case, variant)


@pytest.mark.parametrize("groups,kind,case,variant", bm.f16_mt_pairs())
def test_band_case_f16_multi_tile_vs_unbanded_layer(groups, kind, case, variant, monkeypatch):
    monkeypatch.setenv("MP_F16_MT_GROUPS", groups)
    _run_f16(kind, case, variant)


def test_gemm_form_on_the_single_bands_it_accepts():
    """The blocked-GEMM phase form (fp32 variant 10) takes the phase bands whose conv_w equals their input width and no whole case,
    so the matrix above never launches it - the plan's tuner can.  The 64 -> 128 transposed conv in three bands, variant 10 on
    every band that accepts it and the heuristic on the rest, with the same checks as every pair."""
    assign = bm.gemm_band_variants()
    assert 10 in assign.values() and -1 in assign.values(), assign
    _run_f32("deconv", bm.GEMM_BAND_CASE, assign)


# ---- plan level ---------------------------------------------------------------------------------------------------------------

QUARTER_WIDTHS = list(range(128, 209, 16))  # image widths 512 ... 832 at 1/4 scale
HALF_WIDTHS = list(range(256, 417, 32))     # ... at 1/2 scale


def _library_takes(d, half, n_res, tune):
    """Does the plan have a kernel for descriptor ``d`` as ONE entry?  Restated from the library's own answers, not from
    `Plan._conv_served`: with the tuner on and the layer above its MAC threshold any forced variant (or the Winograd form) will do,
    otherwise the entry is recorded with the heuristic, which then has to take it."""
    tuned = tune == "1" and d.n * d.conv_h * d.conv_w * d.cout * d.cin * d.kh * d.kw >= L._TUNE_MIN_MACS
    if half:
        return any(LIB.mp_f16_conv_supported(ctypes.byref(d), v, n_res, 0) == 1 for v in ([-1] + list(range(L.F16_VARIANTS)) if tuned else [-1]))
    if any(LIB.mp_conv_supported(ctypes.byref(d), v) == 1 for v in (range(-1, L.F32_SMALL_WIDE + 1) if tuned else [-1])):
        return True
    return tuned and L.winograd_enabled() and LIB.mp_conv_winograd_supported(ctypes.byref(d)) == 0


def _expected_bands(whole, bands_of, half, n_res, tune):
    """0 when every whole-layer descriptor is taken (``whole`` None: known not to be), else the smallest band count 2 ... 32 at
    which every band is."""
    if whole is not None and all(_library_takes(d, half, n_res, tune) for d in whole):
        return 0
    for nb in range(2, 33):
        if all(_library_takes(d, half, n_res, tune) for d in bands_of(nb)):
            return nb
    raise AssertionError("no band count serves the layer")


def _rand_bn(c, g):
    bn = BatchNorm2d(c)
    with torch.no_grad():
        bn.gamma.copy_(torch.rand(c, generator=g) + 0.5)
        bn.beta.copy_(torch.randn(c, generator=g) * 0.1)
        bn.moving_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.moving_variance.copy_(torch.rand(c, generator=g) + 0.5)
    return bn


def _plan_check(plan, out, ref64, ref16_of, half, what):
    plan.run()
    plan.run()
    torch.cuda.synchronize()
    if half:
        ref = ref16_of()
        err, tol = (out.cpu() - ref).abs(), ref.abs() * 2.0 ** -9 + 1e-4 * ref.abs().max()
        excess = (err - tol).amax(dim=(0, 1, 2))
        assert not (err > tol).any(), f"{what}: {int((err > tol).sum())} of {err.numel()} beyond one fp16 ulp, worst output column {int(excess.argmax())}"
    else:
        err = (out.cpu().double() - ref64).abs()
        nerr = float(err.max() / ref64.abs().max())
        assert nerr < 2e-5, f"{what}: normalised max error {nerr:.3e}, worst output column {int(err.amax(dim=(0, 1, 2)).argmax())}"


def _bn_affine(bn):
    s = bn.gamma.detach() / torch.sqrt(bn.moving_variance.detach() + 1e-5)
    return s, bn.beta.detach() - bn.moving_mean.detach() * s


@pytest.mark.parametrize("tune", ["1", "0"], ids=["tuned", "heuristic"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "ampO2"])
@pytest.mark.parametrize("layer,w", [("block", w) for w in HALF_WIDTHS] + [("final", w) for w in HALF_WIDTHS])
def test_plan_conv_in_bands_vs_unbanded_layer(layer, w, half, tune, monkeypatch):
    """The full-resolution layers of the HigherHRNet head on every map width of the recipe: the BasicBlock conv 32 -> 32 3x3 +
    residual + ReLU and final_layers.1 32 -> 17 1x1 with bias.  The plan must record them whole exactly when the library takes the
    whole-layer descriptor, else in the fewest bands it takes (`_expected_bands`), and the result is the unbanded layer's."""
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", tune)
    n, h = 1, 8
    g = torch.Generator().manual_seed(w + (1 if layer == "block" else 2))
    if layer == "block":
        conv, bn, relu = Conv2d(32, 32, 3, stride=1, padding=1), _rand_bn(32, g), True
        res = torch.randn(n, 32, h, w, generator=g)
    else:
        conv, bn, relu, res = Conv2d(32, 17, 1, stride=1, padding=0, has_bias=True), None, False, None
    cin, cout, k = conv.in_channels, conv.out_channels, conv.kernel_size
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (1.0 / (cin * k * k)) ** 0.5)
        if conv.bias is not None:
            conv.bias.copy_(torch.randn(cout, generator=g))
    x = torch.randn(n, cin, h, w, generator=g)
    scale, shift = _bn_affine(bn) if bn is not None else (torch.ones(cout), conv.bias.detach())

    def ref_of(cast, dt):
        y = F.conv2d(cast(x).to(dt), cast(conv.weight.detach()).to(dt), None, stride=1, padding=k // 2)
        y = y * scale.to(dt).view(1, -1, 1, 1) + shift.to(dt).view(1, -1, 1, 1)
        if res is not None:
            y = y + cast(res).to(dt)
        return F.relu(y) if relu else y

    plan = Plan(DEV, half=half)
    x32, r32 = x.to(DEV), (res.to(DEV) if res is not None else None)  # kept alive: an fp16 plan reads them through its layout entries
    xd = plan.enter(x32)
    rd = plan.enter(r32) if res is not None else None
    whole = _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=1, pad_top=k // 2, pad_left=k // 2, conv_h=h, conv_w=w,
                          out_h=h, out_w=w, out_mul=1, out_rep=1, out_off_y=0, out_off_x=0, relu=int(relu), flags=0)
    n_res = int(res is not None)
    want = _expected_bands([whole], lambda nb: [d for _, _, d in L.conv_column_bands(n, cin, h, w, cout, k, 1, k // 2, relu, nb)], half, n_res, tune)
    first = len(plan.layer_info)
    out = plan.conv(xd, conv, bn, relu=relu, res1=rd)
    kinds = [e["kind"] for e in plan.layer_info[first:]]
    assert kinds == (["col_slice", "conv_f16" if half else "conv"] * want if want else ["conv_f16" if half else "conv"]) or \
        (not want and kinds == ["conv_winograd"]), f"expected {want} bands, recorded {kinds}"
    # what DESIGN.md 4.13 states, independent of any query: the fp32 416-column block runs as three bands (139 / 139 / 138), the
    # 256-column one is taken whole by a tuned variant, under amp O2 the 416-column block needs bands as well
    if layer == "block" and not half and w == 416:
        assert want == 3 and [e["w"] for e in plan.layer_info[first::2]] == [140, 141, 139], plan.layer_info[first:]
    if layer == "block" and not half and w == 256 and tune == "1":
        assert want == 0
    if layer == "block" and half and w == 416:
        assert want >= 2
    if half:
        out = plan.from_c8(out)
    _plan_check(plan, out, ref_of(lambda t: t, torch.float64), lambda: _h(ref_of(_h, torch.float32)), half, f"{layer} w {w}")


@pytest.mark.parametrize("tune", ["1", "0"], ids=["tuned", "heuristic"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "ampO2"])
@pytest.mark.parametrize("w", QUARTER_WIDTHS)
def test_plan_deconv_in_bands_vs_conv_transpose(w, half, tune, monkeypatch):
    """The transposed conv 66 -> 32 of the HigherHRNet head on the 1/4-scale map widths of the recipe (cin not a multiple of 8)."""
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", tune)
    n, cin, cout, h = 1, 66, 32, 8
    g = torch.Generator().manual_seed(w)
    dc = Conv2dTranspose(cin, cout, 4)
    with torch.no_grad():
        dc.weight.copy_(torch.randn(dc.weight.shape, generator=g) * (0.25 / cin) ** 0.5)
    bn = _rand_bn(cout, g)
    scale, shift = _bn_affine(bn)
    x = torch.randn(n, cin, h, w, generator=g)

    def ref_of(cast, dt):
        y = F.conv_transpose2d(cast(x).to(dt), cast(dc.weight.detach()).to(dt), None, stride=2, padding=1)
        return F.relu(y * scale.to(dt).view(1, -1, 1, 1) + shift.to(dt).view(1, -1, 1, 1))

    plan = Plan(DEV, half=half)
    x32 = x.to(DEV)  # kept alive: an fp16 plan reads it through its layout entry
    xd = plan.enter(x32)

    def phase(py, px):
        return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=2, kw=2, stride=1, pad_top=1 - py, pad_left=1 - px, conv_h=h, conv_w=w,
                             out_h=2 * h, out_w=2 * w, out_mul=2, out_rep=1, out_off_y=py, out_off_x=px, relu=1, flags=0)

    phases = [(py, px) for py in (0, 1) for px in (0, 1)]
    whole_ok = all(_library_takes(phase(py, px), half, 0, tune) for py, px in phases)
    first = len(plan.layer_info)
    out = plan.deconv4x4s2(xd, dc, bn, relu=True)
    kinds = [e["kind"] for e in plan.layer_info[first:]]
    name = "deconv_phase_f16" if half else "deconv_phase"
    if whole_ok:
        assert kinds in ([name] * 4, ["deconv_gemm"]), kinds
    else:  # every phase on its own in the fewest bands its kernels take
        want = []
        for py, px in phases:
            nb = _expected_bands(None, lambda nb: [d for _, _, d in L.deconv_phase_column_bands(n, cin, h, w, cout, py, px, True, nb)], half, 0, tune)
            want += ["col_slice", name] * nb
        assert kinds == want, f"expected {want}, recorded {kinds}"
    if w == 208:
        assert not whole_ok, "the 208-column map of the 832-pixel image is what the band path of the transposed conv was written for"
    if w == 128 and tune == "1":
        assert whole_ok, "the 128-column map of the 512-pixel image is taken whole"
    if half:
        out = plan.from_c8(out)
    _plan_check(plan, out, ref_of(lambda t: t, torch.float64), lambda: _h(ref_of(_h, torch.float32)), half, f"deconv w {w}")


# ---- mp_col_slice / mp_concat_channels, bit for bit ---------------------------------------------------------------------------

def _guarded(numel, dtype, guard):
    """NaN-filled buffer of numel + guard elements; the first numel are the op's output."""
    t = torch.empty(numel + guard, device=DEV, dtype=dtype)
    t.view(torch.int16 if dtype == torch.float16 else torch.int32).fill_(NAN16 if dtype == torch.float16 else 0x7FC00000)
    return t


def _is_sentinel(t):
    if t.dtype == torch.float16:
        return bool((t.view(torch.int16) == NAN16).all())
    return bool((t.view(torch.int32) == 0x7FC00000).all())


@pytest.mark.parametrize("rows,w_in,start,w_out", [(24, 40, 0, 13), (24, 40, 27, 13), (24, 40, 17, 1), (24, 40, 0, 40), (7, 3, 2, 1),
                                                    (2 * 32 * 256, 832, 416, 416)],
                         ids=["start0", "to_the_end", "one_column", "everything", "tiny", "grid_stride"])
@pytest.mark.parametrize("c8", [0, 1], ids=["f32", "c8"])
def test_col_slice_bit_exact(rows, w_in, start, w_out, c8):
    """out[r][0, w_out) = in[r][start, start + w_out): window at the left edge, at the right edge, one column wide, the whole row,
    and 16384 x 416 pixels - above the 16384 x 256 the capped grid covers in one pass, so the grid-stride loop runs again."""
    assert (rows * w_out > 16384 * 256) == (rows > 4096)
    lanes = 8 if c8 else 1
    dtype = torch.float16 if c8 else torch.float32
    g = torch.Generator(device=DEV).manual_seed(rows + w_in + start)
    x = torch.randn(rows, w_in, lanes, generator=g, device=DEV).to(dtype)
    out = _guarded(rows * w_out * lanes, dtype, w_out * lanes)  # one guard row past the end
    _lib.check(LIB.mp_col_slice(_lib.ptr(x), _lib.ptr(out), rows, w_in, start, w_out, c8, _lib.stream()), "mp_col_slice")
    torch.cuda.synchronize()
    assert torch.equal(out[:rows * w_out * lanes].view(rows, w_out, lanes), x[:, start:start + w_out])
    assert _is_sentinel(out[rows * w_out * lanes:]), "mp_col_slice wrote past the end of its output"


def test_col_slice_error_paths():
    t = torch.zeros(4096, device=DEV)
    s = _lib.stream()
    for c8 in (0, 1):
        assert LIB.mp_col_slice(_lib.ptr(t), _lib.ptr(t), 4, 10, 8, 3, c8, s) == -2      # start + w_out > w_in
        assert LIB.mp_col_slice(_lib.ptr(t), _lib.ptr(t), 4, 10, -1, 3, c8, s) == -2     # negative start
        assert LIB.mp_col_slice(_lib.ptr(t), _lib.ptr(t), 0, 10, 0, 3, c8, s) == -2      # no rows
        assert LIB.mp_col_slice(_lib.ptr(t), _lib.ptr(t), -4, 10, 0, 3, c8, s) == -2
        assert LIB.mp_col_slice(_lib.ptr(t), _lib.ptr(t), 4, 10, 0, 0, c8, s) == -2      # empty window
        assert LIB.mp_col_slice(_lib.ptr(t), _lib.ptr(t), 4, 0, 0, 1, c8, s) == -2
        assert LIB.mp_col_slice(None, _lib.ptr(t), 4, 10, 0, 3, c8, s) == -1             # MP_ERR_NULL
        assert LIB.mp_col_slice(_lib.ptr(t), None, 4, 10, 0, 3, c8, s) == -1


@pytest.mark.parametrize("n,ca,cb,h,w,offset", [(3, 32, 17, 6, 8, 0), (2, 3, 5, 3, 5, 0), (2, 32, 17, 6, 8, 1), (1, 1, 1, 1, 1, 0)],
                         ids=["wide", "odd_sizes", "pointer_off_by_4", "one_pixel"])
def test_concat_channels_f32_bit_exact(n, ca, cb, h, w, offset):
    """fp32 NCHW: the 16-byte path (every per-image size and pointer a multiple of 16 bytes), the 4-byte path through sizes (ca*h*w
    odd) and through a base pointer off by 4 bytes (a view one float into a buffer)."""
    g = torch.Generator().manual_seed(n + ca + cb)
    a = torch.randn(n, ca, h, w, generator=g)
    b = torch.randn(n, cb, h, w, generator=g)
    abuf = torch.empty(a.numel() + offset, device=DEV)
    ad = abuf[offset:].view(a.shape)
    ad.copy_(a)
    bd = b.to(DEV)
    numel = n * (ca + cb) * h * w
    out = _guarded(numel, torch.float32, w)
    _lib.check(LIB.mp_concat_channels(ad.data_ptr(), ca, _lib.ptr(bd), cb, _lib.ptr(out), n, h, w, 0, _lib.stream()), "mp_concat_channels")
    torch.cuda.synchronize()
    assert torch.equal(out[:numel].view(n, ca + cb, h, w).cpu(), torch.cat([a, b], 1))
    assert _is_sentinel(out[numel:]), "mp_concat_channels wrote past the end of its output"


@pytest.mark.parametrize("n,ca,cb,h,w", [(3, 32, 17, 6, 7), (2, 8, 34, 5, 3), (1, 16, 8, 1, 1), (8, 256, 66, 64, 64)],
                         ids=["head_widths", "cb34", "one_pixel", "large"])
def test_concat_channels_c8_bit_exact(n, ca, cb, h, w):
    """Channel-blocked fp16: ca a multiple of 8, cb not (the zero pad lanes of b's last block become the result's)."""
    g = torch.Generator().manual_seed(n + ca + cb)
    a = torch.randn(n, ca, h, w, generator=g)
    b = torch.randn(n, cb, h, w, generator=g)
    aa, ba = _to_c8(a), _to_c8(b)
    blocks = (ca + cb + 7) // 8
    numel = n * blocks * h * w * 8
    out = _guarded(numel, torch.float16, w * 8)
    _lib.check(LIB.mp_concat_channels(_lib.ptr(aa), ca, _lib.ptr(ba), cb, _lib.ptr(out), n, h, w, 1, _lib.stream()), "mp_concat_channels")
    torch.cuda.synchronize()
    blk = out[:numel].view(n, blocks, h, w, 8).cpu().permute(0, 1, 4, 2, 3).reshape(n, -1, h, w)
    want = _to_c8(torch.cat([a, b], 1)).c8_tensor.cpu().permute(0, 1, 4, 2, 3).reshape(n, -1, h, w)
    assert torch.equal(blk.view(torch.int16), want.view(torch.int16))
    assert torch.all(blk[:, ca + cb:] == 0), "pad lanes of the result's last block are not zero"
    assert torch.equal(blk[:, :ca + cb].float(), _h(torch.cat([a, b], 1)))
    assert _is_sentinel(out[numel:]), "mp_concat_channels wrote past the end of its output"


def test_concat_channels_grid_stride_loop():
    """More 16-byte words than the capped grid covers in one pass (16384 workgroups x 256 threads): 2 x 80 x 128 x 832 floats =
    4.26 M words of 16 bytes, and the same element count through the 4-byte path (pointer off by 4): 17 M words, four passes."""
    n, ca, cb, h, w = 2, 32, 48, 128, 832
    assert n * (ca + cb) * h * w // 4 > 16384 * 256
    g = torch.Generator().manual_seed(5)
    a = torch.randn(n, ca, h, w, generator=g).to(DEV)
    b = torch.randn(n, cb, h, w, generator=g).to(DEV)
    want = torch.cat([a, b], 1)
    numel = want.numel()
    for offset in (0, 1):
        buf = _guarded(numel + offset, torch.float32, w)
        out = buf[offset:]
        _lib.check(LIB.mp_concat_channels(_lib.ptr(a), ca, _lib.ptr(b), cb, out.data_ptr(), n, h, w, 0, _lib.stream()), "mp_concat_channels")
        torch.cuda.synchronize()
        assert torch.equal(out[:numel].view(want.shape), want), f"output pointer offset {offset * 4} bytes"
        assert _is_sentinel(out[numel:]) and _is_sentinel(buf[:offset])


def test_concat_channels_error_paths():
    t = torch.zeros(4096, device=DEV)
    s = _lib.stream()
    assert LIB.mp_concat_channels(_lib.ptr(t), 12, _lib.ptr(t), 8, _lib.ptr(t), 1, 2, 2, 1, s) == -3   # c8: ca % 8 != 0
    assert LIB.mp_concat_channels(_lib.ptr(t), 12, _lib.ptr(t), 8, _lib.ptr(torch.empty(80, device=DEV)), 1, 2, 2, 0, s) == 0  # fine in fp32
    assert LIB.mp_concat_channels(None, 8, _lib.ptr(t), 8, _lib.ptr(t), 1, 2, 2, 0, s) == -1
    assert LIB.mp_concat_channels(_lib.ptr(t), 8, None, 8, _lib.ptr(t), 1, 2, 2, 0, s) == -1
    assert LIB.mp_concat_channels(_lib.ptr(t), 8, _lib.ptr(t), 8, None, 1, 2, 2, 0, s) == -1
    for bad in [dict(n=0), dict(ca=0), dict(cb=-1), dict(h=0), dict(w=-3)]:
        kw = dict(n=1, ca=8, cb=8, h=2, w=2)
        kw.update(bad)
        assert LIB.mp_concat_channels(_lib.ptr(t), kw["ca"], _lib.ptr(t), kw["cb"], _lib.ptr(t), kw["n"], kw["h"], kw["w"], 0, s) == -2, bad
