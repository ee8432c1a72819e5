"""GPU parity of the four-wave form of the fp32 Winograd kernel's 64-channel cout tile (csrc/conv_wino_f32.hip,
`conv_wino_f32_kernel<.., 2, true>`: one wave per SIMD, 48 accumulators per wave in AGPRs, the transform and the staging of all 256
threads woven between its MFMAs) against the eight-wave two-team form and the one-team form of the same layer.

Every output element is the same chunk-ordered sum through the same output transform in all three forms, so they must agree BIT FOR
BIT (`torch.equal`), and each is within 2e-5 of the output scale of an fp64 `F.conv2d` reference (the bar of
tests/test_gpu_winograd.py).  Output buffers start as NaN: every element has to be written.  `MP_WINO_WIDE` picks the wave form of
a 64-channel cout tile only, so the wide launches force that tile with `MP_WINO_TEAMS=2` as well."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mindpose_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
KNOBS = ("MP_WINO_TEAMS", "MP_WINO_TILES", "MP_WINO_WIDE")

CASES = [
    # n, cin, cout, h, w
    (2, 16, 64, 8, 24),    # full 48-tile band, 16-byte epilogue, even chunk count
    (2, 24, 128, 16, 12),  # 8-byte epilogue; odd chunk count, so the overrun chunk runs; two cout tiles
    (3, 16, 96, 12, 24),   # second band partial (H % R != 0); second cout tile half used
    (2, 8, 80, 8, 24),     # one chunk; Cout not a multiple of 32
    (5, 32, 64, 8, 6),     # grouped, last group clipped to one image
    (2, 16, 32, 4, 6),     # grouped, second 32-channel group wholly past Cout
]


def _desc(n, cin, cout, h, w, relu):
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=3, kw=3, stride=1, pad_top=1, pad_left=1, conv_h=h, conv_w=w, out_h=h,
                         out_w=w, out_mul=1, out_rep=1, out_off_y=0, out_off_x=0, relu=int(relu), flags=0)


_OPS = {}


def _operands(case, full):
    """Operands and the fp64 reference of a case, computed once and shared (read-only) by its parametrisations."""
    if (case, full) not in _OPS:
        n, cin, cout, h, w = case
        g = torch.Generator().manual_seed(cin * 131 + cout * 7 + h)
        x = torch.randn(n, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        r1 = torch.randn(n, cout, h, w, generator=g) if full else None
        r2 = torch.randn(n, cout, h, w, generator=g) if full else None
        ref = F.conv2d(x.double(), wt.double(), padding=1) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
        for r in (r1, r2):
            if r is not None:
                ref = ref + r.double()
        if full:
            ref = F.relu(ref)
        _OPS[(case, full)] = (x, wt, scale, shift, r1, r2, ref)
    return _OPS[(case, full)]


def _winograd(case, full, ops, monkeypatch, **env):
    """One launch through the C ABI under the given experiment knobs; the knobs are read when the launch is configured."""
    n, cin, cout, h, w = case
    x, wt, scale, shift, r1, r2, _ = ops
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))
    lib = _lib.load()
    d = _desc(n, cin, cout, h, w, full)
    assert lib.mp_conv_winograd_supported(ctypes.byref(d)) == 0
    xd, wd, sc, sh = x.to(DEV), wt.to(DEV), scale.to(DEV), shift.to(DEV)
    r1d, r2d = (None if r is None else r.to(DEV) for r in (r1, r2))
    st = _lib.stream()
    pu = torch.empty(lib.mp_conv_winograd_packed_weight_bytes(cout, cin) // 4, device=DEV)
    _lib.check(lib.mp_conv_winograd_pack_weight(_lib.ptr(wd), _lib.ptr(pu), cout, cin, st), "pack U")
    out = torch.full((n, cout, h, w), float("nan"), device=DEV)
    _lib.check(lib.mp_conv2d_winograd_fwd(ctypes.byref(d), _lib.ptr(xd), _lib.ptr(pu), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(r1d),
                                          _lib.ptr(r2d), _lib.ptr(out), st), "winograd")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tiles", [None, 3], ids=["tiles_auto", "tiles3"])
@pytest.mark.parametrize("full", [False, True], ids=["plain", "res1_res2_relu"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}_{c[1]}to{c[2]}_{c[3]}x{c[4]}")
def test_four_wave_form_is_bit_equal_to_both_other_forms_and_within_fp64_bar(case, full, tiles, monkeypatch):
    """`tiles3`: a workgroup walks three consecutive tiles, so the cout tile (and with an even chunk count the tile seam) changes
    inside its run."""
    ops = _operands(case, full)
    ref = ops[-1]
    wide = _winograd(case, full, ops, monkeypatch, MP_WINO_TEAMS=2, MP_WINO_WIDE=1, MP_WINO_TILES=tiles)
    one = _winograd(case, full, ops, monkeypatch, MP_WINO_TEAMS=1, MP_WINO_TILES=tiles)
    eight = _winograd(case, full, ops, monkeypatch, MP_WINO_TEAMS=2, MP_WINO_WIDE=0, MP_WINO_TILES=tiles)
    assert torch.isfinite(wide).all() and torch.isfinite(one).all() and torch.isfinite(eight).all()
    span = float(ref.abs().max())
    errs = {k: float((o.double().cpu() - ref).abs().max()) / span for k, o in (("four waves", wide), ("one team", one), ("eight waves", eight))}
    print("normalised max error vs fp64: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert all(e <= 2e-5 for e in errs.values()), errs
    assert torch.equal(wide, one)
    assert torch.equal(wide, eight)


def test_hrnet_w32_heatmaps_are_bit_equal_with_the_four_wave_form_forced_on_and_off(monkeypatch):
    """HRNet-W32 at 256x192, N = 2, every Winograd launch on the 64-channel cout tile: the plan recorded with the four-wave form,
    with the eight-wave form and with the four-wave form again give the same heat-map bits, and the recorded cout tile is 64 either
    way.  The tuner's per-shape picks (which layers take the Winograd form at all is its timed choice) are cached per process, so
    all plans run the same kernel family for every layer."""
    import mindpose_amd as mp
    x = torch.randn(2, 3, 256, 192, generator=torch.Generator().manual_seed(5)).to(DEV)
    monkeypatch.delenv("MP_WINO_TILES", raising=False)
    monkeypatch.setenv("MP_WINO_TEAMS", "2")
    outs, tiles = [], []
    for wide in ("1", "0", "1"):
        monkeypatch.setenv("MP_WINO_WIDE", wide)
        net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(DEV).eval()
        outs.append(net(x).clone())
        plan = next(iter(net._plans.values()))
        infos = [plan.entry_info(i) for i in range(len(plan))]
        tiles.append([(e["w"], e["cout_tile"]) for e in infos if e["kind_id"] == 9])
    assert torch.isfinite(outs[0]).all()
    assert tiles[0] == tiles[1] == tiles[2]  # same layers in the Winograd form, same description
    assert all(t == 64 for _, t in tiles[0])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
