"""GPU parity of the workgroup forms of the fp32 Winograd kernel (csrc/conv_wino_f32.hip) that a launch can take for one and the same
layer: the two-team workgroup on image-grouped bands (W % 4 != 0 maps: `conv_wino_f32_kernel<1,false,true,2>`, both teams share
the grouped raw planes and V, every thread transforms ONE tile) against the one-team form.

Every output element is the same chunk-ordered sum through the same output transform in either form, so the forms must agree BIT FOR
BIT (`torch.equal`), and each is within 2e-5 of the output scale of an fp64 `F.conv2d` reference (the bar of
tests/test_gpu_winograd.py).  Output buffers start as NaN: every element has to be written."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mindpose_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")

GROUPED = [
    # n, cin, cout, h, w, relu, res1, res2
    (5, 256, 256, 8, 6, True, True, False),   # branch 3 of HRNet-W32: four images per band, the last group clipped to one image
    (2, 16, 32, 4, 6, True, False, True),     # one 64-channel cout tile whose second team is wholly past Cout; group clipped to N
    (3, 8, 16, 4, 10, False, True, False),    # one chunk, 10 tiles per image (30 of 48 tile slots), second team and second half empty
    (4, 64, 96, 8, 6, True, True, False),     # second cout tile half used: its second team has nothing
]


def _desc(n, cin, cout, h, w, relu):
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=3, kw=3, stride=1, pad_top=1, pad_left=1, conv_h=h, conv_w=w, out_h=h,
                         out_w=w, out_mul=1, out_rep=1, out_off_y=0, out_off_x=0, relu=int(relu), flags=0)


def _operands(case):
    n, cin, cout, h, w, relu, has_r1, has_r2 = case
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + h)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    r1 = torch.randn(n, cout, h, w, generator=g) if has_r1 else None
    r2 = torch.randn(n, cout, h, w, generator=g) if has_r2 else None
    ref = F.conv2d(x.double(), wt.double(), padding=1) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    for r in (r1, r2):
        if r is not None:
            ref = ref + r.double()
    if relu:
        ref = F.relu(ref)
    return x, wt, scale, shift, r1, r2, ref


def _winograd(case, ops, monkeypatch, **env):
    """One launch through the C ABI under the given experiment knobs; the knobs are read when the launch is configured."""
    n, cin, cout, h, w, relu = case[:6]
    x, wt, scale, shift, r1, r2, _ = ops
    for k in ("MP_WINO_TEAMS", "MP_WINO_TILES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))
    lib = _lib.load()
    d = _desc(n, cin, cout, h, w, relu)
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
@pytest.mark.parametrize("case", GROUPED, ids=lambda c: f"n{c[0]}_{c[1]}to{c[2]}_{c[3]}x{c[4]}")
def test_grouped_two_team_form_is_bit_equal_to_one_team_and_within_fp64_bar(case, tiles, monkeypatch):
    """MP_WINO_TEAMS=2 forces the two-team workgroup on image-grouped bands (by itself only taken from 128 such workgroups on);
    `tiles3`: a workgroup walks three consecutive (cout tile, image group) units, so the cout tile changes inside its run."""
    ops = _operands(case)
    ref = ops[-1]
    one = _winograd(case, ops, monkeypatch, MP_WINO_TEAMS=1, MP_WINO_TILES=tiles)
    two = _winograd(case, ops, monkeypatch, MP_WINO_TEAMS=2, MP_WINO_TILES=tiles)
    assert torch.isfinite(one).all() and torch.isfinite(two).all()
    span = float(ref.abs().max())
    err_one = float((one.double().cpu() - ref).abs().max()) / span
    err_two = float((two.double().cpu() - ref).abs().max()) / span
    print(f"normalised max error vs fp64: one team {err_one:.3e}, two teams {err_two:.3e}")
    assert err_one <= 2e-5 and err_two <= 2e-5, (err_one, err_two)
    assert torch.equal(one, two)


def test_headline_sized_grouped_launch_takes_two_teams_by_itself(monkeypatch):
    """256 -> 256 at 8x6 with N = 128 (128 two-team workgroups) takes the two-team form without any knob, N = 64 does not, and
    MP_CONV_SHARES_CUS (the training step's launches) keeps one team: read back from a recorded plan entry's cout tile."""
    from mindpose_amd.models.layers import Plan
    for k in ("MP_WINO_TEAMS", "MP_WINO_TILES"):
        monkeypatch.delenv(k, raising=False)
    lib = _lib.load()
    c, h, w = 256, 8, 6
    pu = torch.zeros(lib.mp_conv_winograd_packed_weight_bytes(c, c) // 4, device=DEV)
    ones = torch.ones(c, device=DEV)
    tiles = []
    for n, flags in ((128, 0), (64, 0), (128, _lib.MP_CONV_SHARES_CUS)):
        d = _desc(n, c, c, h, w, True)
        d.flags = flags
        x, out = torch.zeros(n, c, h, w, device=DEV), torch.empty(n, c, h, w, device=DEV)
        plan = Plan(DEV)
        _lib.check(lib.mp_plan_add_conv_winograd(plan.handle, ctypes.byref(d), _lib.ptr(x), _lib.ptr(pu), _lib.ptr(ones), _lib.ptr(ones),
                                                 None, None, _lib.ptr(out)), "mp_plan_add_conv_winograd")
        buf = (ctypes.c_int64 * 12)()
        _lib.check(lib.mp_plan_entry_info(plan.handle, 0, buf), "mp_plan_entry_info")
        assert buf[0] == 9
        tiles.append(int(buf[6]))
    assert tiles == [64, 32, 32]


def test_hrnet_w32_heatmaps_are_bit_equal_with_the_two_team_forms_forced_on_and_off(monkeypatch):
    """HRNet-W32 at 256x192, N = 2: the plan recorded with every Winograd launch forced to two teams (the image-grouped 8x6 layers
    of branch 3 included) and the plan with every one forced to one team give the same heat-map bits.  The tuner's per-shape
    picks are cached per process, so both plans run the same kernel family for every layer."""
    import mindpose_amd as mp
    x = torch.randn(2, 3, 256, 192, generator=torch.Generator().manual_seed(5)).to(DEV)
    outs, tiles = [], []
    for teams in ("2", "1", "2"):
        monkeypatch.setenv("MP_WINO_TEAMS", teams)
        net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(DEV).eval()
        outs.append(net(x).clone())
        plan = next(iter(net._plans.values()))
        infos = [plan.entry_info(i) for i in range(len(plan))]
        tiles.append([(e["w"], e["cout_tile"]) for e in infos if e["kind_id"] == 9])
    assert torch.isfinite(outs[0]).all()
    assert [w for w, _ in tiles[0]] == [w for w, _ in tiles[1]]  # same layers in the Winograd form both ways
    assert all(t == 64 for _, t in tiles[0]) and all(t == 32 for _, t in tiles[1])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
