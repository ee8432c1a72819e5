"""Every (case, forced variant, knob set) pair of the edge matrix of tests/f16_matrix.py on the fp16 convolution family (csrc/conv_f16*.hip)
through the C ABI: 48 variant ids in four kernel families x every class of tile geometry their configure functions can produce (the
classes are listed, and pinned per variant, in tests/test_f16_matrix_cpu.py).  For each pair, after EACH launch (four
per phase kind):

  * guard bands: the input, the packed weights, scale / shift, both residuals and the output sit inside larger allocations whose
    margins hold the NaN pattern of their type; every margin is bit-unchanged;
  * operands bit-unchanged;
  * written exactly inside the window: the output starts as the fp16 NaN pattern (the 1x1 stride-2 data gradient: zeros at the odd
    positions, which nothing writes, the NaN pattern at the owned ones); every element of the window the launch owns is finite
    afterwards, every element outside it keeps its bits - the other phases' pixels, rows behind a ragged band, images behind a short
    group;
  * the padding channels of the last 8-channel block are exactly zero at the owned pixels;
  * accuracy: against the float64 reference of the launch on the fp16-rounded operands (conv / conv_transpose, scale, shift, the
    residuals, ReLU) at the family's bar of tests/test_gpu_f16.py and test_gpu_bands.py, |got - ref| <= 2^-9 |ref| + 1e-4 max |ref|; a
    failure names the worst element's row band, image group and cout tile and whether each is the last one.  A launch that adds into
    its own output (the phases of the transposed conv's data gradient, res1 == out as `_deconv_backward` passes it) is compared with
    reference partial + the stored sum it read, and repeated out of place (res1 = a copy, a fresh output): same bits;
  * cross-variant: all four kernels walk k as (32-channel step ascending, taps inside) and share the epilogue arithmetic
    (conv_f16_dev.h), so every forced variant gives the bits of the heuristic launch of the same case.
The statistics builds (separate instantiations) run the two statistics tests of tests/test_gpu_bn_fuse.py on fm.STATS_EDGE_CASES.
`mp_f16_pack_weight` modes 0 ... 4 and `mp_f16_pack_weight_batch` are compared bit for bit with a numpy restatement of the layout
[Cin_pad32 / 32][T][4][Cout_pad16][8].
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models.train_ops import _PackJob  # noqa: E402
from tests import f16_matrix as fm  # noqa: E402

DEV = torch.device("cuda:0")
LIB = _lib.load()
NAN32 = 0x7FC00000  # the sentinel bit pattern (a quiet NaN) of guard bands ...
NAN16 = 0x7E00      # ... and of fp16 tensors and unwritten outputs
GUARD = 2048        # elements on either side of every operand (a multiple of 16 bytes: the operands keep their alignment)


class Guarded:
    """A contiguous tensor between two NaN guard bands of one allocation (fp16 or fp32); a tensor made without a value holds the
    sentinel everywhere."""

    def __init__(self, shape, value=None, dtype=torch.float16):
        self.numel = int(np.prod(shape))
        self.itype, self.sentinel = {torch.float32: (torch.int32, NAN32), torch.float16: (torch.int16, NAN16)}[dtype]
        self.buf = torch.empty(self.numel + 2 * GUARD, device=DEV, dtype=dtype)
        self.buf.view(self.itype).fill_(self.sentinel)
        self.t = self.buf[GUARD:GUARD + self.numel].view(shape)
        if value is not None:
            self.t.copy_(value)
        self.start = self.bits().clone()

    def bits(self):
        return self.buf.view(self.itype)

    def inner_bits(self):
        return self.t.view(self.itype)

    def assert_guards(self, what):
        b = self.bits()
        assert bool((b[:GUARD] == self.sentinel).all()) and bool((b[GUARD + self.numel:] == self.sentinel).all()), f"{what}: wrote into a guard band"

    def assert_unchanged(self, what):
        assert torch.equal(self.bits(), self.start), f"{what} was written to"


def _h(x):
    return x.half().double()


def _to_c8(x):
    """[n, c, h, w] -> the channel-blocked layout [n, ceil(c / 8), h, w, 8] in fp16, padding channels zero"""
    n, c, h, w = x.shape
    c8 = (c + 7) // 8
    xp = torch.zeros(n, c8 * 8, h, w, dtype=x.dtype)
    xp[:, :c] = x
    return xp.view(n, c8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().half()


def _from_c8(t):
    """[n, c8, h, w, 8] -> [n, 8 c8, h, w] (all channels, the padding ones included)"""
    n, c8, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, c8 * 8, h, w)


def _source_shape(mode, cout, cin, k):
    """Shape of the fp32 weight a packing mode reads; cout / cin are the PACKED conv's (= the launch's) channel counts."""
    return {0: (cout, cin, k, k), 2: (cin, cout, k, k), 1: (cin, cout, 4, 4), 3: (cin, cout, 3, 3), 4: (cout, cin, 4, 4)}[mode]


@functools.lru_cache(maxsize=4)
def _case_data(kind, case):
    """CPU operands of a case (already rounded to fp16 where the kernel sees fp16) and its float64 reference:
    dict(inputs=[one NCHW tensor per launch], weight (fp32 master), scale, shift, res=[...], partial=[per launch: the launch's own
    conv term, scale / shift applied, or None = a window of `full`], full = the case's result before residuals / ReLU, relu, zero_fill)."""
    la = fm.launches(kind, case)
    d0 = la[0].desc
    cout = d0.cout
    g = torch.Generator().manual_seed(1000 * fm.LDS_KINDS.index(kind) + sum(int(v) for v in case))
    rnd = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    unit = kind not in ("conv", "deconv")  # the data gradients run with scale 1, shift 0 (train_ops.py)
    scale = torch.ones(cout) if unit else torch.rand(cout, generator=g) + 0.5
    shift = torch.zeros(cout) if unit else rnd(cout) * 0.1
    aff = lambda y: y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)  # noqa: E731
    partial, relu, zero_fill = None, False, False
    if kind == "conv":
        n, cin, _, k, s, h, w, relu, _, crop = case
        x, wt = rnd(n, cin, h, w), rnd(cout, cin, k, k) / (cin * k * k) ** 0.5
        full = aff(F.conv2d(_h(x), _h(wt), None, stride=s, padding=k // 2))
        full, inputs = full[..., :full.shape[3] - crop], [x]
    elif kind == "deconv":
        n, cin, _, h, w, relu = case
        x, wt = rnd(n, cin, h, w), rnd(cin, cout, 4, 4) / (cin * 4) ** 0.5
        full, inputs = aff(F.conv_transpose2d(_h(x), _h(wt), None, stride=2, padding=1)), [x] * 4
    elif kind == "dgrad_s1":
        n, cin, co_f, k, h, w, _ = case
        dz, wt = rnd(n, co_f, h, w), rnd(co_f, cin, k, k) / (co_f * k * k) ** 0.5
        full, inputs = F.conv_transpose2d(_h(dz), _h(wt), None, stride=1, padding=k // 2), [dz]
    elif kind in ("dgrad_k3s2", "dgrad_k3s2_merged"):
        n, cin, co_f, h, w = case
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        dz, wt = rnd(n, co_f, ho, wo), rnd(co_f, cin, 3, 3) / (co_f * 9 / 4) ** 0.5
        full = F.conv_transpose2d(_h(dz), _h(wt), None, stride=2, padding=1, output_padding=(h - (2 * ho - 1), w - (2 * wo - 1)))
        inputs = [dz] * len(la)
    elif kind == "dgrad_k1s2":
        n, cin, co_f, h, w = case
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        dz, wt = rnd(n, co_f, ho, wo), rnd(co_f, cin, 1, 1) / co_f ** 0.5
        full = F.conv_transpose2d(_h(dz), _h(wt), None, stride=2, padding=0, output_padding=(h - (2 * ho - 1), w - (2 * wo - 1)))
        inputs, zero_fill = [dz], True
        assert float(full[:, :, 1::2].abs().max()) == 0 and float(full[:, :, :, 1::2].abs().max()) == 0
    else:  # deconv_dgrad: dx = conv(dy; the [cin, cout, 4, 4] weight read as [out, in, 4, 4], stride 2, pad 1), phase by phase
        n, cin, co_f, h, w = case
        dy, wt = rnd(n, co_f, 2 * h, 2 * w), rnd(cin, co_f, 4, 4) / (co_f * 4) ** 0.5
        full = F.conv2d(_h(dy), _h(wt), None, stride=2, padding=1)
        inputs, partial = [], []
        for py, px in fm.PHASES:  # the conv is linear in dy: the phase's term is the conv of dy with the other phases' pixels zeroed
            inputs.append(dy[:, :, py::2, px::2].contiguous())
            only = torch.zeros_like(dy)
            only[:, :, py::2, px::2] = dy[:, :, py::2, px::2]
            partial.append(F.conv2d(_h(only), _h(wt), None, stride=2, padding=1))
        assert float((sum(partial) - full).abs().max()) < 1e-9
    assert tuple(full.shape) == (d0.n, cout, d0.out_h, d0.out_w), (full.shape, kind, case)
    res = [rnd(*full.shape) for _ in range(fm.n_res(kind, case))]
    return dict(inputs=inputs, weight=wt, scale=scale, shift=shift, res=res, full=full, partial=partial, relu=bool(relu), zero_fill=zero_fill)


@functools.lru_cache(maxsize=2)
def _device_case(kind, case):
    """The read-only operands on the device, guard-banded: inputs, packed weights per launch, scale / shift, residuals."""
    data = _case_data(kind, case)
    las = fm.launches(kind, case)
    d0 = las[0].desc
    cout, cin, k = d0.cout, d0.cin, d0.kh
    wd = data["weight"].to(DEV).contiguous()
    assert tuple(wd.shape) == _source_shape(las[0].mode, cout, cin, k)
    halfs = LIB.mp_f16_packed_weight_bytes(cout, cin, k, k) // 2
    packed = []
    for la in las:
        if la.merged:  # the four phase packings are slices (2 py + px) of ONE buffer
            p = Guarded((4 * halfs,))
            for i, (py, px) in enumerate(fm.PHASES):
                _lib.check(LIB.mp_f16_pack_weight(_lib.ptr(wd), p.t[i * halfs:].data_ptr(), cout, cin, k, k, la.mode, py, px, _lib.stream()), "pack")
        else:
            p = Guarded((halfs,))
            _lib.check(LIB.mp_f16_pack_weight(_lib.ptr(wd), _lib.ptr(p.t), cout, cin, k, k, la.mode, la.py, la.px, _lib.stream()), "pack")
        torch.cuda.synchronize()
        p.assert_guards("mp_f16_pack_weight")
        assert not bool((p.inner_bits() == NAN16).any()), "mp_f16_pack_weight left elements unwritten"
        p.start = p.bits().clone()
        packed.append(p)
    inputs, seen = [], {}
    for x in data["inputs"]:  # the phases of one input share one buffer
        if id(x) not in seen:
            c8 = _to_c8(x)
            seen[id(x)] = Guarded(c8.shape, c8)
        inputs.append(seen[id(x)])
    padc = (-cout) % 16
    scale = torch.cat([data["scale"], torch.zeros(padc)])
    shift = torch.cat([data["shift"], torch.zeros(padc)])
    res = []
    for r in data["res"]:
        c8 = _to_c8(r)
        res.append(Guarded(c8.shape, c8))
    return dict(inputs=inputs, packed=packed, scale=Guarded(scale.shape, scale, torch.float32), shift=Guarded(shift.shape, shift, torch.float32),
                res=res)


def _window(d, merged):
    """bool [out_h, out_w]: the output pixels a launch owns"""
    win = torch.zeros(d.out_h, d.out_w, dtype=torch.bool)
    for py, px in (fm.PHASES if merged else [(d.out_off_y, d.out_off_x)]):
        win[py:py + (d.conv_h - 1) * d.out_mul + 1:d.out_mul, px:px + (d.conv_w - 1) * d.out_mul + 1:d.out_mul] = True
    return win


def _where(family, w, la, idx):
    """The tile of output element idx = (n, c, row, column) under the launch words w."""
    n, c, row, col = idx
    d = la.desc
    oy, ox = (row % 2, col % 2) if la.merged else (d.out_off_y, d.out_off_x)
    y, x = (row - oy) // d.out_mul, (col - ox) // d.out_mul
    ct = w["w_buf"] // (w["PK"] * w["ks"] ** 2) if family in ("tile", "mt") else w["Cout_pad16"] // w["n_ct"]
    ty, tn, tc = (y // w["R"] if w["tiles_y"] > 1 else 0), n // w["G"], c // ct
    last = lambda i, m: " (the LAST)" if i == m - 1 and m > 1 else ""  # noqa: E731
    return (f"conv pixel ({y}, {x}) phase ({oy}, {ox}) = row band {ty} of {w['tiles_y']}{last(ty, w['tiles_y'])}, image group {tn} of {w['tiles_n']}"
            f"{last(tn, w['tiles_n'])}, cout tile {tc} of {w['n_ct']}{last(tc, w['n_ct'])}; variant {w['variant']} R {w['R']} G {w['G']} PK {w['PK']} x "
            f"{w['n_chunks']} chunks nbuf {w['nbuf']} tiles/workgroup {w['tiles_per_wg']}")


def _worst(t):
    return tuple(int(v) for v in np.unravel_index(int(t.argmax()), t.shape))


def _launch(d, variant, x, packed, dev, r1, r2, out, what):
    rc = LIB.mp_f16_conv2d_fwd(ctypes.byref(d), variant, _lib.ptr(x.t), _lib.ptr(packed.t), _lib.ptr(dev["scale"].t), _lib.ptr(dev["shift"].t),
                               _lib.ptr(r1.t) if r1 is not None else None, _lib.ptr(r2.t) if r2 is not None else None, _lib.ptr(out.t),
                               _lib.stream())
    _lib.check(rc, what)
    torch.cuda.synchronize()


def _run(family, kind, case, variant, env):
    """All launches of a case under one forced variant with every per-launch check; returns the output's bits (CPU, int16)."""
    data, dev = _case_data(kind, case), _device_case(kind, case)
    full = data["full"]
    n, cout, oh, ow = full.shape
    c8 = (cout + 7) // 8
    shape = (n, c8, oh, ow, 8)
    out = Guarded(shape, torch.zeros(shape) if data["zero_fill"] else None)
    if data["zero_fill"]:  # zeros where nothing writes, as the caller leaves them - and the NaN pattern at the pixels the launch owns
        d0 = fm.launches(kind, case)[0].desc
        out.inner_bits().masked_fill_(_window(d0, False).to(DEV).view(1, 1, oh, ow, 1), NAN16)
    res = dev["res"]
    with fm.knobs(**dict(env)):
        for li, la in enumerate(fm.launches(kind, case)):
            d = la.desc
            what = f"{family} {kind} {case} variant {variant} {dict(env)} launch {li}"
            words = fm.launch_words(d, variant, fm.launch_res(kind, case, la), 0)
            assert words is not None, f"{what}: collected, but the library refuses it"
            r1 = out if la.accumulate else (res[0] if res else None)
            r2 = res[1] if len(res) > 1 else None
            before = out.inner_bits().clone()
            _launch(d, variant, dev["inputs"][li], dev["packed"][li], dev, r1, r2, out, what)
            # margins and operands
            out.assert_guards(f"{what}: output")
            for name, t in [("input", dev["inputs"][li]), ("packed weights", dev["packed"][li]), ("scale", dev["scale"]), ("shift", dev["shift"])] + \
                           [(f"res{i + 1}", t) for i, t in enumerate(res)]:
                t.assert_unchanged(f"{what}: {name}")
            # written exactly inside the window
            win = _window(d, la.merged).to(DEV).view(1, 1, oh, ow, 1)
            after = out.inner_bits()
            moved = (after != before) & ~win
            assert not bool(moved.any()), f"{what}: {int(moved.sum())} elements outside the launch's window changed, first (n, block, row, column, lane) " \
                                          f"{torch.nonzero(moved)[:4].tolist()}"
            got_all = _from_c8(out.t.cpu()).double()                      # [n, 8 c8, oh, ow]
            win4 = _window(d, la.merged).view(1, 1, oh, ow)
            bad = ~torch.isfinite(got_all) & win4
            if bool(bad.any()):
                at = _worst(bad.double())
                raise AssertionError(f"{what}: {int(bad.sum())} owned elements are not finite (never written, or a guard band was read), first at "
                                     f"(n, c, row, column) {at}: {_where(family, words, la, at)}")
            pads = _from_c8(out.inner_bits().cpu())[:, cout:] != 0
            assert not bool((pads & win4).any()), f"{what}: padding channels of the last 8-channel block are not zero at owned pixels"
            # accuracy of this launch
            if data["partial"] is not None:
                prev = _from_c8(before.view(torch.float16).cpu()).double()[:, :cout]
                ref = data["partial"][li] + (prev if la.accumulate else 0)
            else:
                ref = full
                for r in data["res"]:
                    ref = ref + _h(r)
            if data["relu"]:
                ref = F.relu(ref)
            scale_max = float(ref.abs().max())
            err = ((got_all[:, :cout] - ref).abs() - ref.abs() * 2.0 ** -9 - 1e-4 * scale_max) * win4
            if float(err.max()) > 0:
                at = _worst(err)
                raise AssertionError(f"{what}: {int((err > 0).sum())} elements beyond 2^-9 |ref| + 1e-4 max |ref|, worst at (n, c, row, column) {at}: got "
                                     f"{float(got_all[at]):.6g} reference {float(ref[at]):.6g}: {_where(family, words, la, at)}")
            if la.accumulate:  # res1 == out, as _deconv_backward passes it: the out-of-place launch gives the same bits
                copy, fresh = Guarded(shape, before.view(torch.float16)), Guarded(shape)
                _launch(d, variant, dev["inputs"][li], dev["packed"][li], dev, copy, None, fresh, what + " (out of place)")
                copy.assert_unchanged(f"{what}: res1 of the out-of-place launch")
                fresh.assert_guards(f"{what}: output of the out-of-place launch")
                diff = fresh.inner_bits() != after
                assert not bool(diff.any()), f"{what}: out aliasing res1 differs from the out-of-place launch in {int(diff.sum())} elements"
    if data["zero_fill"]:
        bits = _from_c8(out.inner_bits().cpu())
        assert not bool(bits[:, :, 1::2].any()) and not bool(bits[:, :, :, 1::2].any()), "odd positions must stay +0"
    return out.inner_bits().cpu()


@functools.lru_cache(maxsize=None)
def _heuristic_bits(kind, case):
    return _run("tile", kind, case, -1, ())


@pytest.mark.parametrize("family,kind,case,variant,env", fm.edge_params())
def test_pair_vs_fp64_reference_and_heuristic_bits(family, kind, case, variant, env):
    bits = _run(family, kind, case, variant, env)
    base = _heuristic_bits(kind, case)
    diff = bits != base
    if bool(diff.any()):
        la = fm.launches(kind, case)[-1]
        with fm.knobs(**dict(env)):
            words = fm.launch_words(la.desc, variant, fm.launch_res(kind, case, la), 0)
        at5 = _worst(diff.double())  # (n, block, row, column, lane)
        at = (at5[0], at5[1] * 8 + at5[4], at5[2], at5[3])
        raise AssertionError(f"{int(diff.sum())} elements differ from the heuristic launch's bits, first at (n, c, row, column) {at}: "
                             f"{_where(family, words, la, at)}")


# ---- the statistics builds on the same edges --------------------------------------------------------------------------------------

# STATS = 1 / 2 are separate instantiations of every kernel; their `valid` flag guards exactly the lanes behind a ragged row band, of a
# short image group and the padding lanes of a tile.  The two statistics tests of tests/test_gpu_bn_fuse.py - every variant the library
# serves, output bit-equal to the plain launch, partial sums against float64 - run here on fm.STATS_EDGE_CASES, with their assertions
# and knobs as they stand there (tests/test_f16_matrix_cpu.py: with statistics mode 1 the launch words still show the classes).
_STATS_IDS = [f"n{c[0]}_{c[1]}to{c[2]}_k{c[3]}s{c[4]}_{c[5]}x{c[6]}" for c in fm.STATS_EDGE_CASES]


@pytest.mark.parametrize("case", fm.STATS_EDGE_CASES, ids=_STATS_IDS)
def test_statistics_forward_on_the_edge_cases(case, monkeypatch):
    from tests import test_gpu_bn_fuse as bnf
    bnf.test_conv_epilogue_statistics_forward(case, monkeypatch)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", fm.STATS_EDGE_CASES, ids=_STATS_IDS)
def test_statistics_backward_on_the_edge_cases(case, relu, monkeypatch):
    from tests import test_gpu_bn_fuse as bnf
    bnf.test_conv_epilogue_statistics_backward(case, relu, monkeypatch)


# ---- weight packing, bit for bit --------------------------------------------------------------------------------------------------

# cin: 3 (one partial 8-group), 10 (cin % 8 != 0; 10 T 4 bytes is no multiple of 16: the batch kernel's contiguous path must fall back),
# 12 (its first group takes the contiguous 16-byte path at T = 1 and 9, its second the general one), 40 (cin % 32 != 0 on the
# contiguous path), 66 (three k-steps, the last with two channels; 66 T 4 is no multiple of 16 at T = 9); cout 17 / 24 / 40: cout % 16 != 0
PACK_CINS, PACK_COUTS = (3, 10, 12, 40, 66), (17, 24, 40)
PACK_FORMS = [(0, k, 0, 0) for k in (1, 2, 3)] + [(2, k, 0, 0) for k in (1, 2, 3)] + [(f, 2, py, px) for f in (1, 3, 4) for py, px in fm.PHASES]


def _packed_layout(w, mode, cout, cin, k, py, px):
    """numpy restatement of the packed layout [Cin_pad32 / 32][T][4][Cout_pad16][8] in fp16 (t = ty * k + tx, channel ci = 32 q + 8 g +
    j), pad channels zero, values rounded to nearest even.  Which source tap lands in tap (ty, tx), from the maths of each form:
      0  forward conv, w [cout, cin, k, k]:  w[co, ci, ty, tx];
      2  data gradient of a stride-1 conv, w [cin, cout, k, k] (the forward conv's [out, in]): roles swapped, taps mirrored;
      1  phase (py, px) of Conv2dTranspose(4, 2, 1), w [cin, cout, 4, 4]: output row 2m + py takes input row i through kernel row
         2 (m - i) + py + 1, and tap ty reads i = m - 1 + py + ty, so ky = 3 - py - 2 ty;
      4  data gradient of that phase, w [cout, cin, 4, 4] in packed terms: the same taps mirrored (ty -> 1 - ty), roles swapped;
      3  data gradient of a 3x3 stride-2 pad-1 conv, w [cin, cout, 3, 3]: dx row 2a + py takes dz row o through kernel row
         2 (a - o) + py + 1, and tap ty reads o = a + ty, so ky = py + 1 - 2 ty - a tap with ky < 0 does not exist (zero)."""
    cp, kp = (cout + 15) // 16 * 16, (cin + 31) // 32 * 32
    out = np.zeros((kp // 32, k * k, 4, cp, 8), np.float16)
    for ty in range(k):
        for tx in range(k):
            if mode == 0:
                src = w[:, :, ty, tx].T
            elif mode == 2:
                src = w[:, :, k - 1 - ty, k - 1 - tx]
            elif mode == 1:
                src = w[:, :, 3 - py - 2 * ty, 3 - px - 2 * tx]
            elif mode == 4:
                src = w[:, :, 3 - py - 2 * (1 - ty), 3 - px - 2 * (1 - tx)].T
            else:
                ky, kx = py + 1 - 2 * ty, px + 1 - 2 * tx
                if ky < 0 or kx < 0:
                    continue
                src = w[:, :, ky, kx]
            blk = np.zeros((kp, cp), np.float16)
            blk[:cin, :cout] = src.astype(np.float16)  # [ci, co], round to nearest even
            out[:, ty * k + tx] = blk.reshape(kp // 32, 4, 8, cp).transpose(0, 1, 3, 2)
    return out.reshape(-1)


@pytest.mark.parametrize("mode,k,py,px", PACK_FORMS, ids=[f"mode{f}-k{k}-phase{py}{px}" for f, k, py, px in PACK_FORMS])
def test_packed_weight_layout(mode, k, py, px):
    g = torch.Generator().manual_seed(100 * mode + 10 * k + 2 * py + px)
    jobs = []
    for cin in PACK_CINS:
        for cout in PACK_COUTS:
            w = torch.randn(_source_shape(mode, cout, cin, k), generator=g)
            numel = LIB.mp_f16_packed_weight_bytes(cout, cin, k, k) // 2
            assert numel == (cin + 31) // 32 * 32 * k * k * ((cout + 15) // 16 * 16)
            jobs.append((cout, cin, w.to(DEV), Guarded((numel,)), Guarded((numel,)), _packed_layout(w.numpy(), mode, cout, cin, k, py, px)))
    arr = (_PackJob * len(jobs))()
    first = np.zeros(len(jobs) + 1, dtype=np.uint32)
    for i, (cout, cin, wd, single, batch, _) in enumerate(jobs):
        assert wd.data_ptr() % 16 == 0
        _lib.check(LIB.mp_f16_pack_weight(_lib.ptr(wd), _lib.ptr(single.t), cout, cin, k, k, mode, py, px, _lib.stream()), "mp_f16_pack_weight")
        arr[i] = _PackJob(wd.data_ptr(), batch.t.data_ptr(), cout, cin, k, k, mode, py, px, 0)
        first[i + 1] = first[i] + ((cin + 31) // 32 * 4 * ((cout + 15) // 16 * 16) + 255) // 256  # one thread per (8 input channels, cout)
    jobs_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    first_dev = torch.from_numpy(first.view(np.int32)).to(DEV)
    _lib.check(LIB.mp_f16_pack_weight_batch(_lib.ptr(jobs_dev), _lib.ptr(first_dev), len(jobs), int(first[-1]), _lib.stream()), "mp_f16_pack_weight_batch")
    torch.cuda.synchronize()
    for cout, cin, _, single, batch, want in jobs:
        what = f"mode {mode} k {k} phase ({py}, {px}) cin {cin} cout {cout}"
        for name, got in (("mp_f16_pack_weight", single), ("mp_f16_pack_weight_batch", batch)):
            got.assert_guards(f"{name} {what}")
            bits = got.inner_bits().cpu().numpy()
            wrong = np.nonzero(bits != want.view(np.int16))[0]
            cp = (cout + 15) // 16 * 16
            assert wrong.size == 0, f"{name} {what}: {wrong.size} elements differ from the layout, first at flat index {int(wrong[0])} = " \
                                    f"(k-step, tap, group, cout, lane) {np.unravel_index(int(wrong[0]), ((cin + 31) // 32, k * k, 4, cp, 8))}"
