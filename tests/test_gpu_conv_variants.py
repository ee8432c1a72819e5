"""Every (case, variant) pair of tests/f32_matrix.py on the fp32 direct convolution (csrc/conv_mfma.h), through the C ABI with the
variant forced: eight tile variants x every epilogue branch, tile edge, staging width and weight packing the training and inference
paths reach (the classes are listed, and pinned per variant, in tests/test_f32_matrix_cpu.py).  For each pair:

  * guard-banded operands: input, residuals, scale / shift and the output sit inside larger allocations whose bands hold NaN (the
    output itself starts as the same NaN bit pattern), so a read outside a tensor turns up as a NaN in the result, a stale or
    missing write as an unwritten element, and neither leaves its allocation;
  * written only inside its window: after EACH launch (four per phase kind) everything outside the descriptor's output window - the
    other phases' pixels, the guard bands - is bit-unchanged and every element inside it was written; the operands are bit-unchanged;
  * accuracy: against the fp64 reference of the kind at the single-layer bar of tests/test_gpu_conv.py, 2e-5 of the reference's max
    abs; a failure names the worst (row, column), the tile it falls in and whether that is the last row tile / image group;
  * in place: with a residual the launch is repeated with `out` aliasing `res1` (the accumulate form) - same bits;
  * cross-variant: the eight tile variants walk k in one order (cin quad ascending, taps inside; the chunk size does not reorder
    it) and share the epilogue arithmetic, so every tile variant gives the heuristic's bits exactly.
`mp_conv_pack_weight` is compared for its five layouts with a numpy restatement of [Cin_pad4 / 4][T][4][Cout_pad16], bit for bit, and
with `mp_conv_pack_weight_batch` over the same jobs.
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
from tests import f32_matrix as fm  # noqa: E402
from tests.test_gpu_bands import _assert_untouched, _window  # noqa: E402

DEV = torch.device("cuda:0")
LIB = _lib.load()
NAN32 = 0x7FC00000  # the sentinel bit pattern (a quiet NaN) of guard bands and unwritten outputs
NAN16 = 0x7E00      # ... of fp16 tensors
GUARD = 1024        # elements on either side of every operand (a multiple of 16 bytes: the operands keep their alignment)
BAR = 2e-5          # single-layer bound of tests/test_gpu_conv.py, relative to the reference's max abs


class Guarded:
    """A contiguous tensor between two NaN guard bands of one allocation: fp32 (the default) or, for the channel-blocked fp16
    activations, fp16 - every element of the bands, and of a tensor made without a value, holds the quiet-NaN sentinel of its type."""

    def __init__(self, shape, value=None, dtype=torch.float32):
        self.numel = int(np.prod(shape))
        self.itype, self.sentinel = {torch.float32: (torch.int32, NAN32), torch.float16: (torch.int16, NAN16)}[dtype]
        self.buf = torch.empty(self.numel + 2 * GUARD, device=DEV, dtype=dtype)
        self.buf.view(self.itype).fill_(self.sentinel)
        self.t = self.buf[GUARD:GUARD + self.numel].view(shape)
        if value is not None:
            self.t.copy_(value)
        self.start = self.buf.view(self.itype).clone()

    def bits(self):
        return self.buf.view(self.itype)

    def assert_guards(self, what):
        b = self.bits()
        assert bool((b[:GUARD] == self.sentinel).all()) and bool((b[GUARD + self.numel:] == self.sentinel).all()), \
            f"{what}: wrote into a guard band"

    def assert_unchanged(self, what):
        assert torch.equal(self.bits(), self.start), f"{what} was written to"

    def assert_written(self, what):
        left = self.bits()[GUARD:GUARD + self.numel] == self.sentinel
        assert not bool(left.any()), f"{what}: {int(left.sum())} elements were never written, first at flat index {int(torch.nonzero(left)[0])}"


@functools.lru_cache(maxsize=4)
def _case_data(kind, case):
    """CPU operands of a case and its fp64 reference: dict(inputs=[one per launch], weight, pack=(cout, cin, k) in packed terms,
    scale, shift, res=[...], ref, zero_fill)."""
    g = torch.Generator().manual_seed(1000 * [k for k, _ in fm.KINDS].index(kind) + sum(int(v) for v in case))
    rnd = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    la = fm.launches(kind, case)
    d0 = la[0].desc
    cout = d0.cout
    unit = kind not in ("conv", "up", "deconv")  # the data gradients run with scale 1, shift 0 (train_ops.py)
    scale = torch.ones(cout) if unit else torch.rand(cout, generator=g) + 0.5
    shift = torch.zeros(cout) if unit else rnd(cout) * 0.1
    aff = lambda y: y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)  # noqa: E731
    zero_fill = False
    if kind == "conv":
        n, cin, _, k, s, h, w, relu, _ = case
        x, wt = rnd(n, cin, h, w), rnd(cout, cin, k, k) / (cin * k * k) ** 0.5
        ref, inputs, pack = aff(F.conv2d(x.double(), wt.double(), None, stride=s, padding=k // 2)), [x], (cout, cin, k)
    elif kind == "up":
        n, cin, _, h, w, f = case
        x, wt = rnd(n, cin, h, w), rnd(cout, cin, 1, 1) / cin ** 0.5
        ref, relu = F.interpolate(aff(F.conv2d(x.double(), wt.double())), scale_factor=f, mode="nearest"), True
        inputs, pack = [x], (cout, cin, 1)
    elif kind == "deconv":
        n, cin, _, h, w, relu = case
        x, wt = rnd(n, cin, h, w), rnd(cin, cout, 4, 4) / (cin * 4) ** 0.5
        ref, inputs, pack = aff(F.conv_transpose2d(x.double(), wt.double(), None, stride=2, padding=1)), [x] * 4, (cout, cin, 2)
    elif kind == "dgrad_s1":
        n, cin, co_f, k, h, w, _ = case
        dz, wt, relu = rnd(n, co_f, h, w), rnd(co_f, cin, k, k) / (co_f * k * k) ** 0.5, False
        ref, inputs, pack = F.conv_transpose2d(dz.double(), wt.double(), None, stride=1, padding=k // 2), [dz], (cin, co_f, k)
    elif kind == "dgrad_k3s2":
        n, cin, co_f, h, w = case
        dz, wt, relu = rnd(n, co_f, h // 2, w // 2), rnd(co_f, cin, 3, 3) / (co_f * 9 / 4) ** 0.5, False
        ref = F.conv_transpose2d(dz.double(), wt.double(), None, stride=2, padding=1, output_padding=1)
        inputs, pack = [dz] * 4, (cin, co_f, 2)
    elif kind == "dgrad_k1s2":
        n, cin, co_f, h, w = case
        dz, wt, relu = rnd(n, co_f, h // 2, w // 2), rnd(co_f, cin, 1, 1) / co_f ** 0.5, False
        ref = F.conv_transpose2d(dz.double(), wt.double(), None, stride=2, padding=0, output_padding=1)
        inputs, pack, zero_fill = [dz], (cin, co_f, 1), True
        assert float(ref[:, :, 1::2].abs().max()) == 0 and float(ref[:, :, :, 1::2].abs().max()) == 0
    else:  # deconv_dgrad
        n, cin, co_f, h, w = case
        dy, wt, relu = rnd(n, co_f, 2 * h, 2 * w), rnd(cin, co_f, 4, 4) / (co_f * 4) ** 0.5, False
        ref = F.conv2d(dy.double(), wt.double(), None, stride=2, padding=1)  # the [cin, cout, 4, 4] weight read as [out, in, 4, 4]
        inputs, pack = [dy[:, :, py::2, px::2].contiguous() for py, px in fm.PHASES], (cin, co_f, 2)
    assert tuple(ref.shape) == (d0.n, cout, d0.out_h, d0.out_w), (ref.shape, kind, case)
    res = [rnd(*ref.shape) for _ in range(fm.n_res(kind, case))]
    for r in res:
        ref = ref + r.double()
    if relu:
        ref = F.relu(ref)
    return dict(inputs=inputs, weight=wt, pack=pack, scale=scale, shift=shift, res=res, ref=ref, zero_fill=zero_fill)


@functools.lru_cache(maxsize=2)
def _device_case(kind, case):
    """The read-only operands on the device, guard-banded, and the packed weights of every launch."""
    data = _case_data(kind, case)
    cout, cin, k = data["pack"]
    wd = data["weight"].to(DEV)
    packed = []
    for la in fm.launches(kind, case):
        p = torch.full((LIB.mp_conv_packed_weight_bytes(cout, cin, k, k) // 4,), float("nan"), device=DEV)
        _lib.check(LIB.mp_conv_pack_weight(_lib.ptr(wd), _lib.ptr(p), cout, cin, k, k, la.transposed, la.py, la.px, _lib.stream()), "pack")
        packed.append(p)
    inputs, seen = [], {}
    for x in data["inputs"]:  # the phases of one input share one buffer
        if id(x) not in seen:
            seen[id(x)] = Guarded(x.shape, x)
        inputs.append(seen[id(x)])
    return dict(inputs=inputs, packed=packed, scale=Guarded(data["scale"].shape, data["scale"]), shift=Guarded(data["shift"].shape, data["shift"]))


def _run(kind, case, variant, in_place=False):
    """All launches of a case under one forced variant, with the window / guard checks after each; returns the output (device)."""
    data, dev = _case_data(kind, case), _device_case(kind, case)
    ref = data["ref"]
    n, cout, oh, ow = ref.shape
    res = [Guarded(r.shape, r) for r in data["res"]]
    if in_place:
        out = res[0]
    else:
        out = Guarded(ref.shape, torch.zeros(ref.shape) if data["zero_fill"] else None)
    for li, la in enumerate(fm.launches(kind, case)):
        d = la.desc
        r1 = out if la.accumulate else (res[0] if res else None)
        r2 = res[1] if len(res) > 1 else None
        before = out.bits().clone()
        what = f"{kind} {case} variant {variant} launch {li}"
        rc = LIB.mp_conv2d_fwd_variant(ctypes.byref(d), variant, _lib.ptr(dev["inputs"][li].t), _lib.ptr(dev["packed"][li]), _lib.ptr(dev["scale"].t),
                                       _lib.ptr(dev["shift"].t), _lib.ptr(r1.t) if r1 else None, _lib.ptr(r2.t) if r2 else None, _lib.ptr(out.t),
                                       _lib.stream())
        _lib.check(rc, what)
        torch.cuda.synchronize()
        out.assert_guards(what)
        win = _window(d, (oh, ow))
        if d.out_rep > 1:  # every conv pixel covers out_rep x out_rep outputs
            assert d.out_rep == d.out_mul and d.out_off_y == 0 and d.out_off_x == 0
            win = torch.ones_like(win)
        inner = lambda b: b[GUARD:GUARD + out.numel].view(-1, oh, ow)  # noqa: E731
        _assert_untouched(inner(before), inner(out.bits()), win, what)
        if not (in_place or la.accumulate or data["zero_fill"]):
            unwritten = (inner(out.bits()) == NAN32) & win
            assert not bool(unwritten.any()), f"{what}: {int(unwritten.sum())} elements of the window were never written, first (plane, row, column) " \
                                              f"{torch.nonzero(unwritten)[:6].tolist()}"
    for name, t in [(f"input {i}", t) for i, t in enumerate(dev["inputs"])] + [("scale", dev["scale"]), ("shift", dev["shift"])] + \
                   [(f"res{i + 1}", t) for i, t in enumerate(res) if t is not out]:
        t.assert_unchanged(f"{kind} {case} variant {variant}: {name}")
    return out.t


def _where(kind, case, variant, idx):
    """The tile of output element idx = (n, c, row, column) under the variant's geometry."""
    n, c, row, col = idx
    for li, la in enumerate(fm.launches(kind, case)):
        d = la.desc
        if d.out_rep == 1 and ((row - d.out_off_y) % d.out_mul or (col - d.out_off_x) % d.out_mul):
            continue
        geo = fm.geometry(d, variant)
        if geo is None:
            return f"launch {li} (not a tile variant of the direct kernel)"
        y, x = (row - d.out_off_y) // d.out_mul, (col - d.out_off_x) // d.out_mul
        ty, tn, tc = y // geo["R"] if geo["tiles_y"] > 1 else 0, n // geo["G"], c // geo["ct"]
        return (f"launch {li}: conv pixel ({y}, {x}) = row tile {ty} of {geo['tiles_y']}{' (the LAST)' if ty == geo['tiles_y'] - 1 and geo['tiles_y'] > 1 else ''}"
                f", image group {tn} of {geo['tiles_n']}{' (the LAST)' if tn == geo['tiles_n'] - 1 and geo['tiles_n'] > 1 else ''}, cout tile {tc} of "
                f"{geo['n_ct']}; R {geo['R']} G {geo['G']} CK {geo['CK']} x {geo['n_chunks']} chunks, {'vector' if geo['vec_staging'] else 'scalar'} staging, "
                f"epilogue {geo['epilogue']}, tile variant {geo['variant']}")
    return "outside every launch's window"


def _worst(t):
    return tuple(int(v) for v in np.unravel_index(int(t.argmax()), t.shape))


def _branches(kind, case, variant):
    return [(fm.geometry(la.desc, variant) or {}).get("epilogue") for la in fm.launches(kind, case)]


@functools.lru_cache(maxsize=2)
def _heuristic_output(kind, case):
    return _run(kind, case, -1).clone()


@pytest.mark.parametrize("kind,case,variant", fm.pairs())
def test_pair_vs_fp64_reference(kind, case, variant):
    ref = _case_data(kind, case)["ref"]
    out = _run(kind, case, variant)
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all()), f"{int((~torch.isfinite(got)).sum())} non-finite outputs (a guard band was read, or an element never " \
                                            f"written), first at {_worst((~torch.isfinite(got)).double())}: {_where(kind, case, variant, _worst((~torch.isfinite(got)).double()))}"
    err = (got - ref).abs()
    nerr = float(err.max()) / float(ref.abs().max())
    print(f"normalised max error {nerr:.3e}")
    assert nerr < BAR, f"normalised max error {nerr:.3e} >= {BAR} at (n, c, row, column) {_worst(err)}: {_where(kind, case, variant, _worst(err))}"
    if kind == "dgrad_k1s2":
        bits = out.view(torch.int32)
        assert not bool(bits[:, :, 1::2].any()) and not bool(bits[:, :, :, 1::2].any()), "odd positions must stay +0"
    if fm.n_res(kind, case):
        aliased = _run(kind, case, variant, in_place=True)
        diff = out.view(torch.int32) != aliased.view(torch.int32)
        assert not bool(diff.any()), f"out aliasing res1 differs from the out-of-place launch in {int(diff.sum())} elements, first at " \
                                     f"{_worst(diff.double().cpu())}: {_where(kind, case, variant, _worst(diff.double().cpu()))}"
    if variant in fm.TILE_VARIANTS:
        base = _heuristic_output(kind, case)
        diff = (out.view(torch.int32) != base.view(torch.int32)).cpu()
        if bool(diff.any()):
            at = _worst(diff.double())
            raise AssertionError(f"{int(diff.sum())} elements differ from the heuristic's bits (max |difference| {float((out - base).abs().max()):.3e}), first at "
                                 f"{at}: {_where(kind, case, variant, at)}; epilogue branches here {_branches(kind, case, variant)}, of the heuristic "
                                 f"{_branches(kind, case, -1)}")


# ---- weight packing, bit for bit --------------------------------------------------------------------------------------------------

PACK_CINS, PACK_COUTS = (3, 10, 66), (17, 24, 40)
PACK_FORMS = [(0, k, 0, 0) for k in (1, 2, 3)] + [(2, k, 0, 0) for k in (1, 2, 3)] + [(f, 2, py, px) for f in (1, 3, 4) for py, px in fm.PHASES]


def _source_shape(form, cout, cin, k):
    """Shape of the weight a packing form reads; cout / cin are the PACKED conv's (= the launch's) channel counts."""
    return {0: (cout, cin, k, k), 2: (cin, cout, k, k), 1: (cin, cout, 4, 4), 3: (cin, cout, 3, 3), 4: (cout, cin, 4, 4)}[form]


def _packed_layout(w, form, cout, cin, k, py, px):
    """numpy restatement of the packed layout [Cin_pad4 / 4][T][4][Cout_pad16] (t = ty * k + tx, channel ci = 4 * quad + lane),
    pad channels zero.  Which source tap lands in tap (ty, tx), from the maths of each form:
      0  forward conv, w [cout, cin, k, k]:  w[co, ci, ty, tx];
      2  data gradient of a stride-1 conv, w [cin, cout, k, k] (the forward conv's [out, in]): roles swapped, taps mirrored;
      1  phase (py, px) of Conv2dTranspose(4, 2, 1), w [cin, cout, 4, 4]: output row 2m + py takes input row i through kernel row
         2 (m - i) + py + 1, and tap ty reads i = m - 1 + py + ty, so ky = 3 - py - 2 ty;
      4  data gradient of that phase, w [cout, cin, 4, 4] in packed terms: the same taps mirrored (ty -> 1 - ty), roles swapped;
      3  data gradient of a 3x3 stride-2 pad-1 conv, w [cin, cout, 3, 3]: dx row 2a + py takes dz row o through kernel row
         2 (a - o) + py + 1, and tap ty reads o = a + ty, so ky = py + 1 - 2 ty - a tap with ky < 0 does not exist (zero)."""
    cp, kp = (cout + 15) // 16 * 16, (cin + 3) // 4 * 4
    out = np.zeros((kp // 4, k * k, 4, cp), np.float32)
    for ty in range(k):
        for tx in range(k):
            if form == 0:
                src = w[:, :, ty, tx].T
            elif form == 2:
                src = w[:, :, k - 1 - ty, k - 1 - tx]
            elif form == 1:
                src = w[:, :, 3 - py - 2 * ty, 3 - px - 2 * tx]
            elif form == 4:
                src = w[:, :, 3 - py - 2 * (1 - ty), 3 - px - 2 * (1 - tx)].T
            else:
                ky, kx = py + 1 - 2 * ty, px + 1 - 2 * tx
                if ky < 0 or kx < 0:
                    continue
                src = w[:, :, ky, kx]
            blk = np.zeros((kp, cp), np.float32)
            blk[:cin, :cout] = src  # [ci, co]
            out[:, ty * k + tx] = blk.reshape(kp // 4, 4, cp)
    return out.reshape(-1)


@pytest.mark.parametrize("form,k,py,px", PACK_FORMS, ids=[f"form{f}-k{k}-phase{py}{px}" for f, k, py, px in PACK_FORMS])
def test_packed_weight_layout(form, k, py, px):
    g = torch.Generator().manual_seed(100 * form + 10 * k + 2 * py + px)
    jobs = []
    for cin in PACK_CINS:
        for cout in PACK_COUTS:
            w = torch.randn(_source_shape(form, cout, cin, k), generator=g)
            numel = LIB.mp_conv_packed_weight_bytes(cout, cin, k, k) // 4
            assert numel == (cin + 3) // 4 * 4 * k * k * ((cout + 15) // 16 * 16)
            jobs.append((cout, cin, w, w.to(DEV), Guarded((numel,)), Guarded((numel,)), _packed_layout(w.numpy(), form, cout, cin, k, py, px)))
    arr = (_PackJob * len(jobs))()
    first = np.zeros(len(jobs) + 1, dtype=np.uint32)
    for i, (cout, cin, _, wd, single, batch, _) in enumerate(jobs):
        _lib.check(LIB.mp_conv_pack_weight(_lib.ptr(wd), _lib.ptr(single.t), cout, cin, k, k, form, py, px, _lib.stream()), "mp_conv_pack_weight")
        arr[i] = _PackJob(wd.data_ptr(), batch.t.data_ptr(), cout, cin, k, k, form, py, px, 0)
        first[i + 1] = first[i] + ((cin + 3) // 4 * 4 * k * k * ((cout + 15) // 16 * 4) + 255) // 256  # one thread per four couts
    jobs_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    first_dev = torch.from_numpy(first.view(np.int32)).to(DEV)
    _lib.check(LIB.mp_conv_pack_weight_batch(_lib.ptr(jobs_dev), _lib.ptr(first_dev), len(jobs), int(first[-1]), _lib.stream()), "mp_conv_pack_weight_batch")
    torch.cuda.synchronize()
    for cout, cin, _, _, single, batch, want in jobs:
        what = f"form {form} k {k} phase ({py}, {px}) cin {cin} cout {cout}"
        for name, got in (("mp_conv_pack_weight", single), ("mp_conv_pack_weight_batch", batch)):
            got.assert_guards(f"{name} {what}")
            bits = got.t.cpu().numpy().view(np.int32)
            wrong = np.nonzero(bits != want.view(np.int32))[0]
            cp = (cout + 15) // 16 * 16
            assert wrong.size == 0, f"{name} {what}: {wrong.size} elements differ from the layout, first at flat index {int(wrong[0])} = " \
                                    f"(quad, tap, lane, cout) {np.unravel_index(int(wrong[0]), ((cin + 3) // 4, k * k, 4, cp))}"
