"""tests/glue_matrix.py checked without a GPU: every entry point keeps its small, ragged and over-the-cap cases (the floors below
fail when a later edit thins a list), the lists hold what tests/test_gpu_train_glue.py is written to reach, and the CPU references
agree with independent ones: the window-loop max-pool with torch's own pooling and its autograd, the fp32 restatement of the
exchange-unit sum with the float64 one, the optimizer rules with torch's fp32 evaluation of them."""
import pytest
import torch

from oracle.nets import maxpool3x3s2_same as oracle_pool
from tests import glue_matrix as gm


@pytest.mark.parametrize("name", list(gm.ENTRIES))
def test_every_entry_keeps_its_floors(name):
    e = gm.ENTRIES[name]
    assert e.cases and e.cap % 256 == 0 and e.source
    elements, units = [e.elements(c) for c in e.cases], [e.units(c) for c in e.cases]
    assert min(elements) < 256, "no case of fewer than 256 elements"
    assert any(v % 256 and (e.vec == 1 or v % e.vec) for v in elements), "no case that is ragged against the block and the vector width"
    assert any(e.cap < u <= e.cap * 1.02 for u in units), "no case that exceeds the cap by less than 2 % (second grid pass, ragged end)"
    # no case is larger than a second pass needs (the fp32 sum's vector case, quads forward, is four passes of its backward)
    assert max(units) <= e.cap * 1.02 * (4 if name == "mp_fuse_upsample_sum_bwd" else 1)


def test_caps_restate_the_launch_code():
    """the caps are products of the block limit in the quoted line and 256 threads; the quoted lines exist in the sources"""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mindpose_amd", "csrc")
    for name, e in gm.ENTRIES.items():
        fname, line = e.source
        with open(os.path.join(csrc, fname)) as f:
            assert line in f.read(), (name, fname, line)
    caps = {n: e.cap for n, e in gm.ENTRIES.items()}
    assert caps["mp_fuse_upsample_sum"] == caps["mp_fuse_upsample_sum_bwd"] == 2097152
    assert caps["mp_f16_fuse_upsample_sum"] == caps["mp_f16_fuse_upsample_sum_bwd"] == 2097152
    assert caps["mp_sum_tensors"] == caps["mp_maxpool3x3s2_same"] == 1048576
    assert caps["mp_maxpool3x3s2_same_bwd"] == caps["mp_gather_phase"] == caps["mp_f16_gather_phase"] == 4194304
    assert caps["mp_adamw_step"] == caps["mp_adamw_step_scaled"] == caps["mp_optimizer_step"] == 1048576
    assert caps["mp_grad_finite_check"] * 4 == gm.FINITE_CAP == 2097152


def test_lists_hold_what_the_gpu_tests_are_written_to_reach():
    over = lambda name: [c for c in gm.ENTRIES[name].cases if gm.ENTRIES[name].units(c) > gm.ENTRIES[name].cap]  # noqa: E731
    # fp32 exchange-unit sum: both paths, each over the cap; one, two and three terms; a repeated scale 1; both ReLU settings
    f32 = gm.FUSE32_CASES
    assert {c[3] % 4 == 0 for c in over("mp_fuse_upsample_sum")} == {True, False}
    assert {(c[3], s) for c in f32 for s in c[4]} >= {(w, s) for w in (6, 10, 14) for s in (1, 2)}
    for vec in (True, False):
        mine = [c for c in f32 if (c[3] % 4 == 0) == vec]
        assert {len(c[4]) for c in mine} == {1, 2, 3} and {c[5] for c in mine} == {0, 1}
    assert any(c[4].count(1) >= 2 for c in f32)
    for n, c, h, w, scales, _ in f32 + gm.FUSE16_CASES:
        assert all(h % s == 0 and w % s == 0 for s in scales)
    assert all(gm.is_pow2(s) for c in f32 for s in c[4])
    # fp16: both forms, each over the cap; on the fast form odd extents, h = 1, w = 1 and the 21 x 13 map; the generic scale sets
    f16 = gm.FUSE16_CASES
    assert {gm.f16_fuse_fast(c) for c in over("mp_f16_fuse_upsample_sum")} == {True, False}
    fast = [c for c in f16 if gm.f16_fuse_fast(c)]
    assert any(c[2] == 1 and c[3] > 1 for c in fast) and any(c[3] == 1 and c[2] > 1 for c in fast) and any(c[2] == c[3] == 1 for c in fast)
    assert any(c[2] % 2 and c[3] % 2 and c[2] > 1 and c[3] > 1 for c in fast) and (3, 17, 21, 13, (1,), 1) in fast
    assert {c[4] for c in f16 if not gm.f16_fuse_fast(c) and c[2:4] == (12, 18)} == {(3,), (2, 3), (2, 3, 6)}
    for cases in (f16, gm.fuse16_bwd_cases()):
        assert {c[1] for c in cases} >= {8, 17, 48} and {c[5] for c in cases} == {0, 1}
    assert any(c[1] % 8 for c in over("mp_f16_fuse_upsample_sum"))  # padding lanes in the second pass as well
    # fan-in sum, pools, stem, gathers, optimizers, overflow check
    assert {(h, k, u) for h, k, u in gm.SUM_CASES} >= {(h, k, u) for h in (0, 1) for k in (2, 3, 4) for u in (1, 255, 256, 257)}
    assert {c[0] for c in over("mp_sum_tensors")} == {0, 1}
    for cases in (gm.POOL_FWD_CASES, gm.POOL_BWD_CASES):
        assert {c[2:] for c in cases} >= set(gm.POOL_MAPS) and set(gm.POOL_MAPS) >= {(1, 1), (2, 3), (3, 2), (5, 5), (7, 12), (13, 9), (18, 14)}
    assert all(c[2] % 2 and c[3] % 2 for c in over("mp_maxpool3x3s2_same") + over("mp_maxpool3x3s2_same_bwd"))  # padded on both sides
    assert len(gm.STEM_CASES) == 2 * 4 * 2 * 3
    small = [c for c in gm.STEM_CASES if c[3] * gm.ceil_div(c[4], 2) * gm.ceil_div(c[5], 2) < 256]
    assert {c[:3] for c in small} == {(k, ci, co) for k in (3, 7) for ci in (1, 2, 3, 4) for co in (5, 64)} and len(small) < len(gm.STEM_CASES)
    for half in (0, 1):
        mine = [c for c in gm.GATHER_CASES if c[0] == half]
        assert {(c[2], c[3], c[4], c[5], c[6]) for c in mine} >= {(c, h, w, py, px) for c in (3, 8, 17) for h, w in ((1, 1), (5, 7), (12, 10))
                                                                 for py, px in gm.PHASES}
    assert gm.OPT_COUNTS == [1, 3, 255, 256, 257, gm.OPT_CAP + 5] and gm.FINITE_COUNTS == [1, 2, 3, 4, 5, 1027, gm.FINITE_CAP + 7]
    kinds = {k for k, _ in gm.OPT_VARIANTS.values()}
    assert kinds == {1, 2, 3, 4}
    sgd = [h for k, h in gm.OPT_VARIANTS.values() if k == 2]
    assert any(h[3] for h in sgd) and any(h[1] and not h[3] for h in sgd) and any(h[2] for h in sgd) and any(h[0] == 0 for h in sgd)
    assert any(h[1] for k, h in gm.OPT_VARIANTS.values() if k == 3)


POOL_CHECK_MAPS = gm.POOL_MAPS + [(4, 4), (6, 9)]


@pytest.mark.parametrize("h,w", POOL_CHECK_MAPS, ids=[f"{h}x{w}" for h, w in POOL_CHECK_MAPS])
@pytest.mark.parametrize("kind", gm.POOL_KINDS + ("constant",))
def test_pool_references_match_torch(h, w, kind):
    """odd and even maps, random values, values full of ties and an all-equal plane: the window loops give torch's max_pool2d on the
    -inf padded map and torch CPU's autograd of it, which sends a tied window's gradient to its first valid element"""
    g = torch.Generator().manual_seed(gm.seed_of(h, w, len(kind)))
    x = {"randn": lambda: gm.randn(g, 2, 3, h, w), "ties": lambda: torch.randint(0, 3, (2, 3, h, w), generator=g).float(),
         "constant": lambda: torch.full((2, 3, h, w), 1.5)}[kind]()
    oh, ow, pt, pl = gm.pool_geometry(h, w)
    assert (pt, pl) == (1 if h % 2 else 0, 1 if w % 2 else 0)
    dy = (gm.randn(g, 2, 3, oh, ow) * 1024).round() / 1024
    xt = x.clone().requires_grad_(True)
    y = oracle_pool(xt)
    y.backward(dy)
    assert torch.equal(gm.maxpool_ref(x), y.detach())
    dx = gm.maxpool_bwd_ref(x, dy)
    assert torch.equal(dx, xt.grad)
    assert torch.equal(dx.double().sum(dim=(2, 3)), dy.double().sum(dim=(2, 3)))  # every window's gradient lands exactly once


def _fuse_data(case, half):
    n, c, h, w, scales, relu = case
    g = torch.Generator().manual_seed(gm.seed_of(case))
    rnd = gm.randn_h if half else gm.randn
    return rnd(g, n, c, h, w), [rnd(g, n, c, h // s, w // s) for s in scales]


@pytest.mark.parametrize("half", [0, 1])
def test_fuse_sum_restatement_vs_float64(half):
    """fp32 sums in the kernels' term order against the float64 sum.  k additions in fp32 lose at most k * 2^-24 of the sum of the
    operands' magnitudes (each partial sum is no larger than it); the fp16 form adds its one rounding, half an fp16 ulp: 2^-11 of
    the value, 2^-25 below the smallest normal.  The bar of the fp16 form is half an ulp + 2^-23 of that magnitude sum."""
    entry = gm.ENTRIES["mp_f16_fuse_upsample_sum" if half else "mp_fuse_upsample_sum"]
    worst = 0.0
    for case in entry.cases:
        if entry.units(case) > entry.cap:
            continue  # same arithmetic, only larger
        base, terms = _fuse_data(case, half)
        scales, relu = case[4], case[5]
        ref = gm.fuse_sum_ref(base, terms, scales, relu)
        got = gm.fuse_sum_restated(base, terms, scales, relu, half=bool(half)).double()
        mag = gm.fuse_sum_ref(base.abs(), [t.abs() for t in terms], scales, 0)
        if half:
            bound = torch.maximum(gm.U16 * ref.abs(), torch.full_like(ref, 2.0 ** -25)) + 2.0 ** -23 * mag
        else:
            bound = len(terms) * gm.U24 * mag
        ratio = float(((got - ref).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, ratio)
        assert got.shape == ref.shape == base.shape
    print(f"half {half}: worst error / bound {worst:.3f}")


def test_fuse_sum_bwd_reference_vs_autograd():
    import torch.nn.functional as F
    for case in gm.FUSE32_CASES[:12]:
        n, c, h, w, scales, relu = case
        base, terms = _fuse_data(case, 0)
        g = torch.Generator().manual_seed(1 + gm.seed_of(case))
        dy = gm.randn(g, n, c, h, w)
        leaves = [base.double().requires_grad_(True)] + [t.double().requires_grad_(True) for t in terms]
        y = leaves[0]
        for t, s in zip(leaves[1:], scales):
            y = y + F.interpolate(t, scale_factor=s, mode="nearest")
        out = F.relu(y) if relu else y
        out.backward(dy.double())
        grads, mags = gm.fuse_sum_bwd_ref(dy, out.detach(), scales, relu)
        for got, leaf, mag in zip(grads, leaves, mags):
            assert torch.allclose(got, leaf.grad, rtol=1e-13, atol=1e-13) and bool((mag >= got.abs() - 1e-12).all())


def test_c8_layout_round_trips():
    x = gm.randn_h(torch.Generator().manual_seed(2), 2, 17, 3, 5)
    t = gm.to_c8(x)
    assert t.shape == (2, 3, 3, 5, 8) and t.dtype == torch.float16
    assert torch.equal(gm.from_c8(t, 17).float(), x)
    assert float(t[:, 2, :, :, 1:].abs().max()) == 0  # channels 17 ... 23: padding lanes
    assert t[1, 2, 1, 4, 0] == x[1, 16, 1, 4] and t[0, 1, 2, 0, 3] == x[0, 11, 2, 0]


def test_pattern_bits_are_finite_and_varied():
    for dtype, bits, mask in ((torch.float32, torch.int32, 0x7F800000), (torch.float16, torch.int16, 0x7C00)):
        p = gm.pattern_bits(100000, dtype)
        assert p.dtype == dtype and bool(torch.isfinite(p).all())
        assert bool(((p.view(bits).to(torch.int64) & mask) != mask).all())
        assert p.view(bits).unique().numel() > 10000 and bool((p < 0).any()) and bool((p > 0).any())


@pytest.mark.parametrize("name", ["adamw"] + list(gm.OPT_VARIANTS))
def test_optimizer_reference_vs_fp32_evaluation(name):
    """the float64 rules against the same rules evaluated by torch in fp32 on fp32 hyper-parameters (what the kernels do), at the bars
    the GPU tests use: 1e-6 of the reference's max abs for AdamW, rtol 2e-5 / atol 2e-6 for the others"""
    g = torch.Generator().manual_seed(gm.seed_of(len(name)))
    n = 4099
    p, gr = gm.randn(g, n), gm.randn(g, n)
    T = torch.tensor
    if name == "adamw":
        hp = gm.ADAMW_HYPER
        m, v = gm.randn(g, n) * 0.1, torch.rand(n, generator=g) * 0.01
        for scale in (1.0, 0.125):
            rp, rm, rv = gm.optimizer_ref(0, p, gr, m, v, hp["lr"], scale, hp["wd"], (hp["b1"], hp["b2"], hp["eps"]))
            gi = gr * T(scale)
            m32 = T(hp["b1"]) * m + (T(1.0) - T(hp["b1"])) * gi
            v32 = T(hp["b2"]) * v + (T(1.0) - T(hp["b2"])) * gi * gi
            p32 = p - T(hp["lr"]) * (m32 / (v32.sqrt() + T(hp["eps"])) + T(hp["wd"]) * p)
            for got, ref in ((p32, rp), (m32, rm), (v32, rv)):
                assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-6
        return
    kind, h = gm.OPT_VARIANTS[name]
    s1 = torch.rand(n, generator=g) + 0.1 if kind == 4 else gm.randn(g, n) * 0.1
    s2 = torch.rand(n, generator=g) * 0.01
    rp, r1, r2 = gm.optimizer_ref(kind, p, gr, None if name == "sgd-plain" else s1, s2 if kind == 1 else None, gm.OPT_LR, gm.OPT_GRAD_SCALE,
                                  gm.OPT_WD, h)
    lr, h = T(gm.OPT_LR), [T(v) for v in h]
    gi = gr * T(gm.OPT_GRAD_SCALE) + T(gm.OPT_WD) * p
    one = T(1.0)
    if kind == 1:
        a = h[0] * s1 + (one - h[0]) * gi
        b = h[1] * s2 + (one - h[1]) * gi * gi
        p32 = p - lr * (one - h[4]).sqrt() / (one - h[3]) * a / (b.sqrt() + h[2])
        assert torch.allclose(b.double(), r2, rtol=2e-5, atol=2e-6)
    elif kind == 2:
        a, d = s1, gi
        if float(h[0]) != 0:
            a = gi if float(h[3]) != 0 else h[0] * s1 + (one - h[1]) * gi
            d = gi + h[0] * a if float(h[2]) != 0 else a
        p32 = p - lr * d
    elif kind == 3:
        a = h[0] * s1 + gi
        p32 = p - lr * (gi + h[0] * a if float(h[1]) != 0 else a)
    else:
        a = s1 + gi * gi
        p32 = p - lr * gi / a.sqrt()
    assert torch.allclose(p32.double(), rp, rtol=2e-5, atol=2e-6)
    if r1 is not None:
        assert torch.allclose(a.double(), r1, rtol=2e-5, atol=2e-6)
    else:
        assert name == "sgd-plain"


def test_stem_and_gather_references():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4)
    for k in (3, 7):
        x, dz = gm.randn(g, 2, 3, 9, 8), gm.randn(g, 2, 5, 5, 4)
        ref, mag = gm.stem_wgrad_ref(x, dz, k)
        # the definition, tap by tap: dW[co][ci][ky][kx] = sum dz[n, co, y, x] * x[n, ci, 2y + ky - p, 2x + kx - p]
        xp = F.pad(x.double(), (k // 2,) * 4)
        for ky, kx in ((0, 0), (k // 2, k - 1), (k - 1, 1)):
            tap = xp[:, :, ky:ky + 2 * 5 - 1:2, kx:kx + 2 * 4 - 1:2]
            want = torch.einsum("noyx,niyx->oi", dz.double(), tap)
            assert torch.allclose(ref[:, :, ky, kx], want, rtol=1e-12, atol=1e-12)
        assert ref.shape == (5, 3, k, k) and bool((mag >= ref.abs()).all())
    x = torch.arange(2 * 3 * 4 * 6).view(2, 3, 4, 6).float()
    for py, px in gm.PHASES:
        out = gm.gather_phase_ref(x, py, px)
        assert out.shape == (2, 3, 2, 3) and out[1, 2, 1, 2] == x[1, 2, 2 + py, 4 + px] and out.is_contiguous()
