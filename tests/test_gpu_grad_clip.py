"""Gradient clipping by global norm decided on the device (csrc/step_end.hip, utils/adamw.py ``clip_norm``,
utils/step_tail.py): the fused overflow check + sum of squares against numpy in fp64 and against ``mp_grad_finite_check``, the tail
with clipping against ``mp_train_tail_advance`` and a Python restatement of the definition in double, the five optimizers resident
against host-driven, and the graphed step end to end.

Bounds.  u = 2^-53.  The products of two fp32 values are exact in fp64, so the sum of squares S of n values is a sum of n
non-negative terms whose every addition rounds once: in ANY order |S - S_true| <= (n - 1) u S_true (1 + O(n u)), and numpy's own
pairwise sum is inside the same bound - the tests ask |S - S_ref| <= (n + 2) u S_ref.  norm = sqrt(S) * base adds the rounding of
the square root and of the product and halves the relative error of S: |norm - ref| <= ((n + 2) / 2 + 3) u ref, with ref = sqrt of
torch's fp64 sum times the same base (one more u for torch's own square root and product is inside the 3).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.utils import DynamicLossScaleManager, GraphedTrainStep, create_optimizer  # noqa: E402
from mindpose_amd.utils.adamw import CLIP_RESOLVED_DTYPE, CLIP_STATE_DTYPE, clip_coefficient  # noqa: E402
from mindpose_amd.utils.step_tail import ARGS_DTYPE, STATE_DTYPE, ResidentStepTail, adam_aux_table  # noqa: E402

from tests import glue_matrix as gm  # noqa: E402

DEV = torch.device("cuda:0")
U53 = 2.0 ** -53
GUARD = 64  # floats (the arena stays 16-byte aligned) / doubles
CAP_BLOCKS = 256 * 8
SPAN = 1024  # quads a workgroup reads per trip
OVER_CAP = 4 * (CAP_BLOCKS * SPAN + 16) + 3  # 2,097,168 quads + 3 values: the second grid pass, 16 quads and a scalar tail long
# scalar tail only (1, 3), one quad, ragged, a part of a trip, several workgroups (one full trip, one partial, + 3), over the grid cap
COUNTS = [1, 3, 4, 255, 1027, 5003, OVER_CAP]
SPECIALS = [3.4028234663852886e38, -3.4028234663852886e38, 1e-45, -1e-40, -0.0, 0.0, 1.0, -2.5, 1.17549435e-38]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _dev_bytes(record: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(record.view(np.uint8).copy()).to(DEV)


def _read(t: torch.Tensor, dtype: np.dtype):
    return t.cpu().numpy().view(dtype)[0]


def sum_partials(partials) -> float:
    """S as the single-wave launches state it: lane l adds partials l, l + 64, ... in index order; then six rounds in which lane l
    adds the value of lane l + off (its own when there is none), off = 32 ... 1; lane 0 holds S."""
    lanes = [0.0] * 64
    for i, p in enumerate(partials):
        lanes[i % 64] += float(p)
    off = 32
    while off >= 1:
        lanes = [lanes[l] + (lanes[l + off] if l + off < 64 else lanes[l]) for l in range(64)]
        off //= 2
    return lanes[0]


# ---- 1. the fused pass ---------------------------------------------------------------------------------------------------------------
_ARENAS = {}


def _arena(count, kind):
    """(host values, device tensor between NaN guard bands), made once and never changed (planting tests restore what they plant)"""
    if (count, kind) not in _ARENAS:
        rs = np.random.RandomState(count % 9973 + (17 if kind == "huge" else 0))
        if kind == "bits":  # every finite bit pattern is equally likely: every magnitude, both signs, denormals
            bits = rs.randint(0, 2 ** 32, size=count, dtype=np.uint64).astype(np.uint32)
            bits[(bits & 0x7f800000) == 0x7f800000] &= np.uint32(0xbfffffff)  # an all-ones exponent loses a bit: finite
            x = bits.view(np.float32).copy()
            k = min(count, len(SPECIALS))
            x[:k] = np.array(SPECIALS, dtype=np.float32)[:k]
        else:  # +-1e30 x [0.5, 1): every square is near 1e60, far outside fp32
            x = ((rs.rand(count) * 0.5 + 0.5) * 1e30 * np.where(rs.rand(count) < 0.5, -1.0, 1.0)).astype(np.float32)
        t = torch.full((count + 2 * GUARD,), float("nan"), dtype=torch.float32)
        t[GUARD:GUARD + count] = torch.from_numpy(x)
        _ARENAS[(count, kind)] = (x, t.to(DEV))
    return _ARENAS[(count, kind)]


def _fused(lib, dev, count, flag_value=0):
    """one launch: (flag, partials as numpy) with the partials between NaN guard bands, every entry pre-filled with NaN"""
    n_part = lib.mp_grad_norm_partials(count)
    flag = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    flag[1] = flag_value
    parts = torch.full((n_part + 2 * GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.mp_grad_finite_norm(dev[GUARD:].data_ptr(), count, flag[1:].data_ptr(), parts[GUARD:].data_ptr(), _lib.stream()),
               "mp_grad_finite_norm")
    torch.cuda.synchronize()
    f, p = flag.cpu(), parts.cpu()
    assert int(f[0]) == 0x5A5A5A5A and int(f[2]) == 0x5A5A5A5A, "the words next to the flag were written"
    assert torch.isnan(p[:GUARD]).all() and torch.isnan(p[GUARD + n_part:]).all(), "the partials' guard bands were written"
    return int(f[1]), p[GUARD:GUARD + n_part].numpy()


def _plain_flag(lib, dev, count):
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib.mp_grad_finite_check(dev[GUARD:].data_ptr(), count, flag.data_ptr(), _lib.stream()), "mp_grad_finite_check")
    return int(flag.item())


@pytest.mark.parametrize("kind", ["bits", "huge"])
@pytest.mark.parametrize("count", COUNTS)
def test_fused_pass_sum_of_squares_and_flag(count, kind):
    lib = _lib.load()
    x, dev = _arena(count, kind)
    assert dev[GUARD:].data_ptr() % 16 == 0
    n_part = lib.mp_grad_norm_partials(count)
    assert n_part == min(max(gm.ceil_div(count // 4, SPAN), 1), CAP_BLOCKS)
    flag, parts = _fused(lib, dev, count)
    assert flag == 0 == _plain_flag(lib, dev, count), "clean data raised a flag"
    assert not np.isnan(parts).any() and (parts >= 0).all(), "a partial was not written"
    s_ref = float(np.sum(x.astype(np.float64) ** 2))
    s = sum_partials(parts)
    assert math.isfinite(s_ref) and s_ref > 0
    if kind == "huge":
        assert s_ref > 3.5e38 and float(np.float32(1e30)) ** 2 > 3.5e38  # an fp32 accumulator would hold inf
    err, bound = abs(s - s_ref), (count + 2) * U53 * s_ref
    print(f"count {count} {kind}: |S - S_ref| / S_ref = {err / s_ref:.3e}, bound {(count + 2) * U53:.3e}, {n_part} partials")
    assert err <= bound, (count, kind, s, s_ref)
    flag2, parts2 = _fused(lib, dev, count)
    assert flag2 == 0 and parts.tobytes() == parts2.tobytes(), "two launches gave different partials"
    assert _fused(lib, dev, count, flag_value=1)[0] == 1, "a flag that was set did not stay set"
    assert torch.isnan(dev[:GUARD]).all() and torch.isnan(dev[GUARD + count:]).all(), "the arena's guard bands changed"
    assert np.array_equal(dev[GUARD:GUARD + count].cpu().numpy().view(np.uint32), x.view(np.uint32)), "the arena changed"


@pytest.mark.parametrize("count", COUNTS)
def test_fused_pass_flag_equals_the_plain_check_on_planted_values(count):
    lib = _lib.load()
    _, dev = _arena(count, "bits")
    n4 = count // 4
    spots = {0, count - 1}
    spots.update(range(n4 * 4, count))  # the scalar tail
    if n4:
        spots.update({4 * (n4 // 2) + 1, 4 * (n4 - 1) + 3})
    if count > 4 * CAP_BLOCKS * SPAN:
        spots.update({4 * CAP_BLOCKS * SPAN - 1, 4 * CAP_BLOCKS * SPAN, 4 * CAP_BLOCKS * SPAN + 5})  # around the second grid pass
    bad = [float("inf"), float("-inf"), float("nan")]
    for j, at in enumerate(sorted(spots)):
        keep = dev[GUARD + at].clone()
        dev[GUARD + at] = bad[j % 3]
        got, want = _fused(lib, dev, count)[0], _plain_flag(lib, dev, count)
        dev[GUARD + at] = keep
        assert got == want == 1, f"count {count}: {bad[j % 3]} at index {at}: fused flag {got}, plain check {want}"
    assert _fused(lib, dev, count)[0] == 0  # restored


def test_fused_pass_refuses_before_launching():
    lib = _lib.load()
    _, dev = _arena(1027, "bits")
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    parts = torch.zeros(8, dtype=torch.float64, device=DEV)
    args = (flag.data_ptr(), parts.data_ptr(), _lib.stream())
    assert lib.mp_grad_finite_norm(None, 4, *args) == -1 and lib.mp_grad_finite_norm(dev.data_ptr(), 4, None, parts.data_ptr(), None) == -1
    assert lib.mp_grad_finite_norm(dev.data_ptr(), 4, flag.data_ptr(), None, None) == -1
    assert lib.mp_grad_finite_norm(dev[GUARD:].data_ptr() + 4, 8, *args) == _lib.MP_ERR_UNSUPPORTED
    assert lib.mp_grad_finite_norm(dev[GUARD:].data_ptr(), 8, flag.data_ptr(), parts.data_ptr() + 4, _lib.stream()) == _lib.MP_ERR_UNSUPPORTED
    assert lib.mp_grad_finite_norm(dev[GUARD:].data_ptr(), 0, *args) == 0 and lib.mp_grad_norm_partials(0) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and float(parts.abs().sum()) == 0.0


# ---- 2. the tail ---------------------------------------------------------------------------------------------------------------------
ITERS, TABLE = 200, 50


def _overflow_pattern() -> np.ndarray:
    """as tests/test_gpu_step_tail.py: seeded, overflow at 0 .. 39 (every initial scale reaches the floor) and five in a row at 60 .. 64"""
    over = np.random.RandomState(7).rand(ITERS) < 0.1
    over[0:40] = True
    over[60:65] = True
    return over


def _tail_blocks(init, applied=0):
    st = np.zeros(1, STATE_DTYPE)
    st["loss_scale"], st["last_overflow_iter"], st["cur_iter"], st["applied_steps"] = init, -1, applied, applied
    return _dev_bytes(st), torch.zeros(ARGS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("static", [1.0, 128.0])
@pytest.mark.parametrize("mean_scale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("init,factor,window", [(2.0 ** 24, 2.0, 2000), (1000.0, 1.5, 2)])
def test_tail_measure_only_is_the_plain_tail(init, factor, window, mean_scale, static):
    lib = _lib.load()
    lr_dev = torch.from_numpy((np.random.RandomState(1).rand(TABLE).astype(np.float32) + np.float32(0.5)) * np.float32(1e-3)).to(DEV)
    aux_dev = torch.from_numpy(adam_aux_table(0.9, 0.999, TABLE)).to(DEV)
    (st_a, args_a), (st_b, args_b) = _tail_blocks(init), _tail_blocks(init)
    scale_a, scale_b = (torch.zeros((), dtype=torch.float32, device=DEV) for _ in range(2))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    parts = torch.from_numpy(np.random.RandomState(2).rand(37) * 1e9).to(DEV)
    cs = torch.zeros(CLIP_STATE_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    over = _overflow_pattern()
    seen = []
    for it in range(ITERS):
        flag.fill_(int(over[it]))
        common = (factor, window, mean_scale, static, lr_dev.data_ptr(), TABLE, aux_dev.data_ptr(), TABLE)
        _lib.check(lib.mp_train_tail_advance(flag.data_ptr(), st_a.data_ptr(), *common, args_a.data_ptr(), scale_a.data_ptr(), _lib.stream()),
                   "mp_train_tail_advance")
        _lib.check(lib.mp_train_tail_advance_clip(flag.data_ptr(), st_b.data_ptr(), *common, args_b.data_ptr(), scale_b.data_ptr(),
                                                  parts.data_ptr(), parts.numel(), math.inf, cs.data_ptr(), _lib.stream()),
                   "mp_train_tail_advance_clip")
        seen.append(torch.stack([torch.cat([st_a, args_a, scale_a.view(1).view(torch.uint8)]),
                                 torch.cat([st_b, args_b, scale_b.view(1).view(torch.uint8)])]))
    seen = torch.stack(seen).cpu()  # one download
    for it in range(ITERS):
        assert torch.equal(seen[it, 0], seen[it, 1]), f"iteration {it}: state / step arguments / loss scale differ from the plain tail"
    c = _read(cs, CLIP_STATE_DTYPE)
    assert int(c["measured_steps"]) == int((~over).sum()) and int(c["clipped_steps"]) == 0
    assert float(c["norm_max"]) >= float(c["last_norm"]) > 0.0


@pytest.mark.parametrize("n_partials", [1, 64, 100, CAP_BLOCKS])
def test_tail_with_a_finite_clip_norm_is_the_definition_in_double(n_partials):
    lib = _lib.load()
    mean_scale, static, factor, window, init = 1.0 / 3.0, 4.0, 2.0, 3, 2.0 ** 10
    lr_dev = torch.tensor([3e-4], dtype=torch.float32, device=DEV)
    st, args = _tail_blocks(init)
    cs = torch.zeros(CLIP_STATE_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    rs = np.random.RandomState(n_partials)
    mgr = DynamicLossScaleManager(init, factor, window)
    want = dict(last_norm=0.0, norm_sum=0.0, norm_max=0.0, measured_steps=0, clipped_steps=0)
    # per step: (magnitude of the partials, clip_norm relative to the step's norm or absolute, overflow)
    plan = [(1e12, ("rel", 0.25), 0), (1e6, ("rel", 1.0), 0), (1e12, ("rel", 0.5), 1), (1e3, ("abs", 1e30), 0), (1e12, ("rel", 1.0 - 2.0 ** -50), 0),
            (1e9, ("abs", math.inf), 0), (1e12, ("rel", 1e-3), 0)]
    saw_equal = False
    for it, (mag, (how, value), overflow) in enumerate(plan):
        host_parts = rs.rand(n_partials) * mag
        parts = torch.from_numpy(host_parts).to(DEV)
        base = mean_scale / mgr.loss_scale / static
        norm = math.sqrt(sum_partials(host_parts)) * base
        clip_norm = norm * value if how == "rel" else value
        flag.fill_(overflow)
        _lib.check(lib.mp_train_tail_advance_clip(flag.data_ptr(), st.data_ptr(), factor, window, mean_scale, static, lr_dev.data_ptr(), 1,
                                                  None, 0, args.data_ptr(), None, parts.data_ptr(), n_partials, clip_norm, cs.data_ptr(),
                                                  _lib.stream()), "mp_train_tail_advance_clip")
        a, s, c = _read(args, ARGS_DTYPE), _read(st, STATE_DTYPE), _read(cs, CLIP_STATE_DTYPE)
        coef = clip_coefficient(norm, clip_norm)
        what = f"step {it} ({n_partials} partials)"
        assert int(a["skip"]) == overflow, what
        assert a["grad_scale"] == np.float32(ctypes.c_float(base * coef).value), (what, a["grad_scale"], base * coef)
        if how == "rel" and value == 1.0:  # norm == clip_norm: not clipped, the scale is the unclipped one bit for bit
            assert coef == 1.0 and a["grad_scale"] == np.float32(ctypes.c_float(base).value), what
            saw_equal = True
        if not overflow:
            want["last_norm"], want["norm_sum"], want["norm_max"] = norm, want["norm_sum"] + norm, max(want["norm_max"], norm)
            want["measured_steps"] += 1
            want["clipped_steps"] += int(norm > clip_norm)
        before = mgr.loss_scale
        mgr.update_loss_scale(bool(overflow))
        assert not overflow or mgr.loss_scale == before / factor, what  # halved as before
        assert float(s["loss_scale"]) == mgr.loss_scale and int(s["skipped_steps"]) == mgr.skipped_steps, what
        for k, v in want.items():  # untouched on the overflow step, the definition bit for bit otherwise
            assert c[k] == v, (what, k, c[k], v)
    assert saw_equal and mgr.skipped_steps == 1
    assert want["clipped_steps"] == 3 and want["measured_steps"] == 6


def test_tail_without_a_flag_and_a_non_finite_norm():
    """fp32 training: no flag, so never skipped; an inf or NaN sum of squares leaves coef = 1 and is recorded as it is"""
    lib = _lib.load()
    lr_dev = torch.tensor([3e-4], dtype=torch.float32, device=DEV)
    st, args = _tail_blocks(1.0, applied=4)
    cs = torch.zeros(CLIP_STATE_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    for it, (value, clipped) in enumerate(((4.0, 1), (math.inf, 1), (math.nan, 1))):
        parts = torch.tensor([1.0, value, 3.0], dtype=torch.float64, device=DEV)
        _lib.check(lib.mp_train_tail_advance_clip(None, st.data_ptr(), 2.0, 1, 0.5, 1.0, lr_dev.data_ptr(), 1, None, 0, args.data_ptr(), None,
                                                  parts.data_ptr(), 3, 1.0, cs.data_ptr(), _lib.stream()), "mp_train_tail_advance_clip")
        a, c = _read(args, ARGS_DTYPE), _read(cs, CLIP_STATE_DTYPE)
        norm = math.sqrt(1.0 + value + 3.0) * 0.5 if math.isfinite(value) else value
        assert int(a["skip"]) == 0 and a["grad_scale"] == np.float32(0.5 * clip_coefficient(norm, 1.0))
        assert int(c["measured_steps"]) == it + 1 and int(c["clipped_steps"]) == clipped
        assert c["last_norm"] == norm or (math.isnan(norm) and math.isnan(c["last_norm"]))
    assert float(_read(cs, CLIP_STATE_DTYPE)["norm_max"]) == math.inf  # the NaN after it did not replace it


# ---- 3. the optimizers -----------------------------------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    """Three parameters; ``names`` decide the groups (beta / gamma / bias are not decayed)."""

    def __init__(self, names):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        for name, shape in zip(names, ((33, 7), (129,), (5,))):
            setattr(self, name, torch.nn.Parameter(torch.randn(*shape, generator=g)))


OPTIMIZERS = {"adamw": dict(name="adamw"), "adam": dict(name="adam", loss_scale=4.0), "sgd": dict(name="sgd", momentum=0.9, loss_scale=4.0),
              "momentum": dict(name="momentum", momentum=0.9, loss_scale=2.0), "adagrad": dict(name="adagrad", loss_scale=4.0)}
GROUPS = {"both": ("weight", "gamma", "bias"), "no_decay_empty": ("w1", "w2", "w3"), "decay_empty": ("gamma", "beta", "bias")}
MAGNITUDES = [1000.0, 50.0, 1000.0, 2000.0, 20.0, 500.0]  # x randn: the true norms straddle CLIP
CLIP, LR, OVERFLOW_AT = 5.0, 1e-3, 2


def _direct_update(lib, opt, grad_scale: np.float32, hyper):
    """the existing host-argument entries on ``opt``'s arenas, per decay group as ``_ArenaOptimizer.step`` launches them"""
    n = opt.flat.numel()
    for start, count, wd in ((0, opt.n_decay, opt.weight_decay), (opt.n_decay, n - opt.n_decay, 0.0)):
        if not count:
            continue
        p, g = opt.flat[start:].data_ptr(), opt._grad_flat[start:].data_ptr()
        st = [s[start:].data_ptr() for s in opt.states] + [None, None]
        if getattr(opt, "kind", 0) == 0:
            rc = lib.mp_adamw_step_scaled(p, g, st[0], st[1], count, float(opt.lr), float(opt.beta1), float(opt.beta2), float(opt.eps),
                                          float(wd), float(grad_scale), None, _lib.stream())
        else:
            h = (ctypes.c_float * 5)(*[float(v) for v in hyper])
            rc = lib.mp_optimizer_step(opt.kind, p, g, st[0], st[1], count, float(opt.lr), float(grad_scale), float(wd), ctypes.byref(h),
                                       _lib.stream())
        _lib.check(rc, "direct update")


@pytest.mark.parametrize("names", list(GROUPS))
@pytest.mark.parametrize("which", list(OPTIMIZERS))
def test_optimizers_resident_equals_host_driven_with_clipping(which, names):
    lib = _lib.load()

    def build(clip_norm=CLIP):
        net = _Toy(GROUPS[names]).to(DEV)
        opt = create_optimizer(net, learning_rate=LR, weight_decay=0.05, overlap=False, clip_norm=clip_norm, **OPTIMIZERS[which])
        return opt, DynamicLossScaleManager(2.0 ** 10, 2.0, 3)

    (host, host_mgr), (res, res_mgr), (ref, _) = build(), build(), build(None)
    n = host.flat.numel()
    static = float(getattr(host, "loss_scale", 1.0))
    tail = ResidentStepTail(res, res_mgr, len(MAGNITUDES))
    g = torch.Generator().manual_seed(9)
    for it, mag in enumerate(MAGNITUDES):
        grad = torch.randn(n, generator=g) * mag
        if it == OVERFLOW_AT:
            grad[(it * 37) % n] = float("inf")
        for opt in (host, res, ref):
            opt._grad_flat.zero_()
            opt._grad_flat[:n].copy_(grad.to(DEV))
        base = host.grads.mean_scale / host_mgr.loss_scale / static
        hyper = host._hyper() if getattr(host, "kind", 0) else None
        for a, b in zip([ref.flat] + ref.states, [host.flat] + host.states):
            a.copy_(b)  # the reference starts every step from the host-driven state
        updated = host.step(host_mgr)
        tail.launch()
        assert updated == (it != OVERFLOW_AT)
        if not updated:
            continue
        # the coefficient is only a factor of the scalar: the existing entry with the restated gradient scale gives the same bits
        norm = math.sqrt(sum_partials(host._clip_partials.cpu().numpy())) * base
        coef = clip_coefficient(norm, CLIP)
        assert host.clip_coef == coef
        _direct_update(lib, ref, np.float32(ctypes.c_float(base * coef).value), hyper)
        assert _same_bits(ref.flat, host.flat), f"step {it}: parameters differ from the entry called with the restated grad_scale"
        for i, (a, b) in enumerate(zip(ref.states, host.states)):
            assert _same_bits(a, b), f"step {it}: state {i}"
        # the recorded norm against torch in fp64
        want = math.sqrt(float((host._grad_flat.double() ** 2).sum())) * base
        got = host.grad_clip_stats()["last_norm"]
        assert got == norm and abs(got - want) <= ((host._grad_flat.numel() + 2) / 2 + 3) * U53 * want, (it, got, want)
    tail.sync()
    assert _same_bits(host.flat, res.flat), "parameters"
    for i, (a, b) in enumerate(zip(host.states, res.states)):
        assert _same_bits(a, b), f"state {i}"
    for field in ("loss_scale", "cur_iter", "last_overflow_iter", "skipped_steps"):
        assert getattr(res_mgr, field) == getattr(host_mgr, field), field
    assert res.global_step == host.global_step == len(MAGNITUDES) - 1
    stats = host.grad_clip_stats()
    assert res.grad_clip_stats() == stats, (res.grad_clip_stats(), stats)
    assert _read(res._clip_state, CLIP_STATE_DTYPE).tobytes() == _read(host._clip_state, CLIP_STATE_DTYPE).tobytes()
    assert stats["measured_steps"] == len(MAGNITUDES) - 1 and 1 <= stats["clipped_steps"] < stats["measured_steps"], stats
    assert stats["max_norm"] > CLIP and stats["last_norm"] > 0 and stats["max_norm"] >= stats["mean_norm"] > 0
    host.reset_grad_clip_stats()
    assert host.grad_clip_stats() == dict(last_norm=0.0, mean_norm=0.0, max_norm=0.0, measured_steps=0, clipped_steps=0)
    for opt in (host, res, ref):
        opt.close()


def test_optimizer_without_a_manager_measures_and_clips_in_fp32():
    """no loss-scale manager: the fused pass runs for the norm alone, its flag is ignored - an inf gradient is not skipped"""
    def build():
        return create_optimizer(_Toy(GROUPS["both"]).to(DEV), name="momentum", momentum=0.9, learning_rate=LR, overlap=False, clip_norm=CLIP)

    host, res = build(), build()
    n = host.flat.numel()
    tail = ResidentStepTail(res, None, 3)
    g = torch.Generator().manual_seed(11)
    for it, mag in enumerate((100.0, 1e-3, 1.0)):
        grad = torch.randn(n, generator=g) * mag
        for opt in (host, res):
            opt._grad_flat.zero_()
            opt._grad_flat[:n].copy_(grad.to(DEV))
        assert host.step() is True
        tail.launch()
    tail.sync()
    assert _same_bits(host.flat, res.flat) and _same_bits(host.states[0], res.states[0])
    stats = host.grad_clip_stats()
    assert res.grad_clip_stats() == stats and stats["measured_steps"] == 3 and stats["clipped_steps"] == 2, stats
    for opt in (host, res):
        opt.close()


def test_clip_resolve_block_layout():
    lib = _lib.load()
    parts = torch.tensor([9.0, 16.0], dtype=torch.float64, device=DEV)
    cs = torch.zeros(CLIP_STATE_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    out = torch.zeros(CLIP_RESOLVED_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    for f, want in ((None, (0, 2.5, 0.8)), (flag, (1, 2.5, 1.0))):
        _lib.check(lib.mp_grad_clip_resolve(f.data_ptr() if f is not None else None, parts.data_ptr(), 2, 1.0, 2.0, 1.0, 2.0, cs.data_ptr(),
                                            out.data_ptr(), _lib.stream()), "mp_grad_clip_resolve")
        r = _read(out, CLIP_RESOLVED_DTYPE)
        assert (int(r["flag"]), float(r["norm"]), float(r["coef"])) == want
    c = _read(cs, CLIP_STATE_DTYPE)
    assert (float(c["last_norm"]), int(c["measured_steps"]), int(c["clipped_steps"])) == (2.5, 1, 1)  # the flagged call recorded nothing
    assert lib.mp_grad_clip_resolve(None, parts.data_ptr(), 2, 1.0, 2.0, 1.0, 0.0, cs.data_ptr(), out.data_ptr(), _lib.stream()) == -2
    assert lib.mp_grad_clip_resolve(None, parts.data_ptr(), CAP_BLOCKS + 1, 1.0, 2.0, 1.0, 1.0, cs.data_ptr(), out.data_ptr(), None) == -2


# ---- 4. the graphed step end to end ------------------------------------------------------------------------------------------------------
STEPS = 4


def _batches():
    g = torch.Generator().manual_seed(3)
    tgt = mp.TopDownGenerateTarget(config=dict(image_size=[192, 256], heatmap_size=[48, 64]), sigma=2.0)
    out = []
    for _ in range(STEPS):
        x = torch.randn(4, 3, 256, 192, generator=g)
        kp = torch.rand(4, 17, 3, generator=g) * torch.tensor([192.0, 256.0, 2.0])
        out.append((x.to(DEV), *tgt(kp.to(DEV))))
    return out


def _train(batches, clip_norm, graphed=True):
    """HRNet-W32 4 x 3 x 256 x 192 under amp O2, ``STEPS`` steps; graphed: the resident graphed step, else the eager host-driven one.
    Per step the recorded norm and torch's fp64 norm of the arena (clipping on)."""
    torch.manual_seed(0)
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(DEV).train()
    mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.create_network_with_loss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True)
    opt = create_optimizer(net, name="adamw", learning_rate=1e-3, weight_decay=0.05, overlap=False, clip_norm=clip_norm)
    mgr = DynamicLossScaleManager(2.0 ** 10, 2.0, 2000)  # (the scale the data-parallel tests train this network at)
    step = GraphedTrainStep(nwl, opt, batches[0], loss_scale_manager=mgr, resident=True, total_steps=STEPS) if graphed else None
    norms = []
    for b in batches:
        if graphed:
            loss_scale = float(step.tail.read_state()["loss_scale"])
            step(*b)
        else:
            loss_scale = mgr.loss_scale
            opt.zero_grad()
            mgr.scale(nwl(*b)).backward()
            opt.step(loss_scale_manager=mgr)
        if clip_norm is not None:
            want = math.sqrt(float((opt._grad_flat.double() ** 2).sum())) * (opt.grads.mean_scale / loss_scale)
            norms.append((opt.grad_clip_stats()["last_norm"], want))
    if graphed:
        step.sync()
    torch.cuda.synchronize()
    out = dict(flat=opt.flat.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), norms=norms, n=opt._grad_flat.numel(),
               mgr=(mgr.loss_scale, mgr.cur_iter, mgr.last_overflow_iter, mgr.skipped_steps), global_step=opt.global_step,
               stats=opt.grad_clip_stats() if clip_norm is not None else None)
    opt.close()
    return out


@pytest.fixture(scope="module")
def graphed_runs():
    mpatch = pytest.MonkeyPatch()
    mpatch.setenv("MINDPOSE_AUTOTUNE", "0")
    try:
        batches = _batches()
        plain, measured = _train(batches, None), _train(batches, math.inf)
        clip_norm = 1e-3 * measured["norms"][0][0]
        return dict(plain=plain, measured=measured, clip_norm=clip_norm, clipped=_train(batches, clip_norm),
                    eager=_train(batches, clip_norm, graphed=False))
    finally:
        mpatch.undo()


def _norms_match_the_arena(run):
    for it, (got, want) in enumerate(run["norms"]):
        assert math.isfinite(got) and abs(got - want) <= ((run["n"] + 2) / 2 + 3) * U53 * want, (it, got, want)


def test_graphed_step_measure_only_changes_nothing(graphed_runs):
    plain, measured = graphed_runs["plain"], graphed_runs["measured"]
    for key in ("flat", "m", "v"):
        assert _same_bits(plain[key], measured[key]), key
    assert plain["mgr"] == measured["mgr"] and plain["global_step"] == measured["global_step"] == STEPS - plain["mgr"][3] > 0
    stats = measured["stats"]
    assert stats["measured_steps"] == measured["global_step"] and stats["clipped_steps"] == 0 and stats["max_norm"] > 0
    _norms_match_the_arena(measured)


def test_graphed_step_clips_every_step_and_equals_the_eager_step(graphed_runs):
    plain, clipped, eager = graphed_runs["plain"], graphed_runs["clipped"], graphed_runs["eager"]
    stats = clipped["stats"]
    assert clipped["mgr"][3] == 0 and stats["measured_steps"] == stats["clipped_steps"] == clipped["global_step"] == STEPS, (stats, clipped["mgr"])
    assert stats["last_norm"] > graphed_runs["clip_norm"]
    _norms_match_the_arena(clipped)
    assert not _same_bits(plain["flat"], clipped["flat"]), "clipping changed nothing"
    for key in ("flat", "m", "v"):
        assert _same_bits(clipped[key], eager[key]), f"{key}: graphed differs from eager"
    assert clipped["mgr"] == eager["mgr"] and eager["stats"] == stats
    assert [a for a, _ in clipped["norms"]] == [a for a, _ in eager["norms"]]


# ---- the recipe runner logs the epoch's norm line ------------------------------------------------------------------------------------------
def test_runner_logs_the_gradient_norm_per_epoch(tmp_path, monkeypatch, caplog):
    """``--cfg-options clip_grad=True clip_value=...`` on the recipe, in fp32 (no loss-scale manager: the fused pass runs for the norm
    alone): every epoch logs one norm line, every step of it clipped at a tiny clip_value, and the statistics start anew per epoch."""
    import logging
    import re

    from mindpose_amd.cli.config import parse_args
    from mindpose_amd.cli.train import train
    from tests.test_gpu_trainer import _argv, _coco_folder
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")
    data = dict(train_root=str(tmp_path / "train"), val_root=str(tmp_path / "val"))
    data["train_label"] = _coco_folder(data["train_root"], 9, 5, "train.json")
    data["val_label"] = _coco_folder(data["val_root"], 2, 6, "val.json")
    argv = _argv(data, str(tmp_path / "out")) + ["amp_level=O0", "val_while_train=False", "clip_grad=True", "clip_value=1e-6"]
    with caplog.at_level(logging.INFO):
        train(parse_args(argv))
    lines = re.findall(r"epoch = (\d+), gradient norm: mean = (\S+), max = (\S+), clipped (\d+) of (\d+) steps \(clip_norm = 1e-06\)", caplog.text)
    assert [int(e) for e, *_ in lines] == [1, 2], caplog.text[-2000:]
    for _, mean, top, clipped, measured in lines:
        assert int(clipped) == int(measured) == 2  # 9 images in batches of 4: two steps per epoch, counted per epoch
        assert 1e-6 < float(mean.rstrip(",")) <= float(top.rstrip(",")) < math.inf
    assert len(re.findall(r"grad_norm = ", caplog.text)) == 2  # the callback's epoch line carries it too


# ---- 5. two ranks ------------------------------------------------------------------------------------------------------------------------
def _clip_dp_worker(rank, world, port, out_dir):
    """Three clipped resident graphed steps of HRNet-W32 under amp O2 on this rank's GPU, different data per rank."""
    import os

    import torch.distributed as dist

    from tests.test_gpu_dp import _batch
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0",
                      MINDPOSE_AUTOTUNE="0")
    dev = torch.device("cuda", rank)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    torch.manual_seed(0)
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(dev).train()
    mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.create_network_with_loss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True)
    opt = create_optimizer(net, name="adamw", learning_rate=1e-3, weight_decay=0.05, overlap=False, bucket_mb=8.0, clip_norm=1e-4)
    batch = _batch(mp, dev, rank)
    step = GraphedTrainStep(nwl, opt, batch, loss_scale_manager=DynamicLossScaleManager(init_loss_scale=1024.0), warmup=2, resident=True,
                            total_steps=3)
    for _ in range(3):
        step(*batch)
    step.sync()
    torch.cuda.synchronize()
    torch.save(dict(flat=opt.flat.cpu(), clip_state=opt._clip_state.cpu(), stats=opt.grad_clip_stats(), mean_scale=opt.grads.mean_scale),
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    opt.close()
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (one rank per device over RCCL/xGMI)")
def test_two_ranks_agree_on_norm_coefficient_and_parameters(tmp_path):
    import os
    import time

    import torch.multiprocessing as mp_

    from tests.test_gpu_dp import _free_port
    ctx = mp_.spawn(_clip_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 120.0  # the children's time limit: past it they are ended and the test fails
    try:
        while not ctx.join(timeout=1.0):  # raises as soon as one child has failed (and ends the other)
            assert time.monotonic() < deadline, "the two ranks did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
    a, b = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2))
    assert a["mean_scale"] == 0.5 and a["stats"]["measured_steps"] == a["stats"]["clipped_steps"] == 3, a["stats"]
    assert torch.equal(a["clip_state"], b["clip_state"]), (a["stats"], b["stats"])
    assert _same_bits(a["flat"], b["flat"]), "the ranks' parameters differ after three clipped steps"
