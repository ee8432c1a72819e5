"""The device-resident step tail (csrc/step_end.hip, utils/step_tail.py) against the host-driven one it restates
(utils/loss_scale.py, utils/adamw.py).  Every comparison is bit for bit: the state machine is integer / double host arithmetic
restated on the device, the update launches run the same fp32 body as the host-argument entries (csrc/optim_update.h)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.utils import DynamicLossScaleManager, create_optimizer  # noqa: E402
from mindpose_amd.utils.lr import WarmupCosineDecayLR, WarmupMultiStepDecayLR  # noqa: E402
from mindpose_amd.utils.step_tail import ARGS_DTYPE, STATE_DTYPE, ResidentStepTail, adam_aux_table  # noqa: E402

DEV = torch.device("cuda:0")
ITERS, TABLE = 200, 50  # the 200 iterations apply > 50 updates: the tail of every run reads the tables' last entry


def _dev_bytes(record: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(record.view(np.uint8).copy()).to(DEV)


def _overflow_pattern() -> np.ndarray:
    """Seeded; overflow at iterations 0 .. 39 - from any of the initial scales that reaches the floor of 1.0 (2^24: 24 halvings,
    1000 / 1.5^k: 18) and holds it for at least 15 more - and five in a row at 60 .. 64, after the scale has grown again."""
    over = np.random.RandomState(7).rand(ITERS) < 0.1
    over[0:40] = True
    over[60:65] = True
    return over


@pytest.mark.parametrize("static", [1.0, 128.0])
@pytest.mark.parametrize("mean_scale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("init,factor,window", [(2.0 ** 24, 2.0, 2000), (2.0, 2.0, 1), (8.0, 2.0, 3), (1000.0, 1.5, 2)])
def test_advance_is_the_loss_scale_manager(init, factor, window, mean_scale, static):
    lib = _lib.load()
    mgr = DynamicLossScaleManager(init, factor, window)
    lr_host = (np.random.RandomState(1).rand(TABLE).astype(np.float32) + np.float32(0.5)) * np.float32(1e-3)
    aux_host = adam_aux_table(0.9, 0.999, TABLE)
    lr_dev, aux_dev = torch.from_numpy(lr_host).to(DEV), torch.from_numpy(aux_host).to(DEV)
    st = np.zeros(1, STATE_DTYPE)
    st["loss_scale"], st["last_overflow_iter"] = init, -1
    state_dev = _dev_bytes(st)
    args_dev = torch.zeros(ARGS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    scale_t = torch.zeros((), dtype=torch.float32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    over = _overflow_pattern()
    applied, floor_held, past_table = 0, 0, 0
    for it in range(ITERS):
        flag.fill_(int(over[it]))  # the flag written directly
        _lib.check(lib.mp_train_tail_advance(flag.data_ptr(), state_dev.data_ptr(), factor, window, mean_scale, static, lr_dev.data_ptr(),
                                             TABLE, aux_dev.data_ptr(), TABLE, args_dev.data_ptr(), scale_t.data_ptr(), _lib.stream()),
                   "mp_train_tail_advance")
        # the host expressions of adamw.py, from the manager BEFORE its update
        grad_scale = mean_scale
        grad_scale /= mgr.loss_scale
        want_scale = ctypes.c_float(float(grad_scale) / float(static)).value
        idx = min(applied, TABLE - 1)
        past_table += applied > TABLE - 1
        want_first = float(applied == 0)
        mgr.update_loss_scale(bool(over[it]))
        applied += not over[it]
        floor_held += bool(over[it]) and mgr.loss_scale == 1.0
        a = args_dev.cpu().numpy().view(ARGS_DTYPE)[0]
        s = state_dev.cpu().numpy().view(STATE_DTYPE)[0]
        what = f"iteration {it}"
        assert int(a["skip"]) == int(over[it]), what
        assert a["grad_scale"] == np.float32(want_scale), (what, a["grad_scale"], want_scale)
        assert a["lr"] == lr_host[idx] and a["aux0"] == aux_host[idx, 0] and a["aux1"] == aux_host[idx, 1], what
        assert a["first_step"] == want_first, what
        assert float(s["loss_scale"]) == mgr.loss_scale, (what, s["loss_scale"], mgr.loss_scale)
        assert (int(s["cur_iter"]), int(s["last_overflow_iter"]), int(s["skipped_steps"]), int(s["applied_steps"])) == \
            (mgr.cur_iter, mgr.last_overflow_iter, mgr.skipped_steps, applied), what
        assert scale_t.cpu().numpy() == np.float32(mgr.loss_scale), what
    assert floor_held >= 5 and past_table > 0  # the pattern did reach the floor, and the clamp of the table index was used


def test_advance_without_a_flag_never_skips_or_scales():
    lib = _lib.load()
    lr_dev = torch.tensor([3e-4], dtype=torch.float32, device=DEV)
    st = np.zeros(1, STATE_DTYPE)
    st["loss_scale"], st["last_overflow_iter"], st["cur_iter"], st["applied_steps"] = 1.0, -1, 4, 4
    state_dev = _dev_bytes(st)
    args_dev = torch.zeros(ARGS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    for it in range(3):
        _lib.check(lib.mp_train_tail_advance(None, state_dev.data_ptr(), 2.0, 1, 1.0 / 3.0, 4.0, lr_dev.data_ptr(), 1, None, 0,
                                             args_dev.data_ptr(), None, _lib.stream()), "mp_train_tail_advance")
        a = args_dev.cpu().numpy().view(ARGS_DTYPE)[0]
        s = state_dev.cpu().numpy().view(STATE_DTYPE)[0]
        assert int(a["skip"]) == 0 and a["grad_scale"] == np.float32(ctypes.c_float((1.0 / 3.0) / 4.0).value)
        assert a["lr"] == np.float32(3e-4) and a["aux0"] == 0 and a["aux1"] == 0 and a["first_step"] == 0
        assert float(s["loss_scale"]) == 1.0 and int(s["applied_steps"]) == 5 + it and int(s["cur_iter"]) == 5 + it
        assert int(s["skipped_steps"]) == 0 and int(s["last_overflow_iter"]) == -1


# ---- update launches ---------------------------------------------------------------------------------------------------------------
GUARD = 64
COUNTS = [1, 255, 1027, 1048576 + 4097]  # under a block, ragged, just over the grid cap of 256 * 16 blocks of 256
LR, GRAD_SCALE, WD = np.float32(1e-3), np.float32(1.0 / 3.0 / 1024.0), np.float32(0.05)
AUX = (np.float32(0.9 ** 3), np.float32(0.999 ** 3))
# name -> (kind, hyper as the host entry takes it, first_step); kind 0 = mp_adamw_step_*
RULES = {"adamw": (0, (0.9, 0.999, 1e-6), 0.0),
         "adam": (1, (0.9, 0.999, 1e-8, float(AUX[0]), float(AUX[1])), 0.0),
         "sgd": (2, (0.9, 0.1, 1.0, 0.0, 0.0), 0.0),
         "sgd_first_step": (2, (0.9, 0.1, 1.0, 1.0, 0.0), 1.0),
         "momentum": (3, (0.9, 1.0, 0.0, 0.0, 0.0), 0.0),
         "adagrad": (4, (0.0, 0.0, 0.0, 0.0, 0.0), 0.0)}
_DATA = {}


def _data(count):
    """param, grad, state1, state2 with NaN guard bands, computed once per count and never changed (the tests clone)."""
    if count not in _DATA:
        g = torch.Generator().manual_seed(count)
        bufs = []
        for lo, hi in ((-1.0, 1.0), (-300.0, 300.0), (0.1, 1.0), (0.1, 1.0)):  # states positive: Adam's v, Adagrad's accumulator
            t = torch.full((count + 2 * GUARD,), float("nan"))
            t[GUARD:GUARD + count] = torch.rand(count, generator=g) * (hi - lo) + lo
            bufs.append(t.to(DEV))
        _DATA[count] = bufs
    return _DATA[count]


def _args_block(skip, first_step):
    rec = np.zeros(1, ARGS_DTYPE)
    rec["skip"], rec["grad_scale"], rec["lr"], rec["aux0"], rec["aux1"], rec["first_step"] = skip, GRAD_SCALE, LR, AUX[0], AUX[1], first_step
    return _dev_bytes(rec)


def _run(name, count, bufs, resident, skip=0):
    lib = _lib.load()
    kind, hyper, first = RULES[name]
    p, g, s1, s2 = (t[GUARD:].data_ptr() for t in bufs)
    block = _args_block(skip, first)
    if kind == 0:
        if resident:
            rc = lib.mp_adamw_step_resident(p, g, s1, s2, count, *hyper, float(WD), block.data_ptr(), _lib.stream())
        else:
            rc = lib.mp_adamw_step_scaled(p, g, s1, s2, count, float(LR), *hyper, float(WD), float(GRAD_SCALE), None, _lib.stream())
    else:
        if resident:  # the step-dependent entries come from the block: hand the launch stale ones
            stale = list(hyper)
            if kind == 1:
                stale[3], stale[4] = 0.5, 0.25
            if kind == 2:
                stale[3] = 1.0 - first
            h = (ctypes.c_float * 5)(*stale)
            rc = lib.mp_optimizer_step_resident(kind, p, g, s1, s2, count, float(WD), ctypes.byref(h), block.data_ptr(), _lib.stream())
        else:
            h = (ctypes.c_float * 5)(*hyper)
            rc = lib.mp_optimizer_step(kind, p, g, s1, s2, count, float(LR), float(GRAD_SCALE), float(WD), ctypes.byref(h), _lib.stream())
    _lib.check(rc, f"{name} resident={resident}")
    torch.cuda.synchronize()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", list(RULES))
def test_resident_update_equals_the_host_argument_entry(name, count):
    start = _data(count)
    host, res, skipped = ([t.clone() for t in start] for _ in range(3))
    _run(name, count, host, resident=False)
    _run(name, count, res, resident=True)
    _run(name, count, skipped, resident=True, skip=1)
    assert not _same_bits(host[0], start[0]), "the host entry did not update anything"
    for what, h, r, s, s0 in zip(("param", "grad", "state1", "state2"), host, res, skipped, start):
        assert _same_bits(h, r), f"{name} count {count}: {what} differs from the host-argument entry"
        assert _same_bits(s, s0), f"{name} count {count}: {what} changed under skip = 1"
        for t in (r, s):
            assert torch.isnan(t[:GUARD]).all() and torch.isnan(t[GUARD + count:]).all(), f"{name} count {count}: {what} guard band"
            assert not torch.isnan(t[GUARD:GUARD + count]).any()


# ---- ResidentStepTail against _ArenaOptimizer.step -------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    """Three parameters; ``names`` decide the groups (beta / gamma / bias are not decayed)."""

    def __init__(self, names):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        for name, shape in zip(names, ((33, 7), (129,), (5,))):
            setattr(self, name, torch.nn.Parameter(torch.randn(*shape, generator=g)))


STEPS = 12
OPTIMIZERS = {"adamw": (dict(name="adamw"), lambda: WarmupMultiStepDecayLR(1e-3, 4, 3, [2, 3], warmup=2)),
              "adam": (dict(name="adam", loss_scale=4.0), lambda: WarmupCosineDecayLR(5e-4, 4, 3, warmup=2)),
              "sgd": (dict(name="sgd", momentum=0.9, loss_scale=4.0), lambda: WarmupCosineDecayLR(5e-4, 4, 3, warmup=2))}
GROUPS = {"both": ("weight", "gamma", "bias"), "no_decay_empty": ("w1", "w2", "w3"), "decay_empty": ("gamma", "beta", "bias")}


@pytest.mark.parametrize("names", list(GROUPS))
@pytest.mark.parametrize("which", list(OPTIMIZERS))
def test_resident_tail_equals_optimizer_step(which, names):
    kwargs, schedule = OPTIMIZERS[which]

    def build():
        net = _Toy(GROUPS[names]).to(DEV)
        opt = create_optimizer(net, learning_rate=schedule(), weight_decay=0.05, overlap=False, **kwargs)
        return net, opt, DynamicLossScaleManager(2.0 ** 10, 2.0, 3)

    (_, host, host_mgr), (_, res, res_mgr) = build(), build()
    n = host.flat.numel()
    assert {"both": 0 < host.n_decay < n, "no_decay_empty": host.n_decay == n, "decay_empty": host.n_decay == 0}[names]
    tail = ResidentStepTail(res, res_mgr, STEPS)
    g = torch.Generator().manual_seed(9)
    updated = []
    for it in range(STEPS):
        grad = torch.randn(n, generator=g) * 1000.0
        if it in (0, 5, 6):
            grad[(it * 37) % n] = float("inf")
        for opt in (host, res):
            opt._grad_flat[:n].copy_(grad.to(DEV))
        updated.append(host.step(host_mgr))
        tail.launch()
    assert updated.count(False) == 3 and not updated[0]
    tail.sync()
    assert _same_bits(host.flat, res.flat), "parameters"
    assert len(host.states) == len(res.states)
    for i, (a, b) in enumerate(zip(host.states, res.states)):
        assert _same_bits(a, b), f"state {i}"
    assert not _same_bits(host.flat, build()[1].flat), "nothing was updated"
    for field in ("loss_scale", "cur_iter", "last_overflow_iter", "skipped_steps"):
        assert getattr(res_mgr, field) == getattr(host_mgr, field), field
    assert res.global_step == host.global_step == STEPS - 3
    for opt in (host, res):
        opt.close()
