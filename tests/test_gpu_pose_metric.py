"""Training-time pose accuracy on the GPU: mp_pose_pck_accuracy (csrc/pose_metric.hip) against the numpy restatement of
tests/test_pose_metric_cpu.py - flags, counters, avg_acc and cnt exactly equal - on the training shape, ragged and misaligned
maps, the threshold-equality pairs of 20 x 20 and more pairs than launch 1's grid holds; the PoseAccuracy meter; and the metric
inside the graph-captured training step, which must leave the step's results bit-equal.

Both inputs and the flags buffer sit between guard bands (NaN for the maps, a byte sentinel for the flags, which also start as the
sentinel): a read outside a map shows up as a NaN - the pair then decodes to (0, 0) and the flags differ - and a pair the launch
skipped as an unwritten byte."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models import metrics  # noqa: E402
from mindpose_amd.utils import AdamWeightDecay, DynamicLossScaleManager, GraphedTrainStep  # noqa: E402
from tests.test_pose_metric_cpu import OracleMeter, pck_oracle  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 256        # elements (maps) / bytes (flags, state) on either side
SENTINEL = 0xA5    # flags and state guard bytes; no flag byte ever takes this value
GRID_CAP = 4096    # launch 1's grid (include/mindpose_hip.h)


class GuardedMaps:
    """fp32 [N, K, H, W] between NaN bands; ``shift`` floats move the tensor off 16-byte alignment."""

    def __init__(self, value, shift=0):
        self.numel = value.size
        self.buf = torch.full((self.numel + 2 * GUARD + shift,), float("nan"), device=DEV)
        self.lo = GUARD + shift
        self.t = self.buf[self.lo:self.lo + self.numel].view(value.shape)
        self.t.copy_(torch.from_numpy(value))
        self.start = self.buf.view(torch.int32).clone()

    def assert_unchanged(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.start), f"{what} was written to"


class GuardedBytes:
    def __init__(self, nbytes, fill, align=8):
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.uint8)
        assert GUARD % align == 0 and self.buf.data_ptr() % align == 0
        self.t = self.buf[GUARD:GUARD + nbytes]
        if fill is not None:
            self.t.fill_(fill)

    def assert_guards(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all(), f"{what}: wrote into a guard band"


def _maps(n, k, h, w, seed):
    """Output and target maps whose values are pairwise distinct within a map (ties occur only where planted): a low random floor
    (part of the output's below zero) and one peak per map, the output's near the target's so that hits and misses both occur."""
    rng = np.random.RandomState(seed)
    hw = h * w
    out = np.empty((n, k, hw), dtype=np.float32)
    tgt = np.empty((n, k, hw), dtype=np.float32)
    for i in range(n):
        for j in range(k):
            out[i, j] = (rng.permutation(hw).astype(np.float32) - hw / 3) / (4 * hw)   # distinct, in [-1/12, 1/6)
            tgt[i, j] = rng.permutation(hw).astype(np.float32) / (4 * hw)              # distinct, in [0, 1/4)
            tx, ty = rng.randint(0, w), rng.randint(0, h)
            px = int(np.clip(tx + rng.randint(-2, 3) * max(1, w // 12), 0, w - 1))
            py = int(np.clip(ty + rng.randint(-2, 3) * max(1, h // 12), 0, h - 1))
            tgt[i, j, ty * w + tx] = 1.0
            out[i, j, py * w + px] = 0.9
    return out.reshape(n, k, h, w), tgt.reshape(n, k, h, w)


def _plant(out, tgt):
    """The named edge cases, where the shape has room for them (maps of at least 6 x 6, K >= 8)."""
    n, k, h, w = out.shape
    if h < 6 or w < 6 or k < 8:
        return
    tgt[0, 0, 3, 3] = 2.0; out[0, 0, 3, 3] = 2.0; out[0, 0, h - 1, w - 1] = 2.0    # two equal maxima: the first index wins (a hit)
    out[0, 1] = -np.abs(out[0, 1]) - 1.0                                            # all-negative output map: (0, 0)
    tgt[0, 2] = 0.0                                                                 # all-zero target: invalid
    tgt[0, 3, 4, 1] = 3.0                                                           # target peak at x = 1: excluded
    tgt[0, 4, 1, 4] = 3.0                                                           # target peak at y = 1: excluded
    tgt[0, 5, 3, 3] = 2.0; out[0, 5, 3, 3] = 2.0; out[0, 5, h - 1, 0] = np.nan      # a NaN anywhere in the output: (0, 0)
    tgt[0, 6, 2, 2] = 2.0; out[0, 6, 2, 2] = np.inf                                 # +inf peak: an ordinary maximum (a hit)
    tgt[:, 7] = 0.0                                                                 # a joint with no valid sample: acc -1, not counted


def _run_kernel(out, tgt, thr=0.5, shift=(0, 0)):
    """One call of the entry on guarded buffers; returns (flags [N, K], header, hits, valid)."""
    n, k, h, w = out.shape
    go, gt = GuardedMaps(out, shift[0]), GuardedMaps(tgt, shift[1])
    flags = GuardedBytes(n * k, None, align=1)
    state = GuardedBytes(metrics.state_bytes(k), 0)
    rc = _lib.load().mp_pose_pck_accuracy(go.t.data_ptr(), gt.t.data_ptr(), n, k, h, w, thr, flags.t.data_ptr(), state.t.data_ptr(),
                                          _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    what = f"[{n}, {k}, {h}, {w}]"
    go.assert_unchanged(what + " output")
    gt.assert_unchanged(what + " target")
    flags.assert_guards(what + " flags")
    state.assert_guards(what + " state")
    f = flags.t.cpu().numpy().reshape(n, k)
    assert not (f == SENTINEL).any(), f"{what}: {(f == SENTINEL).sum()} flag bytes never written"
    head, hits, valid = metrics.parse_state(state.t.cpu().numpy(), k)
    return f, head, hits, valid


def _check(out, tgt, **kw):
    ref = pck_oracle(out, tgt, kw.get("thr", 0.5))
    f, head, hits, valid = _run_kernel(out, tgt, **kw)
    assert np.array_equal(f, ref["flags"]), np.argwhere(f != ref["flags"])[:8]
    assert np.array_equal(hits, ref["hits"]) and np.array_equal(valid, ref["valid"])
    assert float(head["last_avg_acc"]) == ref["avg_acc"] and int(head["last_cnt"]) == ref["cnt"]
    assert int(head["steps"]) == 1 and int(head["sum_cnt"]) == ref["cnt"] and int(head["pad"]) == 0
    assert float(head["sum_acc_cnt"]) == ref["avg_acc"] * float(ref["cnt"])
    return ref


@pytest.mark.parametrize("n,k,h,w", [
    (3, 17, 64, 48),   # the training shape
    (2, 5, 7, 5),      # less than one wave, ragged
    (1, 1, 1, 1),      # smallest input
    (2, 3, 33, 31),    # 1023 elements: 16-byte body plus scalar head and tail, misaligned map starts
    (2, 9, 13, 11),    # ragged, with room for the planted cases
])
def test_kernel_equals_the_oracle(n, k, h, w):
    out, tgt = _maps(n, k, h, w, seed=n * 1000 + h)
    _plant(out, tgt)
    ref = _check(out, tgt)
    if k >= 8 and h >= 6:
        assert ref["flags"][0, :8].tolist() == [3, ref["flags"][0, 1], 0, 0, 0, 1, 3, 0] and ref["acc"][7] == -1.0
        assert ref["cnt"] <= k - 1


@pytest.mark.parametrize("shift", [(1, 0), (2, 3), (3, 1)])
def test_maps_off_16_byte_alignment(shift):
    out, tgt = _maps(2, 9, 16, 12, seed=7)  # hw a multiple of 4: every map starts at the tensor's own misalignment
    _plant(out, tgt)
    _check(out, tgt, shift=shift)


def test_threshold_pairs_at_20x20_follow_the_rule():
    out, tgt = np.zeros((2, 2, 20, 20), dtype=np.float32), np.zeros((2, 2, 20, 20), dtype=np.float32)
    for (i, j), (dx, dy) in {(0, 0): (1, 0), (0, 1): (0, 1), (1, 0): (-1, 0), (1, 1): (0, 0)}.items():
        tgt[i, j, 5, 5] = 1.0
        out[i, j, 5 + dy, 5 + dx] = 1.0
    ref = _check(out, tgt)
    assert ref["flags"].tolist() == [[1, 1], [1, 3]]  # exactly on the threshold is no hit: the inequality is strict
    assert ref["avg_acc"] == 0.25 and ref["cnt"] == 2


@pytest.mark.parametrize("h,w", [(2, 2), (4, 4)])
def test_more_pairs_than_the_grid(h, w):
    n, k = (GRID_CAP + 2 + 2) // 3, 3  # N * K just over the cap: the last pairs are reached by the grid-stride loop only
    assert n * k > GRID_CAP
    out, tgt = _maps(n, k, h, w, seed=11)
    ref = _check(out, tgt)
    assert (ref["valid"].sum() > 0) == (h > 2)  # 2 x 2 maps have no valid pair at all: every flag is a written zero


def test_batch_without_a_valid_pair():
    out, tgt = _maps(2, 4, 8, 6, seed=5)
    ref = _check(out, np.zeros_like(tgt))
    assert ref["cnt"] == 0 and ref["avg_acc"] == 0.0


def test_other_thresholds():
    out, tgt = _maps(3, 6, 16, 12, seed=9)
    flags = {thr: _check(out, tgt, thr=thr)["flags"] for thr in (0.05, 0.5, 2.0)}
    assert not np.array_equal(flags[0.05], flags[2.0])


def test_entry_refuses_before_launching():
    out, tgt = _maps(1, 2, 8, 6, seed=1)
    go, gt = GuardedMaps(out), GuardedMaps(tgt)
    flags, state = GuardedBytes(2, None, align=1), GuardedBytes(metrics.state_bytes(2), 0)
    lib, s = _lib.load(), _lib.stream()
    o, t, f, st = go.t.data_ptr(), gt.t.data_ptr(), flags.t.data_ptr(), state.t.data_ptr()
    assert lib.mp_pose_pck_accuracy(None, t, 1, 2, 8, 6, 0.5, f, st, s) == -1
    assert lib.mp_pose_pck_accuracy(o, None, 1, 2, 8, 6, 0.5, f, st, s) == -1
    assert lib.mp_pose_pck_accuracy(o, t, 1, 2, 8, 6, 0.5, None, st, s) == -1
    assert lib.mp_pose_pck_accuracy(o, t, 1, 2, 8, 6, 0.5, f, None, s) == -1
    assert lib.mp_pose_pck_accuracy(o, t, 1, 0, 8, 6, 0.5, f, st, s) == -2
    assert lib.mp_pose_pck_accuracy(o, t, 1, 2, 4097, 6, 0.5, f, st, s) == -3
    torch.cuda.synchronize()
    assert (flags.t.cpu().numpy() == SENTINEL).all() and not state.t.cpu().numpy().any()  # nothing ran


# ---- the meter ----------------------------------------------------------------------------------------------------------------------------
def test_pose_accuracy_accumulates_and_resets():
    metric = mp.PoseAccuracy()
    meter = OracleMeter(17)
    last = None
    for seed in (21, 22, 23):
        out, tgt = _maps(3, 17, 64, 48, seed=seed)
        _plant(out, tgt)
        if seed == 22:
            tgt[:] = 0.0  # a step that counts nothing
        metric.update(torch.from_numpy(out).to(DEV), torch.from_numpy(tgt).to(DEV))
        last = pck_oracle(out, tgt)
        meter.update(last)
    got = metric.compute()
    assert got["steps"] == 3 and got["count"] == meter.sum_cnt and got["sum_acc_cnt"] == meter.sum_acc_cnt and got["acc"] == meter.acc
    assert got["hits"] == meter.hits.tolist() and got["valid"] == meter.valid.tolist()
    assert metric.sums() == (meter.sum_acc_cnt, meter.sum_cnt, meter.hits.tolist(), meter.valid.tolist())
    assert metric.last() == (last["avg_acc"], last["cnt"])
    acc, avg_acc, cnt = mp.pose_pck_accuracy(torch.from_numpy(out).to(DEV), torch.from_numpy(tgt).to(DEV))
    assert np.array_equal(acc, last["acc"]) and avg_acc == last["avg_acc"] and cnt == last["cnt"]
    metric.reset()
    assert not metric._state.cpu().numpy().any()
    assert metric.compute() == dict(acc=0.0, count=0, steps=0, hits=[0] * 17, valid=[0] * 17, sum_acc_cnt=0.0)


def test_buffers_and_captures(monkeypatch):
    """No allocation during a capture, and none after one: a captured graph replays on the addresses it recorded."""
    metric = mp.PoseAccuracy()
    a = torch.zeros(1, 2, 8, 6, device=DEV)
    with monkeypatch.context() as m:  # (no real capture: the refusal must come before anything is allocated or launched)
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="stream capture"):
            metric.update(a, a)
        assert metric._state is None and metric._flags is None
    metric.update(a, a)  # eager: allocates
    metric.update(torch.zeros(2, 2, 8, 6, device=DEV), torch.zeros(2, 2, 8, 6, device=DEV))  # eager, nothing captured yet: grows
    state, flags = metric._state.data_ptr(), metric._flags.data_ptr()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        metric.update(a, a)
    for shape in ((1, 3, 8, 6), (3, 2, 8, 6)):  # another K, more pairs: would replace what the graph writes to
        with pytest.raises(RuntimeError, match="captured graph"):
            metric.update(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    assert (metric._state.data_ptr(), metric._flags.data_ptr()) == (state, flags)
    metric.reset()
    a[0, 1, 4, 3] = 1.0
    g.replay()
    g.replay()
    got = metric.compute()
    assert got["steps"] == 2 and got["hits"] == [0, 2] and got["valid"] == [0, 2] and got["acc"] == 1.0 and got["count"] == 2


# ---- inside the training step ----------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _batches(n=4, steps=3):
    g = torch.Generator().manual_seed(3)
    make = mp.TopDownGenerateTarget(config=dict(image_size=[192, 256], heatmap_size=[48, 64]), sigma=2.0)
    out = []
    for _ in range(steps):
        x = torch.randn(n, 3, 256, 192, generator=g)
        kp = torch.rand(n, 17, 3, generator=g) * torch.tensor([192.0, 256.0, 2.0])
        target, weight = make(kp.to(DEV))
        out.append((x.to(DEV), target, weight))
    return out


def _run_steps(metric, batches):
    """tests/test_gpu_trainer.py::_run_steps with the resident tail, the metric optional.  Before every step the network runs once
    more in training mode on the step's batch: the parameters are those the step's forward sees and BatchNorm uses the batch's
    statistics, so these are the step's own heat maps."""
    torch.manual_seed(0)
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(DEV).train()
    mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.NetWithLoss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True, metric=metric)
    opt = AdamWeightDecay(net, lr=1e-3, weight_decay=0.05, filter_bias_and_bn=True, overlap=False)
    mgr = DynamicLossScaleManager(2.0 ** 12, 2.0, 2)
    step = GraphedTrainStep(nwl, opt, batches[0], loss_scale_manager=mgr, resident=True, total_steps=len(batches))
    losses, per_step, expect = [], [], []
    for x, target, weight in batches:
        heat = nwl.net(x).detach().clone()
        _, avg_acc, cnt = mp.pose_pck_accuracy(heat, target)
        expect.append((avg_acc, cnt))
        losses.append(step(x, target, weight).detach().clone())
        if metric is not None:
            per_step.append(metric.last())
    step.sync()
    torch.cuda.synchronize()
    out = dict(flat=opt.flat.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), losses=torch.stack(losses),
               mgr=(mgr.loss_scale, mgr.cur_iter, mgr.last_overflow_iter, mgr.skipped_steps), global_step=opt.global_step,
               per_step=per_step, expect=expect, epoch=metric.compute() if metric is not None else None)
    opt.close()
    return out


def test_metric_inside_the_graphed_step(monkeypatch):
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")
    batches = _batches()
    off = _run_steps(None, batches)
    on = _run_steps(mp.PoseAccuracy(), batches)
    for key in ("flat", "m", "v", "losses"):
        assert _same_bits(off[key], on[key]), key
    assert on["mgr"] == off["mgr"] and on["global_step"] == off["global_step"]
    assert on["expect"] == off["expect"]
    assert on["per_step"] == on["expect"], (on["per_step"], on["expect"])
    assert any(cnt > 0 for _, cnt in on["expect"])
    assert on["epoch"]["steps"] == 3  # the warm-up passes were reset away
    assert on["epoch"]["count"] == sum(cnt for _, cnt in on["expect"])
    assert on["epoch"]["sum_acc_cnt"] == sum(a * float(c) for a, c in on["expect"])


# ---- the recipe runner with the key -----------------------------------------------------------------------------------------------------------
def test_runner_logs_the_accuracy(tmp_path, monkeypatch, caplog):
    """`train_accuracy=True` through cli/train.py on the synthetic COCO folder of tests/test_gpu_trainer.py: two epochs of two
    steps, no evaluation.  Every epoch's record carries the accuracy of ITS two steps: the state the trainer reads at an epoch's
    end counts two steps, not the run's so far, and the record holds what was read."""
    import json
    import os

    import mindpose_amd.cli.train as cli_train
    from mindpose_amd.cli.config import parse_args
    from tests.test_gpu_trainer import _argv, _coco_folder
    seen = []

    class Spy(mp.PoseAccuracy):
        def compute(self):
            seen.append(super().compute())
            return seen[-1]

    monkeypatch.setattr(cli_train, "PoseAccuracy", Spy)
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")
    tmp = str(tmp_path)
    data = dict(train_root=os.path.join(tmp, "train"), val_root=os.path.join(tmp, "train"))
    data["train_label"] = data["val_label"] = _coco_folder(data["train_root"], 9, 5, "train.json")
    outdir = os.path.join(tmp, "out")
    with caplog.at_level("INFO"):
        cli_train.train(parse_args(_argv(data, outdir) + ["train_accuracy=True", "val_while_train=False"]))
    with open(os.path.join(outdir, "summary", "summary.jsonl")) as f:
        recs = [json.loads(line) for line in f]
    assert [r["epoch"] for r in recs] == [1, 2] and [r["step"] for r in recs] == [2, 4]
    assert [s["steps"] for s in seen] == [2, 2]  # read once per epoch, reset in between (warm-up and capture not counted)
    for r, s in zip(recs, seen):
        assert 0 < s["count"] <= 2 * 17 and all(0 <= h <= v <= 2 * 4 for h, v in zip(s["hits"], s["valid"])), s  # 2 steps x 4 crops
        assert r["train/acc"] == s["acc"] and r["train/acc_count"] == s["count"], (r, s)
        joints = {f"train/acc_{k}": h / v for k, (h, v) in enumerate(zip(s["hits"], s["valid"])) if v > 0}
        assert joints and {k: v for k, v in r.items() if k.startswith("train/acc_") and k != "train/acc_count"} == joints
        assert np.isfinite(r["train/loss"])
    lines = [m.getMessage() for m in caplog.records if "epoch = " in m.getMessage()]
    assert len(lines) == 2 and all(ln.endswith(f", acc = {s['acc']:.4f}") for ln, s in zip(lines, seen)), lines
