"""Training-time pose accuracy (PCK), host side: the numpy restatement of the HRNet training code's accuracy() that the GPU tests
compare the kernel with, the integer form of its hit test, and the plumbing of the metric through NetWithLoss, EvalCallback, the
cross-rank combine and the recipe runner.  No GPU."""
import json
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import mindpose_amd as mp
from mindpose_amd import _lib
from mindpose_amd.callbacks import EvalCallback
from mindpose_amd.callbacks.eval_callback import combine_train_accuracy
from mindpose_amd.cli.train import train, train_metric
from mindpose_amd.models import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------
def argmax_xy(m):
    """get_max_preds of the original for one [H, W] map: first row-major index of the maximum, (0, 0) unless the maximum is > 0
    (numpy's max of a map with a NaN is NaN, and NaN > 0 is False)."""
    w = m.shape[1]
    with np.errstate(invalid="ignore"):
        peak = bool(m.max() > 0)
    if not peak:
        return 0, 0
    idx = int(np.argmax(m))
    return idx % w, idx // w


def hit_rule(px, py, tx, ty, h, w, thr=0.5):
    """The exact inequality: every term an integer in double for maps up to 4096 x 4096."""
    dx, dy = int(px) - int(tx), int(py) - int(ty)
    return 100.0 * float((dx * w) ** 2 + (dy * h) ** 2) < thr * thr * float((h * w) ** 2)


def hit_float(px, py, tx, ty, h, w, thr=0.5):
    """The original's float64 form: coordinates divided by norm = (h, w) / 10 - x by h / 10, y by w / 10 - then the distance."""
    norm = np.ones(2) * np.array([h, w]) / 10
    d = np.array([px, py], dtype=np.float64) / norm - np.array([tx, ty], dtype=np.float64) / norm
    return bool(np.linalg.norm(d) < thr)


def pck_oracle(output, target, thr=0.5):
    """accuracy() for [N, K, H, W] float arrays: dict(flags [N, K] uint8 = valid | hit << 1, hits [K], valid [K], acc [K] with -1
    where no pair is valid, avg_acc, cnt)."""
    n, k, h, w = output.shape
    flags = np.zeros((n, k), dtype=np.uint8)
    for i in range(n):
        for j in range(k):
            px, py = argmax_xy(output[i, j])
            tx, ty = argmax_xy(target[i, j])
            valid = tx > 1 and ty > 1
            hit = valid and hit_rule(px, py, tx, ty, h, w, thr)
            flags[i, j] = int(valid) | (int(hit) << 1)
    valid = (flags & 1).astype(np.int64).sum(axis=0)
    hits = ((flags >> 1) & 1).astype(np.int64).sum(axis=0)
    acc = np.full(k, -1.0)
    total, cnt = 0.0, 0
    for j in range(k):
        if valid[j] > 0:
            acc[j] = float(hits[j]) / float(valid[j])
            total += acc[j]
            cnt += 1
    return dict(flags=flags, hits=hits, valid=valid, acc=acc, avg_acc=total / cnt if cnt > 0 else 0.0, cnt=cnt)


class OracleMeter:
    """AverageMeter.update(avg_acc, cnt) of the original plus the per-joint counters."""

    def __init__(self, k):
        self.sum_acc_cnt, self.sum_cnt, self.steps = 0.0, 0, 0
        self.hits, self.valid = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)

    def update(self, res):
        self.sum_acc_cnt += res["avg_acc"] * float(res["cnt"])
        self.sum_cnt += res["cnt"]
        self.steps += 1
        self.hits += res["hits"]
        self.valid += res["valid"]

    @property
    def acc(self):
        return self.sum_acc_cnt / self.sum_cnt if self.sum_cnt > 0 else 0.0


@pytest.mark.parametrize("h,w", [(7, 5), (16, 12)])
def test_integer_rule_equals_the_float_form_on_every_pair(h, w):
    disagree = []
    for t in range(h * w):
        for p in range(h * w):
            px, py, tx, ty = p % w, p // w, t % w, t // w
            if hit_rule(px, py, tx, ty, h, w) != hit_float(px, py, tx, ty, h, w):
                disagree.append((px, py, tx, ty))
    assert not disagree, disagree[:5]


def test_threshold_pairs_at_20x20_are_no_hits_under_the_rule():
    for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1)):
        assert 100.0 * float((dx * 20) ** 2 + (dy * 20) ** 2) == 0.25 * float(400 ** 2)  # exactly on the threshold
        assert not hit_rule(5 + dx, 5 + dy, 5, 5, 20, 20)
    assert hit_rule(5, 5, 5, 5, 20, 20)


def test_oracle_on_planted_maps():
    out, tgt = np.full((2, 3, 8, 6), -1.0), np.zeros((2, 3, 8, 6))
    tgt[0, 0, 4, 3] = 1.0; out[0, 0, 4, 3] = 2.0; out[0, 0, 7, 5] = 2.0    # two equal maxima: the first wins -> hit
    tgt[1, 0, 4, 3] = 1.0; out[1, 0, 4, 3] = 1.0; out[1, 0, 0, 0] = np.nan  # a NaN anywhere -> (0, 0): no hit
    tgt[0, 1, 1, 3] = 1.0; tgt[1, 1, 3, 1] = 1.0                            # y = 1, x = 1: excluded
    tgt[0, 2, 2, 2] = 1.0; out[0, 2, 2, 2] = np.inf                         # +inf is an ordinary maximum
    res = pck_oracle(out, tgt)
    assert res["flags"].tolist() == [[3, 0, 3], [1, 0, 0]]
    assert res["acc"].tolist() == [0.5, -1.0, 1.0] and res["cnt"] == 2 and res["avg_acc"] == 0.75
    assert pck_oracle(out, np.zeros_like(tgt))["avg_acc"] == 0.0 and pck_oracle(out, np.zeros_like(tgt))["cnt"] == 0


# ---- state block, header, entry point ----------------------------------------------------------------------------------------------------
def test_state_block_layout():
    assert metrics.STATE_HEAD_DTYPE.itemsize == 48 and metrics.state_bytes(17) == 48 + 16 * 17
    raw = np.zeros(metrics.state_bytes(3), dtype=np.uint8)
    raw[:48].view(metrics.STATE_HEAD_DTYPE)[0] = (4, 9, 6.5, 0.75, 2, 0)
    raw[48:].view("<i8")[:] = [1, 2, 3, 4, 5, 6]
    head, hits, valid = metrics.parse_state(raw, 3)
    assert (int(head["steps"]), int(head["sum_cnt"]), float(head["sum_acc_cnt"]), float(head["last_avg_acc"]), int(head["last_cnt"])) \
        == (4, 9, 6.5, 0.75, 2)
    assert hits.tolist() == [1, 2, 3] and valid.tolist() == [4, 5, 6]


def test_header_declares_the_entry_and_the_binding_refuses_before_any_launch():
    header = open(os.path.join(ROOT, "include", "mindpose_hip.h")).read()
    assert re.search(r"\bint\s+mp_pose_pck_accuracy\s*\(const float\*", header)
    assert "mp_pose_pck_accuracy" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every call below is refused on the host
    call = lambda **kw: lib.mp_pose_pck_accuracy(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("output", fake), ("target", fake), ("n", 2), ("k", 17), ("h", 64), ("w", 48), ("thr", 0.5), ("flags", fake), ("state", fake),
        ("stream", None))])
    for name in ("output", "target", "flags", "state"):
        assert call(**{name: None}) == -1, name                                  # MP_ERR_NULL
    assert call(k=0) == -2 and call(n=0) == -2 and call(h=0) == -2 and call(thr=0.0) == -2 and call(thr=float("nan")) == -2
    assert call(n=1 << 16, k=1 << 15) == -2                                       # N * K of 2^31
    assert call(h=4097) == -3 and call(w=4097) == -3                              # MP_ERR_UNSUPPORTED
    assert call(output=fake + 2) == -3 and call(state=fake + 4) == -3


def test_metric_is_exported_and_refuses_cpu_tensors():
    assert mp.PoseAccuracy is metrics.PoseAccuracy and mp.pose_pck_accuracy is metrics.pose_pck_accuracy
    assert mp.models.PoseAccuracy is metrics.PoseAccuracy
    m = mp.PoseAccuracy()
    assert m.thr == 0.5 and m.compute() == dict(acc=0.0, count=0, steps=0, hits=[], valid=[], sum_acc_cnt=0.0)
    m.reset()  # nothing allocated yet: a no-op
    with pytest.raises(_lib.MindposeHipError):
        m.update(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))  # no CPU fallback


# ---- NetWithLoss --------------------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))

    def forward(self, x):
        return x * self.w


class _Loss(torch.nn.Module):
    def forward(self, out, label, *extra):
        return ((out - label) ** 2).mean()


class _Recorder:
    def __init__(self):
        self.calls = []

    def update(self, output, target):
        self.calls.append((output, target))


def test_net_with_loss_hands_the_heat_maps_to_the_metric_only_when_asked():
    x, label = torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4)
    plain = mp.NetWithLoss(_Net(), _Loss(), has_extra_inputs=False)
    assert plain.metric is None and mp.create_network_with_loss(_Net(), _Loss()).metric is None
    ref = plain.train()(x, label)
    rec = _Recorder()
    nwl = mp.NetWithLoss(_Net(), _Loss(), has_extra_inputs=False, metric=rec).train()
    loss = nwl(x, label)
    assert torch.equal(loss, ref) and len(rec.calls) == 1
    out, tgt = rec.calls[0]
    assert not out.requires_grad and torch.equal(out, x) and tgt is label
    loss.backward()  # the loss still reaches the network
    assert nwl.net.w.grad is not None
    nwl.eval()(x, label)
    assert len(rec.calls) == 1  # evaluation does not count


# ---- EvalCallback ---------------------------------------------------------------------------------------------------------------------------
def _epoch(cb, net, **kw):
    with cb:
        cb.on_train_step_end(torch.tensor(0.5))
        cb.on_train_epoch_end(1, net, 1e-3, **kw)


def test_eval_callback_writes_the_accuracy_fields(tmp_path, caplog):
    tm = dict(acc=0.625, count=8, steps=4, hits=[6, 0, 9], valid=[8, 0, 12], sum_acc_cnt=5.0)
    with caplog.at_level("INFO"):
        _epoch(EvalCallback(summary_dir=str(tmp_path)), _Net(), train_metrics=tm)
    rec = json.loads(open(tmp_path / "summary.jsonl").read())
    assert rec["train/acc"] == 0.625 and rec["train/acc_count"] == 8
    assert rec["train/acc_0"] == 0.75 and rec["train/acc_2"] == 0.75 and "train/acc_1" not in rec  # joint 1 had no valid pair
    assert any(r.getMessage().endswith("loss = 0.500000, acc = 0.6250") for r in caplog.records)


def test_eval_callback_without_the_metric_writes_the_record_as_before(tmp_path, caplog):
    with caplog.at_level("INFO"):
        _epoch(EvalCallback(summary_dir=str(tmp_path)), _Net())
    rec = json.loads(open(tmp_path / "summary.jsonl").read())
    assert rec == {"step": 1, "epoch": 1, "train/lr": 1e-3, "train/loss": 0.5}
    assert any(r.getMessage() == "[rank = 0] epoch = 1, lr = 1.000e-03, loss = 0.500000" for r in caplog.records)


def test_cross_rank_combine_adds_the_sums_before_dividing():
    a = (1.5, 2, [3, 0, 1], [4, 0, 2])   # rank 0: two joints counted, mean accuracy 0.75
    b = (3.0, 3, [1, 2, 1], [2, 2, 1])   # rank 1: three joints counted, mean accuracy 1.0
    both = combine_train_accuracy([a, b])
    assert both["acc"] == 4.5 / 5 and both["count"] == 5                         # not the mean of 0.75 and 1.0
    assert both["hits"] == [4, 2, 2] and both["valid"] == [6, 2, 3]
    assert both["joint_acc"] == [4 / 6, 1.0, 2 / 3]
    one = combine_train_accuracy([a])
    assert one["acc"] == 0.75 and one["joint_acc"] == [0.75, None, 0.5]
    assert combine_train_accuracy([(0.0, 0, [0], [0])]) == dict(acc=0.0, count=0, hits=[0], valid=[0], joint_acc=[None])


def test_eval_callback_adds_the_sums_over_the_ranks_before_dividing(tmp_path):
    """The path two ranks take: this rank's sums packed into one float64 vector, the all-reduce (here: a stand-in that adds a second
    rank's vector), unpacked, then divided."""
    mine, other = (1.5, 2, [3, 0, 1], [4, 0, 2]), (3.0, 3, [1, 2, 1], [2, 2, 1])
    cb = EvalCallback(summary_dir=str(tmp_path), rank_id=0, device_num=2)
    packed = []

    def all_reduce(v):
        if v.numel() == 1:  # the epoch loss: both ranks the same
            return v * 2
        packed.append(v.tolist())
        return v + torch.tensor([other[0], other[1]] + other[2] + other[3], dtype=v.dtype)

    cb.all_reduce = all_reduce
    tm = dict(acc=0.75, count=mine[1], steps=1, hits=mine[2], valid=mine[3], sum_acc_cnt=mine[0])
    _epoch(cb, _Net(), train_metrics=tm)
    assert packed == [[1.5, 2.0, 3.0, 0.0, 1.0, 4.0, 0.0, 2.0]]  # sum_acc_cnt, sum_cnt, hits[K], valid[K]
    rec = json.loads(open(tmp_path / "summary.jsonl").read())
    both = combine_train_accuracy([mine, other])
    assert rec["train/loss"] == 0.5 and rec["train/acc"] == both["acc"] == 0.9 and rec["train/acc_count"] == 5
    assert [rec[f"train/acc_{k}"] for k in range(3)] == both["joint_acc"] == [4 / 6, 1.0, 2 / 3]


# ---- Trainer ----------------------------------------------------------------------------------------------------------------------------------
class _NoBatches:
    def get_dataset_size(self):
        return 0

    def __iter__(self):
        return iter(())


class _Optimizer:
    lr, global_step, _schedule, clip_norm = 1e-3, 0, None, None  # (an arena optimizer always has the last two)

    def __init__(self):
        from types import SimpleNamespace
        self.grads = SimpleNamespace(overlap=False)


def test_trainer_reads_and_resets_the_metric_once_per_epoch():
    from mindpose_amd.engine import Trainer
    events = []

    class _Metric:
        def compute(self):
            events.append("compute")
            return dict(acc=0.5, epoch_read=events.count("compute"))

        def reset(self):
            events.append("reset")

    class _New:
        def on_train_epoch_end(self, epoch, net, lr, train_metrics=None):
            events.append(("callback", epoch, train_metrics))

    class _Old:  # a callback written before the metric existed
        def on_train_epoch_end(self, epoch, net, lr):
            events.append(("old callback", epoch))

    nwl = mp.NetWithLoss(_Net(), _Loss(), metric=_Metric())
    Trainer(nwl, _Optimizer(), resident=False).train(2, _NoBatches(), callbacks=[_New()])
    assert events == ["compute", "reset", ("callback", 1, dict(acc=0.5, epoch_read=1)),
                      "compute", "reset", ("callback", 2, dict(acc=0.5, epoch_read=2))]
    del events[:]
    Trainer(mp.NetWithLoss(_Net(), _Loss()), _Optimizer(), resident=False).train(1, _NoBatches(), callbacks=[_Old(), _New()])
    assert events == [("old callback", 1), ("callback", 1, None)]  # no metric: the keyword is not passed at all


# ---- the recipe runner ------------------------------------------------------------------------------------------------------------------------
def test_cli_key_builds_the_metric_for_topdown_and_is_refused_for_bottomup():
    assert train_metric(Namespace(pipeline_method="topdown")) is None
    assert train_metric(Namespace(pipeline_method="bottomup", train_accuracy=False)) is None
    metric = train_metric(Namespace(pipeline_method="topdown", train_accuracy=True))
    assert isinstance(metric, mp.PoseAccuracy) and metric.thr == 0.5
    with pytest.raises(ValueError, match="train_accuracy.*topdown"):
        train_metric(Namespace(pipeline_method="bottomup", train_accuracy=True))
    with pytest.raises(ValueError, match="train_accuracy.*topdown"):  # the runner refuses before it opens anything
        train(Namespace(pipeline_method="bottomup", train_accuracy=True))
