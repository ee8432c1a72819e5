"""The training step under every documented switch and stream layout (INTEGRATION.md "Switches (environment)").

Part 1 - stream order, deterministically (tests/stream_audit.py): the eager `HRNet.train_forward` with the branch side streams on,
under all four combinations of MINDPOSE_TRAIN_FUSE_STREAMS x MINDPOSE_TRAIN_CHAIN_MODULES, must read no tensor on a stream that is
not ordered behind the launch that wrote it.  Before `HRNet.train_forward` made chaining depend on where the rows run, the
(FUSE_STREAMS=0, chained) case reported every branch i > 0 of the modules 1.. of stages 3 and 4 (27 reads, first lines):

    stage3.1.branches.1.0: input read without an order: producer stream main (produced at stage3.0.fuse_layers.1) -> consumer stream side0, no wait in between
    stage3.1.branches.2.0: input read without an order: producer stream main (produced at stage3.0.fuse_layers.2) -> consumer stream side1, no wait in between
    ...
    stage4.1.branches.3.0: input read without an order: producer stream main (produced at stage4.0.fuse_layers.3) -> consumer stream side2, no wait in between

Part 2 - values.  Class A rows are documented "same bits": a freshly built network, one `GraphedTrainStep` capture and two replays
per setting, gradient arena and loss `torch.equal` to the eager single-stream all-defaults step (the baseline of
tests/test_gpu_train_f16.py::test_graphed_o2_step_equals_eager: 4x3x64x64, loss scale 4096).  Class B rows are not: they are tried
for equal bits first and otherwise held to the CPU oracle (tests/train_oracle.py), with their distance to the default step
printed.  Every row also shows that its switch took effect where the code offers a handle (autograd node counts, MP_CONV_PHASES4
launches, early-flush calls, the streams and edges the audit saw); a row without a handle says so.

Each configuration is captured once; nothing here retries.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models import train_ops as T  # noqa: E402
from mindpose_amd.models.backbones import hrnet as H  # noqa: E402
from tests.stream_audit import audit_train_forward  # noqa: E402

DEV = torch.device("cuda:0")
SCALE = 4096.0
SWITCHES = ["MINDPOSE_FAN_OUT_ONE_NODE", "MINDPOSE_WGRAD_EARLY_FLUSH", "MINDPOSE_DGRAD_PHASES4", "MINDPOSE_TRAIN_BRANCH_STREAMS",
            "MINDPOSE_TRAIN_FUSE_STREAMS", "MINDPOSE_TRAIN_CHAIN_MODULES", "MINDPOSE_WGRAD_GROUP", "MINDPOSE_FAN_OUT",
            "MINDPOSE_BN16_MASK_FROM_Z", "MINDPOSE_FUSE_RESIDUAL", "MINDPOSE_FUSE_BLOCK", "MINDPOSE_FUSE_BLOCK64", "MINDPOSE_HIP_GRAPH",
            "MINDPOSE_PLAN_LANES", "MINDPOSE_BN_FUSE", "MINDPOSE_BN_FUSE_PARTS"]


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    """Every test starts from the defaults: the rows set their own switch through monkeypatch (all are read at call time)."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _assert_defaults():
    assert not [n for n in SWITCHES if n in os.environ]


def _build(amp):
    from mindpose_amd.utils import AdamWeightDecay
    torch.manual_seed(0)
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(DEV).train()
    if amp:
        mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.create_network_with_loss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True)
    opt = AdamWeightDecay(net, lr=1e-3, weight_decay=0.05, filter_bias_and_bn=True, overlap=False)
    return net, nwl, opt


def _batch(n=4):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 3, 64, 64, generator=g).to(DEV)
    kp = (torch.rand(n, 17, 3, generator=g) * torch.tensor([64.0, 64.0, 2.0])).to(DEV)
    target, weight = mp.TopDownGenerateTarget(config=dict(image_size=[64, 64], heatmap_size=[16, 16]), sigma=2.0)(kp)
    return x, target, weight


def _node_counts(loss):
    """Autograd nodes by class name, walked from ``loss.grad_fn``."""
    seen, todo, counts = set(), [loss.grad_fn], {}
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        name = type(fn).__name__
        counts[name] = counts.get(name, 0) + 1
        todo += [f for f, _ in fn.next_functions]
    return counts


class _Launches:
    """Counts through the library's own launch helpers: MP_CONV_PHASES4 launches / four-phase launches of the stride-2 data gradient,
    weight-gradient groups that left on the early-flush side stream."""

    def __init__(self, m):
        self.phases4 = self.phase = self.early = self.flushes = 0
        real_plain, real_stats, real_flush = T._conv16_launch, T._conv16_stats_launch, T._wgrad_flush_key

        def plain(lib, d, *a, **k):
            self._count(d)
            return real_plain(lib, d, *a, **k)

        def stats(lib, d, *a, **k):
            self._count(d)
            return real_stats(lib, d, *a, **k)

        def flush(lib, key, joined=False):
            self.early += int(joined)
            self.flushes += 1
            return real_flush(lib, key, joined)

        m.setattr(T, "_conv16_launch", plain)
        m.setattr(T, "_conv16_stats_launch", stats)
        m.setattr(T, "_wgrad_flush_key", flush)

    def _count(self, d):
        if d.flags & _lib.MP_CONV_PHASES4:
            self.phases4 += 1
        elif d.out_mul == 2 and d.kh == 2:
            self.phase += 1


def _eager(amp, monkeypatch, branch_streams=False):
    """One eager step: (loss, gradient arena, per-parameter gradients, autograd node counts, launch counts)."""
    x, target, weight = _batch()
    net, nwl, opt = _build(amp)
    with monkeypatch.context() as m:
        seen = _Launches(m)
        prev = H.set_branch_streams(branch_streams)
        try:
            with H.quiet_accumulate_grad_stream_warning():
                opt.zero_grad()
                loss = nwl(x, target, weight)
                nodes = _node_counts(loss)
                (loss * SCALE).backward()
                torch.cuda.synchronize()
        finally:
            H.set_branch_streams(prev)
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    return dict(loss=float(loss.detach()), arena=opt.grads.arena.clone(), grads=grads, nodes=nodes, seen=seen)


def _captured(amp, monkeypatch, segments=None):
    """A freshly built network and optimizer, ONE capture, two replays: (loss, arena) of each replay + what the capture launched."""
    from mindpose_amd.utils import DynamicLossScaleManager, GraphedTrainStep
    x, target, weight = _batch()
    net, nwl, opt = _build(amp)
    with monkeypatch.context() as m:
        seen = _Launches(m)
        step = GraphedTrainStep(nwl, opt, (x, target, weight), loss_scale_manager=DynamicLossScaleManager(init_loss_scale=SCALE),
                                warmup=2, segments=segments)
    nodes = _node_counts(step.static_loss) if step.segments == 1 else {}
    runs = []
    for _ in range(2):
        step.replay(exchange=False)
        torch.cuda.synchronize()
        runs.append((float(step.static_loss.detach()), opt.grads.arena.clone()))
    return dict(runs=runs, nodes=nodes, seen=seen, step=step)


def _audit(amp, n=2, branch_streams=True):
    """The audited eager forward (2x3x64x64) under the current environment."""
    x, _, _ = _batch(n)
    net, _, _ = _build(amp)
    mpatch = pytest.MonkeyPatch()
    prev = H.set_branch_streams(branch_streams)
    try:
        with mpatch.context() as m, audit_train_forward(m, net.backbone) as audit:
            out = net(x)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
    finally:
        H.set_branch_streams(prev)
    return audit


@pytest.fixture(scope="module")
def baseline_o2():
    _assert_defaults()
    return _eager(True, pytest.MonkeyPatch())


@pytest.fixture(scope="module")
def baseline_f32():
    _assert_defaults()
    return _eager(False, pytest.MonkeyPatch())


@pytest.fixture(scope="module")
def default_audit():
    _assert_defaults()
    return _audit(True)


def _same_bits(got, base, what):
    for i, (loss, arena) in enumerate(got["runs"]):
        assert loss == base["loss"], (what, i, loss, base["loss"])
        assert torch.equal(arena, base["arena"]), f"{what}: replay {i} differs from the eager all-defaults step"
    assert torch.equal(got["runs"][0][1], got["runs"][1][1]), f"{what}: two replays differ"


# ---- part 1: the stream-order audit --------------------------------------------------------------------------------------------------

def _row_streams(audit):
    return {audit.labels.get(s, s) for s in audit.streams_of["row"]}


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "o2"])
@pytest.mark.parametrize("fuse,chain", [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")])
def test_stream_order_of_train_forward(monkeypatch, amp, fuse, chain):
    monkeypatch.setenv("MINDPOSE_TRAIN_FUSE_STREAMS", fuse)
    monkeypatch.setenv("MINDPOSE_TRAIN_CHAIN_MODULES", chain)
    audit = _audit(amp)
    print(f"FUSE_STREAMS={fuse} CHAIN_MODULES={chain}: {audit.checked} reads checked, {len(audit.edges)} wait_stream edges, "
          f"{len(audit.violations)} violations\n{audit.report()}")
    assert audit.checked > 300 and len(audit.edges) > 20  # the wrappers saw the network
    assert not audit.violations, audit.report()
    # the switches took effect: where the rows ran, and how many forks / joins were issued
    assert _row_streams(audit) == ({"main"} if fuse == "0" else {"main", "side0", "side1", "side2"})
    assert {audit.labels.get(s, s) for s in audit.streams_of["block"]} == {"main", "side0", "side1", "side2"}
    # 8 modules; per module a fork and a join per side branch; with the rows on the side streams a fork per side row, and their join
    # unless the next module of the stage is chained to them
    n_branch = 1 + 4 * 2 + 3 * 3   # side branches over all modules: stage 2 (one module), 3 (four), 4 (three)
    n_rows = 1 + 4 * 2 + 2 * 3     # side rows (the last module of stage 4 has one row)
    chained = fuse == "1" and chain == "1"
    forks = n_branch - ((3 * 2 + 2 * 3) if chained else 0)
    joins = n_branch
    if fuse == "1":
        forks += n_rows
        joins += n_rows - ((3 * 2 + 2 * 3) if chained else 0)
    assert len(audit.edges) == forks + joins, (len(audit.edges), forks, joins)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "o2"])
def test_stream_order_audit_on_one_stream_is_trivially_clean(amp):
    audit = _audit(amp, branch_streams=False)
    assert audit.checked > 300 and not audit.edges and not audit.violations, audit.report()
    assert all(len(v) == 1 for v in audit.streams_of.values()) and len(set.union(*audit.streams_of.values())) == 1
    assert {"block", "row", "conv_bn_seq", "fan_out_many", "grad_join", "fuse_sum", "conv_bn_act"} <= set(audit.streams_of)


# ---- part 2, class A: documented "same bits" -----------------------------------------------------------------------------------------

def test_captured_step_with_fan_out_one_node_off(monkeypatch, baseline_o2):
    assert baseline_o2["nodes"].get("FanOutManyFnBackward", 0) >= 7 and baseline_o2["nodes"].get("GradJoinFnBackward", 0) == 1
    monkeypatch.setenv("MINDPOSE_FAN_OUT_ONE_NODE", "0")
    got = _captured(True, monkeypatch)
    assert "FanOutManyFnBackward" not in got["nodes"] and "GradJoinFnBackward" not in got["nodes"]  # the switch took effect
    assert got["nodes"]["FanOutFnBackward"] > baseline_o2["nodes"].get("FanOutFnBackward", 0)
    _same_bits(got, baseline_o2, "MINDPOSE_FAN_OUT_ONE_NODE=0")
    eager = _eager(True, monkeypatch)
    assert "FanOutManyFnBackward" not in eager["nodes"]
    assert eager["loss"] == baseline_o2["loss"] and torch.equal(eager["arena"], baseline_o2["arena"])


def test_captured_step_with_wgrad_early_flush_off(monkeypatch, baseline_o2):
    assert baseline_o2["seen"].early > 0
    monkeypatch.setenv("MINDPOSE_WGRAD_EARLY_FLUSH", "0")
    got = _captured(True, monkeypatch)
    assert got["seen"].early == 0  # no group left on the side stream of the early flush
    _same_bits(got, baseline_o2, "MINDPOSE_WGRAD_EARLY_FLUSH=0")
    eager = _eager(True, monkeypatch)
    assert eager["seen"].early == 0
    assert eager["loss"] == baseline_o2["loss"] and torch.equal(eager["arena"], baseline_o2["arena"])


def test_captured_step_with_dgrad_phases4_off(monkeypatch, baseline_o2):
    """Four phase launches against the one MP_CONV_PHASES4 launch.  The one launch of a fused chain also masks the gradient and
    leaves the BatchNorm backward sums of the layer below (MINDPOSE_BN_FUSE_PARTS bit 16).  The four launches used to leave those
    sums to the BatchNorm kernel's own reduction - another order: loss equal, gradients up to 3.5e-3 of a tensor's max-norm away
    (7.8e-4 in the median), within the oracle's acceptance but not the "same bits" the switch is documented with.  Each phase now
    runs the merged launch's variant and fills its quarter of the merged launch's partial sums."""
    assert baseline_o2["seen"].phases4 > 0 and baseline_o2["seen"].phase == 0
    monkeypatch.setenv("MINDPOSE_DGRAD_PHASES4", "0")
    got = _captured(True, monkeypatch)
    # three passes (two warm-up, one captured) of four launches where the default step has one MP_CONV_PHASES4 launch
    assert got["seen"].phases4 == 0 and got["seen"].phase == 3 * 4 * baseline_o2["seen"].phases4
    _same_bits(got, baseline_o2, "MINDPOSE_DGRAD_PHASES4=0")
    eager = _eager(True, monkeypatch)
    assert eager["seen"].phases4 == 0 and eager["seen"].phase == 4 * baseline_o2["seen"].phases4
    assert eager["loss"] == baseline_o2["loss"] and torch.equal(eager["arena"], baseline_o2["arena"])


def test_dgrad_phases4_off_without_batchnorm_sums_from_the_data_gradient(monkeypatch, baseline_o2):
    """The same with MINDPOSE_BN_FUSE_PARTS=15 on both sides (the data-gradient launches are plain ones, each phase with its own tuned
    variant): captured and eager, bit for bit."""
    monkeypatch.setenv("MINDPOSE_BN_FUSE_PARTS", "15")
    base15 = _eager(True, monkeypatch)
    assert base15["seen"].phases4 == baseline_o2["seen"].phases4 and base15["seen"].phase == 0 and base15["loss"] == baseline_o2["loss"]
    monkeypatch.setenv("MINDPOSE_DGRAD_PHASES4", "0")
    got = _captured(True, monkeypatch)
    assert got["seen"].phases4 == 0 and got["seen"].phase == 3 * 4 * baseline_o2["seen"].phases4
    _same_bits(got, base15, "MINDPOSE_DGRAD_PHASES4=0, MINDPOSE_BN_FUSE_PARTS=15")
    eager = _eager(True, monkeypatch)
    assert eager["seen"].phases4 == 0 and eager["seen"].phase == 4 * baseline_o2["seen"].phases4
    assert eager["loss"] == base15["loss"] and torch.equal(eager["arena"], base15["arena"])


STREAM_ROWS = [dict(MINDPOSE_TRAIN_FUSE_STREAMS="0"), dict(MINDPOSE_TRAIN_CHAIN_MODULES="0"),
               dict(MINDPOSE_TRAIN_FUSE_STREAMS="0", MINDPOSE_TRAIN_CHAIN_MODULES="0"), dict(MINDPOSE_TRAIN_BRANCH_STREAMS="0")]
_ids = lambda env: "-".join(f"{k[len('MINDPOSE_'):]}={v}" for k, v in env.items())  # noqa: E731


def _stream_switch_took_effect(env, default_audit):
    """The audited eager forward under ``env`` against the one under the defaults: other streams for the rows, or other edges."""
    audit = _audit(True)
    assert not audit.violations, audit.report()
    if env.get("MINDPOSE_TRAIN_BRANCH_STREAMS") == "0":
        assert not audit.edges and len(set.union(*audit.streams_of.values())) == 1
    elif env.get("MINDPOSE_TRAIN_FUSE_STREAMS") == "0":
        assert _row_streams(audit) == {"main"} and _row_streams(default_audit) == {"main", "side0", "side1", "side2"}
    else:
        assert _row_streams(audit) == _row_streams(default_audit) and len(audit.edges) > len(default_audit.edges)


@pytest.mark.parametrize("env", STREAM_ROWS, ids=_ids)
def test_captured_o2_step_under_stream_switches(monkeypatch, baseline_o2, default_audit, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _stream_switch_took_effect(env, default_audit)
    _same_bits(_captured(True, monkeypatch), baseline_o2, _ids(env))


@pytest.mark.parametrize("env", STREAM_ROWS[:2], ids=_ids)
def test_captured_fp32_step_under_stream_switches(monkeypatch, baseline_f32, env):
    """(the audit of these two settings on the fp32 network is test_stream_order_of_train_forward[...-fp32])"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same_bits(_captured(False, monkeypatch), baseline_f32, "fp32 " + _ids(env))


@pytest.mark.parametrize("env", STREAM_ROWS[:2], ids=_ids)
def test_segmented_o2_step_under_stream_switches(monkeypatch, baseline_o2, env):
    """Four captured segments: `join_branch_streams` is the only join at a cut, whatever streams the rows and the modules used.
    (No handle of its own: the switches' effect on the forward is shown by the one-graph rows above.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = _captured(True, monkeypatch, segments=4)
    assert got["step"].segments == 4 and len(got["step"].graphs) == 4
    _same_bits(got, baseline_o2, "segments=4 " + _ids(env))


def test_eager_step_with_branch_streams_equals_eager_without(monkeypatch, baseline_o2):
    """MINDPOSE_TRAIN_BRANCH_STREAMS=1 outside a capture: forward and backward with the branches and rows on side streams."""
    monkeypatch.setenv("MINDPOSE_TRAIN_BRANCH_STREAMS", "1")
    audit = _audit(True, branch_streams=False)  # the environment alone turns the side streams on
    assert _row_streams(audit) == {"main", "side0", "side1", "side2"} and not audit.violations, audit.report()
    eager = _eager(True, monkeypatch)
    assert eager["loss"] == baseline_o2["loss"] and torch.equal(eager["arena"], baseline_o2["arena"])


# ---- part 2, class B: not documented as same bits ------------------------------------------------------------------------------------

def _distance(grads, base):
    """Per tensor: max-norm distance to the default step's gradient relative to that gradient's max-norm -> (largest, median, name)."""
    rel = {}
    for k, g in base.items():
        rel[k] = float((grads[k] - g).abs().max() / g.abs().max().clamp_min(1e-30))
    worst = max(rel, key=rel.get)
    return rel[worst], float(torch.tensor(list(rel.values())).median()), worst


def _oracle_yardstick(what):
    from tests import train_oracle
    loss, got = train_oracle.hip_step()
    train_oracle.check_against_oracle(loss, got, what)


CLASS_B = [("MINDPOSE_WGRAD_GROUP", "1"), ("MINDPOSE_WGRAD_GROUP", "3"), ("MINDPOSE_FAN_OUT", "0"), ("MINDPOSE_BN16_MASK_FROM_Z", "0"),
           ("MINDPOSE_FUSE_RESIDUAL", "0")]
# what the matrix measured ("The step under its switches"): these reproduce the default step bit for bit at this
# shape and are pinned like class A.  (MINDPOSE_WGRAD_GROUP: the grouped launch cuts every layer's pixels into the slabs the
# one-layer launch uses at 4x3x64x64 - at other sizes the split-K partition may differ, tests/test_gpu_train_f16.py allows 2e-5.)
# MINDPOSE_FAN_OUT=0 rounds every pairwise fp16 add: held to the oracle.
SAME_BITS_B = {("MINDPOSE_WGRAD_GROUP", "1"), ("MINDPOSE_WGRAD_GROUP", "3"), ("MINDPOSE_BN16_MASK_FROM_Z", "0"),
               ("MINDPOSE_FUSE_RESIDUAL", "0")}


@pytest.mark.parametrize("name,value", CLASS_B, ids=[f"{n[len('MINDPOSE_'):]}={v}" for n, v in CLASS_B])
def test_eager_o2_step_under_class_b_switch(monkeypatch, baseline_o2, name, value):
    monkeypatch.setenv(name, value)
    eager = _eager(True, monkeypatch)
    # the switch took effect
    if name == "MINDPOSE_FAN_OUT":
        assert baseline_o2["nodes"].get("FanOutManyFnBackward", 0) > 0
        assert not any(k.startswith(("FanOutFn", "FanOutManyFn")) for k in eager["nodes"])
    elif name == "MINDPOSE_WGRAD_GROUP":
        # smaller groups = more weight-gradient launches (every layer of this network has an fp16 weight gradient)
        assert T._wgrad_group_size() == int(value) != T.WGRAD_GROUP and eager["seen"].flushes > baseline_o2["seen"].flushes
        assert value != "1" or eager["seen"].flushes > 200
    elif name == "MINDPOSE_FUSE_RESIDUAL":
        # no effect to show under amp O2 with the defaults: the fused chains (MINDPOSE_BN_FUSE) take every residual block before this
        # switch is read - the row pins exactly that; the per-cell form is compared at block level under MINDPOSE_BN_FUSE=0
        # (tests/test_gpu_train_f16.py) and at step level in fp32 below
        assert not any(k.startswith("ResidualBlock") for k in baseline_o2["nodes"])
    # (MINDPOSE_BN16_MASK_FROM_Z: no handle - the switch only changes which pointer the BatchNorm backward launch receives)
    equal = eager["loss"] == baseline_o2["loss"] and torch.equal(eager["arena"], baseline_o2["arena"])
    worst, median, where = _distance(eager["grads"], baseline_o2["grads"])
    print(f"class B {name}={value}: equal bits {equal}; per-tensor max-norm distance to the default step / gradient max-norm: "
          f"largest {worst:.3e} ({where}), median {median:.3e}")
    assert eager["loss"] == baseline_o2["loss"]  # none of these touches the forward pass
    if (name, value) in SAME_BITS_B:
        assert equal, f"{name}={value} is pinned as same bits"
    else:
        _oracle_yardstick(f"O2 step, {name}={value}")


def test_eager_fp32_step_with_fuse_residual_off(monkeypatch, baseline_f32):
    """fp32 is where MINDPOSE_FUSE_RESIDUAL decides: `ResidualBlock32Fn` (identity gradient added in the first conv's data-gradient
    epilogue) against the per-cell nodes (autograd adds it with its own kernel).  One fp32 add of the same two operands either way."""
    n_blocks = baseline_f32["nodes"].get("ResidualBlock32FnBackward", 0)
    assert n_blocks > 50
    monkeypatch.setenv("MINDPOSE_FUSE_RESIDUAL", "0")
    eager = _eager(False, monkeypatch)
    assert "ResidualBlock32FnBackward" not in eager["nodes"]
    worst, median, where = _distance(eager["grads"], baseline_f32["grads"])
    equal = torch.equal(eager["arena"], baseline_f32["arena"])
    print(f"class B fp32 MINDPOSE_FUSE_RESIDUAL=0: equal bits {equal}; largest per-tensor distance {worst:.3e} ({where}), median {median:.3e}")
    assert eager["loss"] == baseline_f32["loss"]
    assert equal


# ---- inference switches --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def inference_default():
    _assert_defaults()
    return _infer()


def _infer(runs=1):
    torch.manual_seed(0)
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(DEV).eval()
    mp.models.auto_mixed_precision(net, "O2")
    x = torch.randn(3, 3, 256, 192, generator=torch.Generator().manual_seed(17)).to(DEV)
    outs = []
    for _ in range(runs):
        outs.append(net(x).clone())
    torch.cuda.synchronize()
    plan = net.get_plan(x.shape, x.device)
    return dict(outs=outs, info=list(plan.layer_info), plan=plan)


def _fused_blocks(info):
    return sorted(e["cin"] for e in info if e["kind"] == "basicblock_f16")


def test_inference_with_fuse_block_off(monkeypatch, inference_default):
    widths = _fused_blocks(inference_default["info"])
    assert 32 in widths and (64 in widths or 128 in widths), widths
    monkeypatch.setenv("MINDPOSE_FUSE_BLOCK", "0")
    got = _infer()
    assert not _fused_blocks(got["info"])  # the plan changed: every fused block is two conv entries now
    assert len(got["info"]) == len(inference_default["info"]) + len(widths)
    assert torch.equal(got["outs"][0], inference_default["outs"][0])


def test_inference_with_fuse_block64_off(monkeypatch, inference_default):
    widths = _fused_blocks(inference_default["info"])
    monkeypatch.setenv("MINDPOSE_FUSE_BLOCK64", "0")
    got = _infer()
    assert any(c in (64, 128) for c in widths)
    assert _fused_blocks(got["info"]) == [c for c in widths if c not in (64, 128)] and 32 in _fused_blocks(got["info"])
    assert len(got["info"]) == len(inference_default["info"]) + sum(1 for c in widths if c in (64, 128))
    assert torch.equal(got["outs"][0], inference_default["outs"][0])


def test_inference_on_one_lane_from_a_hip_graph(monkeypatch, inference_default):
    assert any(e["kind"] == "barrier" for e in inference_default["info"]) and inference_default["plan"]._multi
    monkeypatch.setenv("MINDPOSE_PLAN_LANES", "0")
    monkeypatch.setenv("MINDPOSE_HIP_GRAPH", "1")
    got = _infer(runs=4)
    assert not any(e["kind"] == "barrier" for e in got["info"]) and not got["plan"]._multi  # one lane
    assert got["plan"]._graph is not None  # runs 3 and 4 replayed the captured graph
    for out in got["outs"]:
        assert torch.equal(out, inference_default["outs"][0])
