"""The OHKM joint MSE on the GPU (csrc/joints_loss.hip, models/loss/ohkm.py) against the float64 restatement of
tests/ohkm_restated.py: row sums, selection, loss and gradient on the smallest shapes at which a kernel can go wrong (one element,
odd HW, one past a wave of joints, the LDS ranking up to K = 1024, more samples than the final reduction has threads), the tie and
NaN rules of the order, the rows the backward must not read, known answers, the C ABI's refusals, the loss inside the graph-captured
training step, and the recipe runner with the two --cfg-options.

TOLERANCES (those test_loss_fwd_bwd holds joint_mse to): row sums and loss 1e-6 relative to float64, gradient
rtol 1e-6 / atol 1e-12 with exact zero bits in rows that are not selected, selection exactly equal.

The C-ABI runs keep pred and target between NaN bands (a read outside a tensor turns a row sum into NaN and the selection differs)
and every output between sentinel bands that must come back untouched."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.utils import AdamWeightDecay, DynamicLossScaleManager, GraphedTrainStep  # noqa: E402
from tests import ohkm_restated as R  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 256  # elements on either side of a guarded tensor
PATTERN = {torch.float32: -12345.0, torch.uint8: 0xA5, torch.float64: -12345.0}


class Guarded:
    """A contiguous tensor between guard bands; ``shift`` elements move it off 16-byte alignment.  Inputs: NaN bands.  Outputs:
    bands and body pre-filled with a pattern."""

    def __init__(self, shape, dtype=torch.float32, value=None, shift=0):
        numel = int(np.prod(shape))
        fill = float("nan") if value is not None else PATTERN[dtype]
        self.buf = torch.full((numel + 2 * GUARD + shift,), fill, device=DEV, dtype=dtype)
        self.lo, self.numel = GUARD + shift, numel
        self.t = self.buf[self.lo:self.lo + numel].view(shape)
        if value is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(value)))
        self.start = self.buf.clone()

    def _bits(self, t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t

    def assert_unchanged(self, what):
        assert torch.equal(self._bits(self.buf), self._bits(self.start)), f"{what} was written to"

    def assert_guards(self, what):
        for band, ref in ((self.buf[:self.lo], self.start[:self.lo]), (self.buf[self.lo + self.numel:], self.start[self.lo + self.numel:])):
            assert torch.equal(self._bits(band), self._bits(ref)), f"{what}: wrote into a guard band"


def _inputs(n, k, h, w, seed, weighted):
    """target + a[n,k] * noise: the row sums of every sample form a shuffled geometric ladder (ratio 1 + max(2e-3, 2 / K) between
    neighbours), so that the order of the fp32 sums is the order of the float64 ones.  The noise of a row has unit mean square; with
    weights (0.5, 1, 2.5, and one 0 per sample when K > 1) the amplitude takes the weight out again, so the weighted sums form the
    ladder."""
    rng = np.random.RandomState(seed)
    hw = h * w
    target = rng.rand(n, k, h, w).astype(np.float32)
    noise = rng.randn(n, k, hw)
    noise /= np.sqrt((noise ** 2).mean(axis=2, keepdims=True))
    step = max(2e-3, 2.0 / k)
    rungs = np.stack([rng.permutation(k) for _ in range(n)]).astype(np.float64)
    want = 0.02 * (1.0 + step) ** rungs / hw  # mean squared error of the row, times its weight
    weight = None
    if weighted:
        weight = rng.choice([0.5, 1.0, 2.5], size=(n, k)).astype(np.float32)
        amp = np.sqrt(want / weight)
        if k > 1:
            weight[np.arange(n), rng.randint(0, k, n)] = 0.0
    else:
        amp = np.sqrt(want)
    pred = (target + (amp[..., None] * noise).reshape(n, k, h, w)).astype(np.float32)
    return pred, target, weight


def _assert_separated(s):
    """The precondition on the inputs: adjacent sorted row sums of a sample differ by more than 1e-4 relative."""
    for row in np.asarray(s, dtype=np.float64):
        srt = np.sort(row)
        gaps = np.diff(srt)
        assert (gaps > 1e-4 * np.abs(srt[1:])).all(), "inputs: two row sums of a sample are closer than 1e-4 relative"


def _raw_fwd(pred, target, weight, topk, shift=0):
    """mp_joints_ohkm_fwd through the C ABI on guarded buffers: (loss, row_sum, sel) as numpy plus the device tensors for the backward."""
    lib = _lib.load()
    n, k, h, w = pred.shape
    gp, gt = Guarded(pred.shape, value=pred, shift=shift), Guarded(pred.shape, value=target, shift=shift)
    gw = Guarded((n, k), value=weight) if weight is not None else None
    loss, row_sum, sel = Guarded((1,)), Guarded((n, k)), Guarded((n, k), dtype=torch.uint8)
    ws_bytes = lib.mp_joints_ohkm_workspace_bytes(n, k)
    ws = Guarded((ws_bytes // 8,), dtype=torch.float64)
    assert ws.t.data_ptr() % 8 == 0
    _lib.check(lib.mp_joints_ohkm_fwd(gp.t.data_ptr(), gt.t.data_ptr(), gw.t.data_ptr() if gw else None, loss.t.data_ptr(),
                                      row_sum.t.data_ptr(), sel.t.data_ptr(), ws.t.data_ptr(), ws_bytes, n, k, h * w, topk,
                                      _lib.stream()), "mp_joints_ohkm_fwd")
    torch.cuda.synchronize()
    for g, what in ((gp, "pred"), (gt, "target")) + (((gw, "weight"),) if gw else ()):
        g.assert_unchanged(what)
    for g, what in ((loss, "loss"), (row_sum, "row_sum"), (sel, "sel"), (ws, "workspace")):
        g.assert_guards(what)
    return dict(loss=loss.t.cpu().numpy()[0], row_sum=row_sum.t.cpu().numpy(), sel=sel.t.cpu().numpy(), gp=gp, gt=gt, gw=gw, gsel=sel,
                topk=topk)


def _raw_bwd(f, g=None):
    """mp_joints_ohkm_bwd on the buffers of ``_raw_fwd``: the gradient as numpy; ``g``: the upstream scalar (None = NULL = 1)."""
    lib = _lib.load()
    n, k, h, w = f["gp"].t.shape
    grad = Guarded((n, k, h, w), shift=f["gp"].lo - GUARD)
    go = torch.full((1,), g, device=DEV) if g is not None else None
    before = [(x, x.buf.clone()) for x in (f["gp"], f["gt"], f["gsel"])]
    _lib.check(lib.mp_joints_ohkm_bwd(f["gp"].t.data_ptr(), f["gt"].t.data_ptr(), f["gw"].t.data_ptr() if f["gw"] else None,
                                      f["gsel"].t.data_ptr(), go.data_ptr() if go is not None else None, grad.t.data_ptr(), n, k, h * w,
                                      f["topk"], _lib.stream()), "mp_joints_ohkm_bwd")
    torch.cuda.synchronize()
    grad.assert_guards("grad_pred")
    for x, was in before:
        assert torch.equal(x._bits(x.buf), x._bits(was)), "the backward wrote to an input"
    return grad.t.cpu().numpy()


def _assert_grad(got, want, sel, what=""):
    """Selected rows: rtol 1e-6 / atol 1e-12 against float64.  Other rows: zero BITS."""
    on = sel.astype(bool)
    assert (got[~on].view(np.int32) == 0).all(), f"{what}: a row that is not selected is not exact zeros"
    np.testing.assert_allclose(got[on], want[on], rtol=1e-6, atol=1e-12, err_msg=what)


# ---- the kernels against the restatement ----------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 3, 4, 1), (3, 17, 3, 4, 8), (3, 17, 3, 5, 8), (2, 17, 16, 12, 17), (2, 17, 16, 12, 1), (2, 65, 3, 4, 8), (1, 133, 3, 4, 8),
          (1, 1024, 2, 2, 1000), (300, 5, 3, 4, 2)]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("shape", SHAPES + [(3, 17, 3, 4, 8, 1), (2, 17, 16, 12, 5, 3)], ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_restatement(shape, weighted):
    """The shapes of DESIGN.md 4.17, and two of them again 1 and 3 floats off 16-byte alignment (HW % 4 == 0 on the 4-byte path)."""
    n, k, h, w, topk = shape[:5]
    shift = shape[5] if len(shape) > 5 else 0
    pred, target, weight = _inputs(n, k, h, w, seed=11 + n + k, weighted=weighted)
    want_loss, s64, want_sel, want_grad = R.ohkm(pred, target, weight, topk, g=1.5)
    _assert_separated(s64)
    if weighted:
        assert (weight == 0).any() == (k > 1) and (weight > 1).any()
    f = _raw_fwd(pred, target, weight, topk, shift=shift)
    scale = np.abs(s64)
    print(f"shape {shape} weighted {weighted}: row_sum worst rel err {np.max(np.abs(f['row_sum'] - s64) / np.maximum(scale, 1e-300)):.3g}, "
          f"loss {f['loss']!r} want {want_loss!r}")
    assert (np.abs(f["row_sum"] - s64) <= 1e-6 * scale).all()
    assert np.array_equal(f["sel"], want_sel)
    own = R.select(f["row_sum"], topk) if k <= 160 else R.select_fast(f["row_sum"], topk)
    assert np.array_equal(f["sel"], own), "the selection does not follow the rule on the kernel's own row sums"
    assert (f["sel"].sum(axis=1) == topk).all()
    assert abs(float(f["loss"]) - want_loss) <= 1e-6 * abs(want_loss)
    grad = _raw_bwd(f, g=1.5)
    _assert_grad(grad, want_grad, want_sel, str(shape))
    # NULL grad_out is 1
    if shape == SHAPES[1]:
        _assert_grad(_raw_bwd(f), R.grad(pred, target, weight, want_sel, topk), want_sel, "grad_out NULL")
    # a second run: the same bits
    f2 = _raw_fwd(pred, target, weight, topk, shift=shift)
    assert np.array_equal(f2["row_sum"].view(np.int32), f["row_sum"].view(np.int32)) and np.array_equal(f2["sel"], f["sel"])
    assert np.float32(f2["loss"]).view(np.int32) == np.float32(f["loss"]).view(np.int32)
    assert np.array_equal(_raw_bwd(f2, g=1.5).view(np.int32), grad.view(np.int32))


def test_python_api_matches_the_c_abi():
    """``joints_ohkm_mse`` and the autograd path of ``JointsOHKMMSELoss`` give the C ABI's bits ([N, K, 1] weights as the data
    pipeline hands them)."""
    n, k, h, w, topk = 3, 17, 16, 12, 8
    pred, target, weight = _inputs(n, k, h, w, seed=5, weighted=True)
    f = _raw_fwd(pred, target, weight, topk)
    grad = _raw_bwd(f, g=1.5)
    tp, tt, tw = torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), torch.from_numpy(weight).to(DEV).reshape(n, k, 1)
    loss, row_sum, sel = mp.joints_ohkm_mse(tp, tt, tw, topk)
    assert loss.shape == () and row_sum.shape == (n, k) and sel.shape == (n, k) and sel.dtype == torch.uint8
    assert np.array_equal(row_sum.cpu().numpy().view(np.int32), f["row_sum"].view(np.int32)) and np.array_equal(sel.cpu().numpy(), f["sel"])
    assert float(loss) == float(f["loss"])
    tp.requires_grad_(True)
    out = mp.create_loss("joint_ohkm_mse", use_target_weight=True, topk=topk)(tp, tt, tw)
    assert float(out.detach()) == float(f["loss"])
    (out * 1.5).backward()
    assert np.array_equal(tp.grad.cpu().numpy().view(np.int32), grad.view(np.int32))
    # without the flag the weight is ignored
    plain = mp.create_loss("joint_ohkm_mse", topk=topk)(tp.detach(), tt, tw)
    assert float(plain) == float(_raw_fwd(pred, target, None, topk)["loss"])


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [1, 2])
def test_ties_go_to_the_lower_index(fit):
    """Rows 2, 9 and 14 of samples 0 and 1 are bit-identical (maps and weight) and ``topk`` lets only ``fit`` of them in; sample 1
    is sample 0 with joints 0 and 1 exchanged, so the tied value has one rank in both.  Sample 2 has all-zero weights: every sum
    is 0 and the first topk joints are selected."""
    n, k, h, w = 3, 17, 3, 4
    pred, target, _ = _inputs(n, k, h, w, seed=7, weighted=False)
    weight = np.full((n, k), 1.5, dtype=np.float32)
    weight[2] = 0.0
    for j in (9, 14):
        pred[0, j], target[0, j] = pred[0, 2], target[0, 2]
    order = [1, 0] + list(range(2, k))
    pred[1], target[1] = pred[0, order], target[0, order]
    s64 = R.row_sums(pred, target, weight)
    _assert_separated(np.delete(s64[:2], [9, 14], axis=1))  # apart from the planted ties the sums are a ladder
    above = int((s64[0] > s64[0, 2]).sum())
    assert above == int((s64[1] > s64[1, 2]).sum()) and 0 < above and above + 3 < k
    topk = above + fit
    f = _raw_fwd(pred, target, weight, topk)
    bits = f["row_sum"].view(np.int32)
    assert (bits[:2, 9] == bits[:2, 2]).all() and (bits[:2, 14] == bits[:2, 2]).all(), "a row sum depends on where the row lies"
    assert np.array_equal(f["sel"], R.select(s64, topk)) and np.array_equal(f["sel"], R.select(f["row_sum"], topk))
    assert f["sel"][:2, [2, 9, 14]].tolist() == [[1, 0, 0] if fit == 1 else [1, 1, 0]] * 2
    assert (f["row_sum"][2] == 0).all() and f["sel"][2].tolist() == [1] * topk + [0] * (k - topk)
    _assert_grad(_raw_bwd(f, g=1.0), R.grad(pred, target, weight, f["sel"], topk), f["sel"])


# ---- non-finite rows and the rows the backward must not read ------------------------------------------------------------------------------------
def test_nonfinite_rows_are_selected_and_unselected_rows_are_not_read():
    n, k, h, w, topk = 3, 17, 3, 4, 8
    pred, target, _ = _inputs(n, k, h, w, seed=9, weighted=False)
    pred[0, 5] = np.nan
    pred[1, 11] = np.inf
    want_loss, s64, want_sel, want_grad = R.ohkm(pred, target, None, topk)
    f = _raw_fwd(pred, target, None, topk)
    assert np.isnan(f["row_sum"][0, 5]) and f["row_sum"][1, 11] == np.inf
    assert np.array_equal(f["sel"], want_sel) and f["sel"][0, 5] == 1 and f["sel"][1, 11] == 1
    assert (f["sel"].sum(axis=1) == topk).all()
    assert not np.isfinite(f["loss"]) and not np.isfinite(want_loss)
    # the guard: what the rows that were not selected hold after the forward must not matter (and is not read)
    off = torch.from_numpy(want_sel == 0).to(DEV)
    f["gp"].t[off] = float("nan")
    f["gt"].t[off] = float("nan")
    grad = _raw_bwd(f)
    assert not np.isfinite(grad[0, 5]).any() and not np.isfinite(grad[1, 11]).any()
    finite = want_sel.astype(bool).copy()
    finite[0, 5] = finite[1, 11] = False
    assert (grad[want_sel == 0].view(np.int32) == 0).all(), "a row that is not selected was read (or not zero-filled)"
    np.testing.assert_allclose(grad[finite], want_grad[finite], rtol=1e-6, atol=1e-12)
    # through the loss class: the same selection reaches autograd
    tp = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    out = mp.JointsOHKMMSELoss(topk=topk)(tp, torch.from_numpy(target).to(DEV))
    out.backward()
    assert not torch.isfinite(out) and not torch.isfinite(tp.grad[0, 5]).any() and not torch.isfinite(tp.grad[1, 11]).any()
    assert torch.isfinite(tp.grad[2]).all()


# ---- known answers ------------------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    n, k, h, w = 128, 17, 64, 48
    pred, target = torch.ones(n, k, h, w, device=DEV), torch.zeros(n, k, h, w, device=DEV)
    weight = torch.full((n, k, 1), 0.5, device=DEV)
    for topk in range(1, k + 1):
        assert float(mp.create_loss("joint_ohkm_mse", use_target_weight=True, topk=topk)(pred, target, weight)) == 0.5, topk
    _, row_sum, sel = mp.joints_ohkm_mse(pred, target, weight, 8)
    assert (row_sum == 0.5 * h * w).all() and sel.cpu().numpy().tolist() == [[1] * 8 + [0] * 9] * n  # all equal: the first eight
    g = torch.Generator().manual_seed(1)
    pred = torch.randn(n, k, h, w, generator=g).to(DEV).requires_grad_(True)
    target = torch.rand(n, k, h, w, generator=g).to(DEV)
    weight = torch.rand(n, k, 1, generator=g).to(DEV)
    full = mp.create_loss("joint_ohkm_mse", use_target_weight=True, topk=k)(pred, target, weight)
    full.backward()
    grad, pred.grad = pred.grad, None
    mse = mp.create_loss("joint_mse", use_target_weight=True)(pred, target, weight)
    mse.backward()
    assert abs(float(full.detach()) - float(mse.detach())) <= 1e-6 * float(mse.detach())
    torch.testing.assert_close(grad, pred.grad, rtol=1e-6, atol=1e-12)
    losses = [float(mp.joints_ohkm_mse(pred, target, weight, topk)[0]) for topk in (1, 4, 8, 12, 16, 17)]
    assert all(a >= b for a, b in zip(losses, losses[1:])) and losses[0] > losses[-1], losses


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = _lib.load()
    n, k, h, w, topk = 2, 17, 3, 4, 8
    pred, target, weight = _inputs(n, k, h, w, seed=3, weighted=True)
    gp, gt, gw = Guarded(pred.shape, value=pred), Guarded(pred.shape, value=target), Guarded((n, k), value=weight)
    loss, row_sum, sel, grad = Guarded((1,)), Guarded((n, k)), Guarded((n, k), dtype=torch.uint8), Guarded(pred.shape)
    ws_bytes = lib.mp_joints_ohkm_workspace_bytes(n, k)
    ws = Guarded((ws_bytes // 8,), dtype=torch.float64)

    def fwd(**kw):
        a = dict(pred=gp.t.data_ptr(), target=gt.t.data_ptr(), weight=gw.t.data_ptr(), loss=loss.t.data_ptr(), row_sum=row_sum.t.data_ptr(),
                 sel=sel.t.data_ptr(), work=ws.t.data_ptr(), work_bytes=ws_bytes, n=n, k=k, hw=h * w, topk=topk)
        a.update(kw)
        return lib.mp_joints_ohkm_fwd(*a.values(), _lib.stream())

    def bwd(**kw):
        a = dict(pred=gp.t.data_ptr(), target=gt.t.data_ptr(), weight=gw.t.data_ptr(), sel=sel.t.data_ptr(), grad_out=None,
                 grad=grad.t.data_ptr(), n=n, k=k, hw=h * w, topk=topk)
        a.update(kw)
        return lib.mp_joints_ohkm_bwd(*a.values(), _lib.stream())

    for name in ("pred", "target", "loss", "row_sum", "sel"):
        assert fwd(**{name: None}) == -1, name                                                  # MP_ERR_NULL
    for name in ("pred", "target", "sel", "grad"):
        assert bwd(**{name: None}) == -1, name
    for call in (fwd, bwd):
        for kw in (dict(n=0), dict(k=0), dict(hw=0), dict(hw=-4), dict(topk=0), dict(topk=k + 1), dict(k=1025)):
            assert call(**kw) == -2, (call.__name__, kw)                                       # MP_ERR_SHAPE
    assert fwd(work=None) == -5 and fwd(work_bytes=ws_bytes - 1) == -5 and fwd(work_bytes=0) == -5  # MP_ERR_WORKSPACE
    torch.cuda.synchronize()
    for g_, what in ((loss, "loss"), (row_sum, "row_sum"), (sel, "sel"), (grad, "grad"), (ws, "workspace"), (gp, "pred"), (gt, "target")):
        g_.assert_unchanged(what)
    assert fwd() == 0 and bwd() == 0  # the same buffers are accepted as they are
    torch.cuda.synchronize()


# ---- inside the training step -------------------------------------------------------------------------------------------------------------------
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


def _run_steps(batches, graphed, metric=None):
    """The pattern of tests/test_gpu_pose_metric.py::_run_steps with ``joint_ohkm_mse(topk=8)``: HRNet-W32, amp O2, the graphed step
    with the resident tail - or the same three steps eagerly (forward, scaled backward, ``optimizer.step`` with the manager).
    Before every step the network runs once more on the step's batch: ``floor`` is the joint_mse of the step's own heat maps."""
    torch.manual_seed(0)
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(DEV).train()
    mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.NetWithLoss(net, mp.create_loss("joint_ohkm_mse", use_target_weight=True, topk=8), has_extra_inputs=True, metric=metric)
    mse = mp.create_loss("joint_mse", use_target_weight=True)
    opt = AdamWeightDecay(net, lr=1e-3, weight_decay=0.05, filter_bias_and_bn=True, overlap=False)
    mgr = DynamicLossScaleManager(2.0 ** 12, 2.0, 2)
    step = GraphedTrainStep(nwl, opt, batches[0], loss_scale_manager=mgr, resident=True, total_steps=len(batches)) if graphed else None
    losses, floor = [], []
    for x, target, weight in batches:
        heat = nwl.net(x).detach().clone()
        floor.append(float(mse(heat, target, weight)))
        if graphed:
            losses.append(step(x, target, weight).detach().clone())
        else:
            opt.zero_grad()
            loss = nwl(x, target, weight)
            mgr.scale(loss).backward()
            opt.step(loss_scale_manager=mgr)
            losses.append(loss.detach().clone())
    if graphed:
        step.sync()
    torch.cuda.synchronize()
    out = dict(flat=opt.flat.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), losses=torch.stack(losses), floor=floor,
               mgr=(mgr.loss_scale, mgr.cur_iter, mgr.last_overflow_iter, mgr.skipped_steps), global_step=opt.global_step,
               epoch=metric.compute() if metric is not None else None)
    opt.close()
    return out


def test_ohkm_inside_the_graphed_step(monkeypatch):
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")
    batches = _batches()
    graphed = _run_steps(batches, graphed=True)
    eager = _run_steps(batches, graphed=False)
    with_metric = _run_steps(batches, graphed=True, metric=mp.PoseAccuracy())
    print("losses", graphed["losses"].tolist(), "joint_mse of the same maps", graphed["floor"], "loss scale state", graphed["mgr"])
    for other, what in ((eager, "eager"), (with_metric, "with PoseAccuracy")):
        for key in ("losses", "flat", "m", "v"):
            assert _same_bits(graphed[key], other[key]), (what, key)
        assert other["mgr"] == graphed["mgr"] and other["global_step"] == graphed["global_step"], what
        assert other["floor"] == graphed["floor"], what
    assert torch.isfinite(graphed["losses"]).all() and graphed["global_step"] > 0
    for loss, floor in zip(graphed["losses"].tolist(), graphed["floor"]):
        assert loss >= floor > 0, (loss, floor)  # the mean of the eight largest of seventeen row sums is no less than the mean of all
    assert with_metric["epoch"]["steps"] == len(batches)


# ---- the recipe runner with the two options -----------------------------------------------------------------------------------------------------
def test_runner_trains_with_ohkm(tmp_path, monkeypatch):
    import mindpose_amd.cli.train as cli_train
    from mindpose_amd.cli.config import parse_args
    from tests.test_gpu_trainer import _argv, _coco_folder
    made = []
    real = cli_train.create_loss
    monkeypatch.setattr(cli_train, "create_loss", lambda name, **kw: made.append(real(name, **kw)) or made[-1])
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")
    tmp = str(tmp_path)
    data = dict(train_root=os.path.join(tmp, "train"), val_root=os.path.join(tmp, "train"))
    data["train_label"] = data["val_label"] = _coco_folder(data["train_root"], 9, 5, "train.json")
    outdir = os.path.join(tmp, "out")
    cli_train.train(parse_args(_argv(data, outdir) + ["loss=joint_ohkm_mse", "loss_setting.topk=8", "val_while_train=False"]))
    assert len(made) == 1 and isinstance(made[0], mp.JointsOHKMMSELoss) and made[0].topk == 8 and made[0].use_target_weight
    with open(os.path.join(outdir, "summary", "summary.jsonl")) as f:
        recs = [json.loads(line) for line in f]
    assert [r["epoch"] for r in recs] == [1, 2] and [r["step"] for r in recs] == [2, 4]
    assert all(np.isfinite(r["train/loss"]) and r["train/loss"] > 0 for r in recs), recs
