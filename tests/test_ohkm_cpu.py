"""CPU-side checks of the OHKM joint MSE (``joint_ohkm_mse``): registry name, exports, constructor, argument errors, the C-ABI
declarations and their refusals, the recipe switch, and the invariants of the float64 restatement (tests/ohkm_restated.py) that the
GPU tests compare the kernels with."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mindpose_amd as mp
from mindpose_amd import _lib
from oracle import loss as oloss
from tests import ohkm_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mp_joints_ohkm_workspace_bytes", "mp_joints_ohkm_fwd", "mp_joints_ohkm_bwd")


# ---- the drop-in boundary ----------------------------------------------------------------------------------------------------------------------
def test_registry_exports_and_defaults():
    for name in ("JointsOHKMMSELoss", "joint_ohkm_mse"):
        assert mp.entrypoint("loss", name) is mp.JointsOHKMMSELoss
    assert mp.models.JointsOHKMMSELoss is mp.JointsOHKMMSELoss is mp.models.loss.JointsOHKMMSELoss
    assert mp.models.joints_ohkm_mse is mp.joints_ohkm_mse is mp.models.loss.joints_ohkm_mse
    params = [(k, v.default) for k, v in list(inspect.signature(mp.JointsOHKMMSELoss.__init__).parameters.items())[1:]]
    assert params == [("use_target_weight", False), ("topk", 8)]
    assert list(inspect.signature(mp.JointsOHKMMSELoss.forward).parameters)[1:] == ["pred", "target", "target_weight"]
    assert list(inspect.signature(mp.joints_ohkm_mse).parameters) == ["pred", "target", "weight", "topk"]
    loss = mp.create_loss("joint_ohkm_mse", use_target_weight=True, topk=5)
    assert isinstance(loss, mp.JointsOHKMMSELoss) and isinstance(loss, mp.models.loss.Loss)
    assert loss.topk == 5 and loss.use_target_weight is True and mp.create_loss("joint_ohkm_mse").topk == 8


def test_argument_errors():
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="topk"):
            mp.JointsOHKMMSELoss(topk=bad)
    z = torch.zeros(2, 4, 3, 2)
    with pytest.raises(ValueError, match="topk"):
        mp.JointsOHKMMSELoss(topk=5)(z, z)                      # topk > K
    with pytest.raises(ValueError, match=r"\[N,K,H,W\]"):
        mp.JointsOHKMMSELoss(topk=2)(z, torch.zeros(2, 4, 3, 3))  # mismatched shapes
    with pytest.raises(ValueError, match=r"\[N,K,H,W\]"):
        mp.JointsOHKMMSELoss(topk=2)(z[0], z[0])
    with pytest.raises(ValueError, match="target_weight"):
        mp.JointsOHKMMSELoss(use_target_weight=True, topk=2)(z, z)  # missing weight
    with pytest.raises(ValueError, match="target_weight"):
        mp.JointsOHKMMSELoss(use_target_weight=True, topk=2)(z, z, torch.ones(2, 3))
    with pytest.raises(ValueError, match="topk"):
        mp.joints_ohkm_mse(z, z, None, 0)
    with pytest.raises(ValueError, match="topk"):
        mp.joints_ohkm_mse(z, z, None, 5)
    # valid arguments on CPU tensors: the HIP path has no CPU fallback
    with pytest.raises(_lib.MindposeHipError):
        mp.JointsOHKMMSELoss(topk=2)(z, z)
    with pytest.raises(_lib.MindposeHipError):
        mp.JointsOHKMMSELoss(use_target_weight=True, topk=2)(z, z, torch.ones(2, 4, 1))
    with pytest.raises(_lib.MindposeHipError):
        mp.joints_ohkm_mse(z, z, None, 4)


def test_symbols_declared_listed_and_refusing():
    header = open(os.path.join(ROOT, "include", "mindpose_hip.h")).read()
    declared = set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
    assert "unsigned char* sel_dev" in header  # the element type of sel is part of the ABI
    lib = _lib.load()
    assert lib.mp_joints_ohkm_workspace_bytes(128, 17) >= 128 * 8 and lib.mp_joints_ohkm_workspace_bytes(128, 17) % 256 == 0
    assert lib.mp_joints_ohkm_workspace_bytes(0, 17) == 0 and lib.mp_joints_ohkm_workspace_bytes(4, 0) == 0
    # the refusals come before any HIP call, so they are testable without a GPU (the pointers are never followed)
    p = 4096
    ws = lib.mp_joints_ohkm_workspace_bytes(2, 17)

    def fwd(pred=p, target=p, weight=None, loss=p, row_sum=p, sel=p, work=p, work_bytes=ws, n=2, k=17, hw=12, topk=8):
        return lib.mp_joints_ohkm_fwd(pred, target, weight, loss, row_sum, sel, work, work_bytes, n, k, hw, topk, None)

    def bwd(pred=p, target=p, weight=None, sel=p, grad_out=None, grad=p, n=2, k=17, hw=12, topk=8):
        return lib.mp_joints_ohkm_bwd(pred, target, weight, sel, grad_out, grad, n, k, hw, topk, None)

    for name in ("pred", "target", "loss", "row_sum", "sel"):
        assert fwd(**{name: None}) == -1, name
    for name in ("pred", "target", "sel", "grad"):
        assert bwd(**{name: None}) == -1, name
    for call in (fwd, bwd):
        for kw in (dict(n=0), dict(k=0), dict(hw=0), dict(n=-1), dict(topk=0), dict(topk=18), dict(k=1025, topk=8),
                   dict(n=1 << 22, k=1024)):
            assert call(**kw) == -2, (call.__name__, kw)
    assert fwd(work=None) == -5 and fwd(work_bytes=ws - 1) == -5 and fwd(work_bytes=0) == -5 and fwd(work=p + 4) == -5


def test_recipe_switch_parses():
    """The two --cfg-options of INTEGRATION.md: the recipe's use_target_weight and loss_with_extra_input carry over."""
    from mindpose_amd.cli.config import parse_args
    recipe = os.path.join(ROOT, "tests", "golden", "recipes", "hrnet_w32_ascend.yaml")
    args = parse_args(["--config", recipe, "--cfg-options", "loss=joint_ohkm_mse", "loss_setting.topk=8"])
    assert args.loss == "joint_ohkm_mse" and args.loss_setting == dict(use_target_weight=True, topk=8) and args.loss_with_extra_input
    loss = mp.create_loss(args.loss, **args.loss_setting)
    assert isinstance(loss, mp.JointsOHKMMSELoss) and loss.topk == 8 and loss.use_target_weight


# ---- the restatement's own invariants --------------------------------------------------------------------------------------------------------
def _case(n, k, h, w, seed, weighted=True):
    rng = np.random.RandomState(seed)
    target = rng.rand(n, k, h, w).astype(np.float32)
    amp = (0.05 + 0.9 * rng.permutation(k) / k).astype(np.float32)
    pred = target + amp[None, :, None, None] * rng.randn(n, k, h, w).astype(np.float32)
    weight = rng.choice([0.0, 0.5, 1.0, 2.5], size=(n, k)).astype(np.float32) if weighted else None
    return pred, target, weight


@pytest.mark.parametrize("weighted", [False, True])
def test_topk_equal_k_is_joint_mse(weighted):
    pred, target, weight = _case(3, 17, 6, 5, 0, weighted)
    loss, s, sel, grad = R.ohkm(pred, target, weight, 17)
    assert sel.all()
    ref = float(oloss.joints_mse(pred, target, weight, use_target_weight=weighted))
    assert abs(loss - ref) <= 1e-6 * abs(ref)
    ref_grad = oloss.joints_mse_grad(pred, target, weight, use_target_weight=weighted)
    np.testing.assert_allclose(grad, ref_grad, rtol=1e-5, atol=1e-12)  # the oracle's gradient is formed in fp32


def test_loss_is_monotone_in_topk_and_picks_the_largest():
    pred, target, weight = _case(4, 17, 6, 5, 1)
    losses = []
    for topk in range(1, 18):
        loss, s, sel, _ = R.ohkm(pred, target, weight, topk)
        losses.append(loss)
        assert (sel.sum(axis=1) == topk).all()
        for a in range(s.shape[0]):
            assert s[a][sel[a] == 1].min() >= s[a][sel[a] == 0].max() if topk < 17 else True
    assert all(a >= b for a, b in zip(losses, losses[1:])), losses
    assert losses[0] > losses[-1]


def test_tie_and_nan_order():
    nan, inf = float("nan"), float("inf")
    s = np.array([[1.0, 3.0, 3.0, 0.5, 3.0, 2.0],       # equal values: the lower index
                  [0.0, -0.0, 0.0, -0.0, 0.0, 0.0],      # -0.0 == +0.0: the index alone
                  [1.0, nan, inf, nan, 5.0, -inf],       # NaN before +inf, NaNs by index
                  [nan, nan, nan, nan, nan, nan]], dtype=np.float32)
    expect = {1: [[0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]],
              2: [[0, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0, 1, 0, 1, 0, 0], [1, 1, 0, 0, 0, 0]],
              3: [[0, 1, 1, 0, 1, 0], [1, 1, 1, 0, 0, 0], [0, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0]],
              4: [[0, 1, 1, 0, 1, 1], [1, 1, 1, 1, 0, 0], [0, 1, 1, 1, 1, 0], [1, 1, 1, 1, 0, 0]],
              6: [[1] * 6] * 4}
    for topk, want in expect.items():
        assert R.select(s, topk).tolist() == want, topk
        assert R.select_fast(s, topk).tolist() == want, topk
    assert R.before(nan, 3, inf, 0) and not R.before(inf, 0, nan, 3) and R.before(nan, 1, nan, 3) and not R.before(nan, 3, nan, 1)
    assert R.before(0.0, 0, -0.0, 1) and not R.before(-0.0, 1, 0.0, 0) and R.before(2.0, 5, 1.0, 0)
    # the order is total: every pair is ordered one way, and the ranks are a permutation
    for row in s:
        ranks = sorted(sum(R.before(row[j], j, row[i], i) for j in range(6) if j != i) for i in range(6))
        assert ranks == list(range(6))
    # the sort form agrees with the rank form on random rows with planted ties and NaNs
    rng = np.random.RandomState(2)
    r = rng.rand(5, 40).astype(np.float32)
    r[:, 7] = r[:, 21] = r[:, 30]
    r[1, 3] = r[1, 33] = nan
    for topk in (1, 2, 3, 20, 39, 40):
        assert np.array_equal(R.select(r, topk), R.select_fast(r, topk)), topk


def test_nonfinite_rows_reach_loss_and_gradient():
    pred, target, weight = _case(2, 6, 3, 4, 3)
    pred[0, 4, 1, 1] = float("nan")
    pred[1, 2] = float("inf")
    loss, s, sel, grad = R.ohkm(pred, target, None, 2)
    assert sel[0, 4] == 1 and sel[1, 2] == 1 and not np.isfinite(loss)
    assert np.isnan(grad[0, 4, 1, 1]) and np.isinf(grad[1, 2]).all()
    off = sel == 0
    assert (grad[off] == 0).all() and np.isfinite(grad[(sel == 1) & np.isfinite(s)]).all()
