"""JointsOHKMMSELoss: the joint MSE with online hard keypoint mining (OHKM) on the MI355X HIP path (the reference has no counterpart;
CPN and the HRNet training code train with it).

Per sample only the ``topk`` joints with the largest error contribute:

    S[n,k] = sum_hw( w[n,k] * (pred - target)^2 )          the row sums of JointsMSELoss
    L      = sum_n sum_{k in top-k of S[n,:]} S[n,k] / (N * topk * H * W)

The order behind "top-k" is total: a NaN sum first, then the larger sum, then the lower joint index (so a non-finite row is always
selected and reaches the loss, its gradient and the loss-scale overflow check).  ``topk = K`` is ``JointsMSELoss``.

Against the HRNet training code (``JointsOHKMMSELoss`` of lib/core/loss.py): that loss carries a factor 0.5 and multiplies pred and
target by the weight BEFORE squaring, this one has no 0.5 and multiplies the squared error by the weight, as ``JointsMSELoss`` here
and in the reference does.  With 0 / 1 weights (COCO visibility) this loss is exactly twice the HRNet code's.

The selection is made on the device (``mp_joints_ohkm_fwd``, csrc/joints_loss.hip: three launches, no read-back), the backward is one
launch that zero-fills the rows that were not selected without reading them; both capture into the training step's graph.
"""
from typing import Optional, Tuple

import torch

from ... import _lib
from ...register import register
from .loss import Loss

__all__ = ["JointsOHKMMSELoss", "joints_ohkm_mse"]


def launch_ohkm_fwd(pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor],
                    topk: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``mp_joints_ohkm_fwd`` on contiguous fp32 CUDA tensors: ``(loss [1], row_sum [N, K] fp32, sel [N, K] uint8)``."""
    lib = _lib.load()
    n, k, h, w = pred.shape
    ws_bytes = lib.mp_joints_ohkm_workspace_bytes(n, k)
    ws = torch.empty(ws_bytes // 8, device=pred.device, dtype=torch.float64)
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    row_sum = torch.empty(n, k, device=pred.device, dtype=torch.float32)
    sel = torch.empty(n, k, device=pred.device, dtype=torch.uint8)
    _lib.check(lib.mp_joints_ohkm_fwd(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(loss), _lib.ptr(row_sum),
                                      _lib.ptr(sel), _lib.ptr(ws), ws_bytes, n, k, h * w, topk, _lib.stream()), "mp_joints_ohkm_fwd")
    return loss, row_sum, sel


class _JointsOHKMMSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, topk):
        loss, _, sel = launch_ohkm_fwd(pred, target, weight, topk)
        ctx.save_for_backward(pred, target, weight if weight is not None else torch.empty(0, device=pred.device), sel)
        ctx.has_weight = weight is not None
        ctx.topk = topk
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        pred, target, weight, sel = ctx.saved_tensors
        n, k, h, w = pred.shape
        grad = torch.empty_like(pred)
        go = grad_out.detach().float().reshape(1).contiguous()
        _lib.check(lib.mp_joints_ohkm_bwd(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(weight) if ctx.has_weight else None,
                                          _lib.ptr(sel), _lib.ptr(go), _lib.ptr(grad), n, k, h * w, ctx.topk, _lib.stream()),
                   "mp_joints_ohkm_bwd")
        return grad, None, None, None


def _prepare(pred, target, weight, topk: int, weight_required: bool):
    """Argument errors first (they need no device), then contiguous fp32 CUDA tensors and the [N, K] weight (or None)."""
    for name, t in (("pred", pred), ("target", target)):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a torch.Tensor")
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError("pred and target must both be [N,K,H,W]")
    n, k = pred.shape[:2]
    if topk > k:
        raise ValueError(f"topk = {topk} exceeds the {k} joints of the heat maps")
    if weight is None and weight_required:
        raise ValueError("target_weight is required when use_target_weight=True")
    if weight is not None and (not torch.is_tensor(weight) or weight.numel() != n * k):
        raise ValueError(f"target_weight must be a tensor of N * K = {n * k} values")
    pred, target = _lib.require_cuda_f32(pred, "pred"), _lib.require_cuda_f32(target, "target")
    if weight is not None:
        weight = _lib.require_cuda_f32(weight, "target_weight").reshape(n, k)
    return pred, target, weight


def _check_topk(topk) -> int:
    if isinstance(topk, bool) or int(topk) != topk or int(topk) < 1:
        raise ValueError(f"topk must be an integer >= 1, got {topk!r}")
    return int(topk)


@register("loss", extra_name="joint_ohkm_mse")
class JointsOHKMMSELoss(Loss):
    """Joint MSE over the ``topk`` hardest joints of every sample (see the module docstring for the exact definition and for the
    factor 2 and the weight convention against the HRNet training code)."""

    def __init__(self, use_target_weight: bool = False, topk: int = 8) -> None:
        super().__init__(reduction="mean")
        self.topk = _check_topk(topk)
        self.use_target_weight = use_target_weight

    def forward(self, pred: torch.Tensor, target: torch.Tensor, target_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        pred, target, weight = _prepare(pred, target, target_weight if self.use_target_weight else None, self.topk,
                                        weight_required=self.use_target_weight)
        return _JointsOHKMMSEFn.apply(pred, target, weight, self.topk)


def joints_ohkm_mse(pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor],
                    topk: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The forward alone, for inspection and tests: ``(loss 0-d fp32, row_sum [N, K] fp32, sel [N, K] uint8)`` on the device;
    ``weight`` None means 1.  No gradient is recorded."""
    pred, target, weight = _prepare(pred, target, weight, _check_topk(topk), weight_required=False)
    with torch.no_grad():
        loss, row_sum, sel = launch_ohkm_fwd(pred.detach(), target.detach(), weight, int(topk))
    return loss.reshape(()), row_sum, sel
