"""JointsMSELoss and JointsMSELossWithMask on the MI355X HIP path (reference: mindpose/models/loss/mse.py:11-72).

L = mean_{n,k,h,w}( w[n,k] * (pred - target)^2 ): one pass over pred/target (16 B per lane), a
deterministic two-stage reduction, and an analytic backward kernel wired through autograd.

The masked form, L = sum((pred - target)^2 * mask[n,h,w]) / (N K H W), takes its operands as VIEWS (the heat-map channels of
a stage output, a corner of the padded target and of the mask) and reads them in place through their strides.
"""
from typing import Optional

import torch

from ... import _lib
from ...register import register
from .loss import Loss


class _JointsMSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight):
        lib = _lib.load()
        n, k, h, w = pred.shape
        ws_bytes = lib.mp_joints_mse_workspace_bytes(n, k)
        ws = torch.empty(ws_bytes // 4, device=pred.device, dtype=torch.float32)
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        _lib.check(lib.mp_joints_mse_fwd(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(loss),
                                         _lib.ptr(ws), ws_bytes, n, k, h * w, _lib.stream()), "mp_joints_mse_fwd")
        ctx.save_for_backward(pred, target, weight if weight is not None else torch.empty(0, device=pred.device))
        ctx.has_weight = weight is not None
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        pred, target, weight = ctx.saved_tensors
        n, k, h, w = pred.shape
        grad = torch.empty_like(pred)
        go = grad_out.detach().float().reshape(1).contiguous()
        _lib.check(lib.mp_joints_mse_bwd(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(weight) if ctx.has_weight else None,
                                         _lib.ptr(go), _lib.ptr(grad), n, k, h * w, _lib.stream()), "mp_joints_mse_bwd")
        return grad, None, None


@register("loss", extra_name="joint_mse")
class JointsMSELoss(Loss):
    def __init__(self, use_target_weight: bool = False, reduction: Optional[str] = "mean") -> None:
        super().__init__(reduction=reduction)
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' (the reference recipes' setting) runs on the HIP path")
        self.use_target_weight = use_target_weight

    def forward(self, pred: torch.Tensor, target: torch.Tensor, target_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        pred = _lib.require_cuda_f32(pred, "pred")
        target = _lib.require_cuda_f32(target, "target")
        if pred.shape != target.shape or pred.dim() != 4:
            raise ValueError("pred and target must both be [N,K,H,W]")
        weight = None
        if self.use_target_weight:
            if target_weight is None:
                raise ValueError("target_weight is required when use_target_weight=True")
            weight = _lib.require_cuda_f32(target_weight, "target_weight").reshape(pred.shape[0], pred.shape[1])
        return _JointsMSEFn.apply(pred, target, weight)


def _view4(t: torch.Tensor, name: str) -> torch.Tensor:
    """A [N,K,H,W] fp32 CUDA view the strided kernels can read in place: unit column stride (anything else is copied)."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.MindposeHipError(f"{name} must be a CUDA tensor: the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        t = t.float()
    if t.stride(-1) != 1 or any(s < 0 for s in t.stride()):
        t = t.contiguous()
    return t


def _mask_view(mask: torch.Tensor, shape) -> torch.Tensor:
    """The [N,H,W] mask as the kernels read it: fp32, or one byte per pixel (uint8 / bool), unit column stride."""
    if not torch.is_tensor(mask):
        raise TypeError("mask must be a torch.Tensor")
    if not mask.is_cuda:
        raise _lib.MindposeHipError("mask must be a CUDA tensor: the HIP path has no CPU fallback")
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"mask must be [N,H,W] = {tuple(shape)}, got {tuple(mask.shape)}")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    elif mask.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"mask must be float32, uint8 or bool, got {mask.dtype}")
    if mask.stride(-1) != 1:
        mask = mask.contiguous()
    return mask


def launch_mse_mask_fwd(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """``mp_joints_mse_mask_fwd`` on prepared views (``_view4`` / ``_mask_view``); returns the [1] loss."""
    lib = _lib.load()
    n, k, h, w = pred.shape
    ws_bytes = lib.mp_joints_mse_mask_workspace_bytes(n, k)
    ws = torch.empty(ws_bytes // 4, device=pred.device, dtype=torch.float32)
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    _lib.check(lib.mp_joints_mse_mask_fwd(pred.data_ptr(), *pred.stride()[:3], target.data_ptr(), *target.stride()[:3],
                                          mask.data_ptr(), int(mask.dtype == torch.uint8), *mask.stride()[:2], _lib.ptr(loss),
                                          _lib.ptr(ws), ws_bytes, n, k, h, w, _lib.stream()), "mp_joints_mse_mask_fwd")
    return loss


def launch_mse_mask_bwd(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, grad_out: torch.Tensor, grad: torch.Tensor) -> None:
    """``mp_joints_mse_mask_bwd``: writes ``grad`` (a [N,K,H,W] view, e.g. the heat-map channels of a stage gradient) in place;
    ``grad_out`` is the [1] upstream gradient on the device."""
    lib = _lib.load()
    n, k, h, w = pred.shape
    _lib.check(lib.mp_joints_mse_mask_bwd(pred.data_ptr(), *pred.stride()[:3], target.data_ptr(), *target.stride()[:3],
                                          mask.data_ptr(), int(mask.dtype == torch.uint8), *mask.stride()[:2], _lib.ptr(grad_out),
                                          grad.data_ptr(), *grad.stride()[:3], n, k, h, w, _lib.stream()), "mp_joints_mse_mask_bwd")


class _JointsMSEMaskFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask):
        ctx.save_for_backward(pred, target, mask)
        return launch_mse_mask_fwd(pred, target, mask).reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        pred, target, mask = ctx.saved_tensors
        grad = torch.empty(pred.shape, device=pred.device, dtype=torch.float32)
        launch_mse_mask_bwd(pred, target, mask, grad_out.detach().float().reshape(1).contiguous(), grad)
        return grad, None, None


@register("loss", extra_name="joint_mse_with_mask")
class JointsMSELossWithMask(Loss):
    """Joint MSE with a pixel mask (mse.py:47-72): masked-out positions do not contribute, but count in the mean."""

    def __init__(self, reduction: Optional[str] = "mean") -> None:
        super().__init__(reduction=reduction)
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' (the reference recipes' setting) runs on the HIP path")

    def forward(self, pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        pred, target = _view4(pred, "pred"), _view4(target, "target")
        if pred.dim() != 4 or pred.shape != target.shape:
            raise ValueError("pred and target must both be [N,K,H,W]")
        mask = _mask_view(mask, (pred.shape[0], pred.shape[2], pred.shape[3]))
        return _JointsMSEMaskFn.apply(pred, target, mask)
