"""AELoss - the associative-embedding ("grouping") loss - on the MI355X HIP path (reference: mindpose/models/loss/ae.py:11-89).

The reference scatters ``tag_ind`` into an [N, M, K, H, W] mask and reduces masked tensors of that size; at most M*K of those
entries per image are non-zero.  ``mp_ae_loss_fwd`` gathers them (one workgroup per image), forms the per-person reference
embeddings and the push / pull terms in fp64 and returns ``[push, pull]``, each the mean over N; ``mp_ae_loss_bwd`` writes the
gradient of the tag planes - zero but for the indexed pixels - for the two upstream gradients.  Both are deterministic.
"""
from typing import Optional, Tuple

import torch

from ... import _lib
from ...register import register
from .loss import Loss


def _tag_views(pred: torch.Tensor, tag_ind: torch.Tensor, tag_per_joint: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """``pred`` as an [N, K, H, W] fp32 view whose planes are dense (only the batch stride is free) and ``tag_ind`` as
    contiguous int32 [N, M, K, 2]; K = 1 without ``tag_per_joint`` (ae.py:41-44)."""
    for t, name in ((pred, "pred"), (tag_ind, "target")):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise _lib.MindposeHipError(f"{name} must be a CUDA tensor: the HIP path has no CPU fallback")
    if tag_ind.dtype.is_floating_point or tag_ind.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"tag_ind must have an integer dtype, got {tag_ind.dtype}")
    if not tag_per_joint:
        if pred.dim() != 3 or tag_ind.dim() != 3:
            raise ValueError("without tag_per_joint pred must be [N,H,W] and the tag indices [N,M,2]")
        pred, tag_ind = pred[:, None], tag_ind[:, :, None]
    if pred.dim() != 4 or tag_ind.dim() != 4 or tag_ind.shape[0] != pred.shape[0] or tag_ind.shape[2] != pred.shape[1] \
            or tag_ind.shape[3] != 2 or tag_ind.shape[1] < 1:
        raise ValueError(f"pred must be [N,K,H,W] and the tag indices [N,M,K,2], got {tuple(pred.shape)} and {tuple(tag_ind.shape)}")
    if pred.dtype != torch.float32:
        pred = pred.float()
    n, k, h, w = pred.shape
    if pred.stride(3) != 1 or pred.stride(2) != w or (k > 1 and pred.stride(1) != h * w) or pred.stride(0) < k * h * w:
        pred = pred.contiguous()
    return pred, tag_ind.to(torch.int32).contiguous()


def launch_ae_fwd(tags: torch.Tensor, tag_ind: torch.Tensor) -> torch.Tensor:
    """``mp_ae_loss_fwd`` on prepared views (``_tag_views``); returns the [2] tensor (push, pull)."""
    lib = _lib.load()
    n, k, h, w = tags.shape
    ws_bytes = lib.mp_ae_loss_workspace_bytes(n)
    ws = torch.empty(ws_bytes // 8, device=tags.device, dtype=torch.float64)
    out = torch.empty(2, device=tags.device, dtype=torch.float32)
    _lib.check(lib.mp_ae_loss_fwd(tags.data_ptr(), tags.stride(0), _lib.ptr(tag_ind), _lib.ptr(out), _lib.ptr(ws), ws_bytes, n,
                                  tag_ind.shape[1], k, h * w, _lib.stream()), "mp_ae_loss_fwd")
    return out


def launch_ae_bwd(tags: torch.Tensor, tag_ind: torch.Tensor, grad_out2: torch.Tensor, grad: torch.Tensor) -> None:
    """``mp_ae_loss_bwd``: writes ``grad`` ([N, K, H, W] with dense planes, e.g. the tag channels of a stage gradient) in place;
    ``grad_out2`` is the contiguous fp32 [2] upstream gradient of (push, pull)."""
    lib = _lib.load()
    n, k, h, w = tags.shape
    _lib.check(lib.mp_ae_loss_bwd(tags.data_ptr(), tags.stride(0), _lib.ptr(tag_ind), _lib.ptr(grad_out2), grad.data_ptr(),
                                  grad.stride(0), n, tag_ind.shape[1], k, h * w, _lib.stream()), "mp_ae_loss_bwd")


class _AELossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tags, tag_ind):
        ctx.save_for_backward(tags, tag_ind)
        return launch_ae_fwd(tags, tag_ind)

    @staticmethod
    def backward(ctx, grad_out):
        tags, tag_ind = ctx.saved_tensors
        grad = torch.empty(tags.shape, device=tags.device, dtype=torch.float32)
        launch_ae_bwd(tags, tag_ind, grad_out.detach().float().reshape(2).contiguous(), grad)
        return grad, None


@register("loss", extra_name="ae")
class AELoss(Loss):
    """Associative embedding loss (`"End-to-End Learning for Joint Detection and Grouping" <https://arxiv.org/abs/1611.05424>`_).

    Inputs: ``pred`` - the predicted tags, [N, K, H, W] (``tag_per_joint``) or [N, H, W]; ``target`` - the tag positions,
    [N, M, K, 2] or [N, M, 2], each entry (flat index into H*W, flag).  Output: the [2] tensor (push loss, pull loss).
    """

    def __init__(self, tag_per_joint: bool = True, reduction: Optional[str] = "mean") -> None:
        super().__init__(reduction=reduction)
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' (the reference recipes' setting) runs on the HIP path")
        self.tag_per_joint = tag_per_joint
        self.eps = 0.01  # compiled into the kernels (ae.py:38)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        tags, tag_ind = _tag_views(pred, target, self.tag_per_joint)
        return _AELossFn.apply(tags, tag_ind)
