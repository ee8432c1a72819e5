"""AEMultiLoss - heat-map MSE plus associative-embedding loss over the resolution levels of a bottom-up model (reference:
mindpose/models/loss/multi_loss.py:12-107).

One ``torch.autograd.Function`` spans the list of stage predictions.  Its forward launches ``mp_joints_mse_mask_fwd`` on the
heat-map channels and ``mp_ae_loss_fwd`` on the tag channels of every enabled stage - all operands are views of the stage
tensors and of the padded ``target`` / ``mask`` / ``tag_ind`` batch arrays, read in place.  Its backward allocates ONE gradient
per stage, of the prediction's full shape: the MSE kernel fills the heat-map channels, the AE kernel the tag channels, and
channels (or stages) without an enabled term are zero.
"""
from typing import List, Sequence, Tuple

import torch

from ... import _lib
from ...register import register
from .ae import AELoss, _tag_views, launch_ae_bwd, launch_ae_fwd
from .loss import Loss
from .mse import JointsMSELossWithMask, _mask_view, _view4, launch_mse_mask_bwd, launch_mse_mask_fwd


class _AEMultiLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, target, mask, tag_ind, *preds):
        k = cfg.num_joints
        dev = preds[0].device
        total = [torch.zeros(1, device=dev, dtype=torch.float32) for _ in range(3)]
        saved, plan = [], []
        for i in range(cfg.num_stages):
            w, h = (int(v) for v in cfg.stage_sizes[i])
            pred = preds[i]
            entry = dict(shape=tuple(pred.shape), mse=None, ae=None)
            if cfg.with_mse_loss[i]:
                pv, tv = _view4(pred[:, :k], "preds"), _view4(target[:, i, :, :h, :w], "target")
                mv = _mask_view(mask[:, i, :h, :w], (pred.shape[0], h, w))
                total[0] = total[0] + launch_mse_mask_fwd(pv, tv, mv) * float(cfg.mse_loss_factor[i])
                entry["mse"] = len(saved)
                saved += [pv, tv, mv]
            if cfg.with_ae_loss[i]:
                tags = pred[:, k:] if cfg.tag_per_joint else pred[:, k]
                tags, tind = _tag_views(tags, tag_ind[:, i], cfg.tag_per_joint)
                both = launch_ae_fwd(tags, tind) * float(cfg.ae_loss_factor[i])
                total[1], total[2] = total[1] + both[0:1], total[2] + both[1:2]
                entry["ae"] = len(saved)
                saved += [tags, tind]
            plan.append(entry)
        ctx.save_for_backward(*saved)
        ctx.plan, ctx.cfg, ctx.num_preds = plan, cfg, len(preds)
        return torch.cat(total)

    @staticmethod
    def backward(ctx, grad_out):
        cfg, saved = ctx.cfg, ctx.saved_tensors
        k = cfg.num_joints
        go = grad_out.detach().float().reshape(3)
        grads: List[torch.Tensor] = []
        for i, entry in enumerate(ctx.plan):
            shape = entry["shape"]
            if entry["mse"] is None and entry["ae"] is None:
                grads.append(torch.zeros(shape, device=go.device, dtype=torch.float32))
                continue
            grad = torch.empty(shape, device=go.device, dtype=torch.float32)
            if entry["mse"] is not None:
                pv, tv, mv = saved[entry["mse"]:entry["mse"] + 3]
                launch_mse_mask_bwd(pv, tv, mv, (go[0:1] * float(cfg.mse_loss_factor[i])).contiguous(), grad[:, :k])
            else:
                grad[:, :k].zero_()
            tag_end = k
            if entry["ae"] is not None:
                tags, tind = saved[entry["ae"]:entry["ae"] + 2]
                tag_end = k + tags.shape[1]
                launch_ae_bwd(tags, tind, (go[1:3] * float(cfg.ae_loss_factor[i])).contiguous(), grad[:, k:tag_end])
            if tag_end < shape[1]:
                grad[:, tag_end:].zero_()
            grads.append(grad)
        grads += [None] * (ctx.num_preds - len(grads))
        return (None, None, None, None, *grads)


@register("loss", extra_name="ae_multi_loss")
class AEMultiLoss(Loss):
    """Combined MSE and AE loss over several resolution levels.

    Inputs: ``preds`` - one [N, aK, H, W] prediction per level (a = 2 where the level has tags); ``target`` - [N, S, K, Hmax, Wmax],
    smaller levels zero-padded; ``mask`` - [N, S, Hmax, Wmax] (float32, uint8 or bool); ``tag_ind`` - [N, S, M, K, 2]
    ([N, S, M, 2] without ``tag_per_joint``).  ``stage_sizes`` entries are (W, H).  Output: the [3] tensor (mse, push, pull).
    """

    def __init__(
        self,
        num_joints: int = 17,
        num_stages: int = 2,
        stage_sizes: List[Tuple[int, int]] = [(128, 128), (256, 256)],
        mse_loss_factor: List[float] = [1.0, 1.0],
        ae_loss_factor: List[float] = [0.001, 0.001],
        with_mse_loss: List[bool] = [True, True],
        with_ae_loss: List[bool] = [True, False],
        tag_per_joint: bool = True,
    ) -> None:
        super().__init__()
        self.mse_criterion = JointsMSELossWithMask()
        self.ae_criterion = AELoss(tag_per_joint=tag_per_joint)
        for name, seq in (("stage_sizes", stage_sizes), ("mse_loss_factor", mse_loss_factor), ("ae_loss_factor", ae_loss_factor),
                          ("with_mse_loss", with_mse_loss), ("with_ae_loss", with_ae_loss)):
            if len(seq) < num_stages:
                raise ValueError(f"{name} needs one entry per stage ({num_stages}), got {len(seq)}")
        self.num_joints = num_joints
        self.num_stages = num_stages
        self.stage_sizes = stage_sizes
        self.mse_loss_factor = mse_loss_factor
        self.ae_loss_factor = ae_loss_factor
        self.with_mse_loss = with_mse_loss
        self.with_ae_loss = with_ae_loss
        self.tag_per_joint = tag_per_joint

    def _validate(self, preds: Sequence[torch.Tensor], target: torch.Tensor, mask: torch.Tensor, tag_ind: torch.Tensor) -> None:
        if not isinstance(preds, (list, tuple)) or len(preds) < self.num_stages:
            raise ValueError(f"preds must be a list of {self.num_stages} stage predictions")
        for t, name in [(p, "preds") for p in preds[:self.num_stages]] + [(target, "target"), (mask, "mask"), (tag_ind, "tag_ind")]:
            if not torch.is_tensor(t):
                raise TypeError(f"{name} must be a torch.Tensor")
            if not t.is_cuda:
                raise _lib.MindposeHipError(f"{name} must be a CUDA tensor: the HIP path has no CPU fallback")
        k, s = self.num_joints, self.num_stages
        n = preds[0].shape[0]
        if target.dim() != 5 or target.shape[0] != n or target.shape[1] < s or target.shape[2] != k:
            raise ValueError(f"target must be [N,S,K,Hmax,Wmax] with N = {n}, S >= {s}, K = {k}, got {tuple(target.shape)}")
        if mask.dim() != 4 or mask.shape[0] != n or mask.shape[1] < s or tuple(mask.shape[2:]) != tuple(target.shape[3:]):
            raise ValueError(f"mask must be [N,S,Hmax,Wmax] matching target, got {tuple(mask.shape)}")
        if mask.dtype not in (torch.float32, torch.uint8, torch.bool):
            raise ValueError(f"mask must be float32, uint8 or bool, got {mask.dtype}")
        want = 5 if self.tag_per_joint else 4
        if tag_ind.dim() != want or tag_ind.shape[0] != n or tag_ind.shape[1] < s or tag_ind.shape[-1] != 2 \
                or (self.tag_per_joint and tag_ind.shape[3] != k):
            raise ValueError(f"tag_ind must be [N,S,M,K,2] ([N,S,M,2] without tag_per_joint), got {tuple(tag_ind.shape)}")
        if tag_ind.dtype.is_floating_point or tag_ind.dtype == torch.bool:
            raise ValueError(f"tag_ind must have an integer dtype, got {tag_ind.dtype}")
        for i in range(s):
            w, h = (int(v) for v in self.stage_sizes[i])
            need = k + ((k if self.tag_per_joint else 1) if self.with_ae_loss[i] else 0)
            p = preds[i]
            if p.dim() != 4 or p.shape[0] != n or p.shape[1] < need or tuple(p.shape[2:]) != (h, w):
                raise ValueError(f"preds[{i}] must be [N, >= {need}, {h}, {w}], got {tuple(p.shape)}")
            if self.tag_per_joint and self.with_ae_loss[i] and p.shape[1] != 2 * k:
                raise ValueError(f"preds[{i}] must have {2 * k} channels (heat maps + one tag map per joint), got {p.shape[1]}")
            if h > target.shape[3] or w > target.shape[4]:
                raise ValueError(f"stage {i} ({w} x {h}) does not fit the padded target {tuple(target.shape[3:])}")

    def forward(self, preds: List[torch.Tensor], target: torch.Tensor, mask: torch.Tensor, tag_ind: torch.Tensor) -> torch.Tensor:
        self._validate(preds, target, mask, tag_ind)
        stages = [p if p.dtype == torch.float32 and p.is_contiguous() else p.float().contiguous() for p in preds[:self.num_stages]]
        if target.dtype != torch.float32:
            target = target.float()
        return _AEMultiLossFn.apply(self, target, mask, tag_ind.to(torch.int32), *stages)
