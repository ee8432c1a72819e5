"""Bottom-up (associative-embedding) heat-map decoder on the MI355X HIP path.

Same constructor, call signature and outputs as the reference's ``BottomUpHeatMapAEDecoder``
(mindpose/models/decoders/bottom_up_decoder.py:13-203).  ``decode`` is two launches on the current stream
(``mp_bottomup_parse_nms_topk``, ``mp_bottomup_gather``): stage mean + mask + NMS + per-tile top-k in one, the merge to the
global top ``max_num`` and the tag gather in the other.

Reproduced reference quirk (``shift_coordinate=True``): the +-0.25 offsets are taken at the selected pixels in FLAT-INDEX order
(MindSpore's ``masked_select``) but added to ``ind_k``, which is in VALUE order, so entry m of ``ind_k`` gets the offset of the
m-th smallest selected flat index, not of its own pixel.  The drop-in contract is the reference's output, quirk included.
"""
from typing import List, Sequence, Tuple

import torch

from ... import _lib
from ...register import register
from .decoder import Decoder

_MAX_NUM_LIMIT = 64  # csrc/bottomup_ops.hip kBuMaxM
_MAX_LOWER_STAGES = 3


@register("decoder", extra_name="bottomup_heatmap_ae")
class BottomUpHeatMapAEDecoder(Decoder):
    def __init__(self, num_joints: int = 17, num_stages: int = 2, with_ae_loss: List[bool] = [True, False], use_nms: bool = False,
                 nms_kernel: int = 5, max_num: int = 30, tag_per_joint: bool = True, shift_coordinate: bool = False) -> None:
        super().__init__()
        self.num_joints = num_joints
        self.num_stages = num_stages
        self.with_ae_loss = with_ae_loss
        self.use_nms = use_nms
        self.nms_kernel = nms_kernel
        self.max_num = max_num
        self.tag_per_joint = tag_per_joint
        self.shift_coordinate = shift_coordinate
        if not 1 <= num_stages <= _MAX_LOWER_STAGES + 1:
            raise ValueError(f"num_stages must be 1 to {_MAX_LOWER_STAGES + 1}")
        if len(with_ae_loss) < num_stages:
            raise ValueError("with_ae_loss needs one entry per stage")
        if not any(with_ae_loss[:num_stages]):
            raise ValueError("at least one stage must carry the associative-embedding tags")
        if use_nms and nms_kernel not in (1, 3, 5, 7):
            raise ValueError("nms_kernel must be 1, 3, 5 or 7")
        if not 1 <= max_num <= _MAX_NUM_LIMIT:
            raise ValueError(f"max_num must be 1 to {_MAX_NUM_LIMIT} on the HIP path, got {max_num}")

    def forward(self, model_output: Sequence[torch.Tensor], mask: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        heatmap, tagging_heatmap = self.decouple_output(model_output)
        return self.decode(heatmap, tagging_heatmap, mask)

    def decouple_output(self, output: Sequence[torch.Tensor]) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        """bottom_up_decoder.py:93-100: the first num_joints channels of every stage are heat maps, the rest of a stage with
        ``with_ae_loss`` its tags (views, no copy)."""
        if len(output) < self.num_stages:
            raise ValueError(f"expected {self.num_stages} model outputs, got {len(output)}")
        heatmap, tagging = [], []
        for i in range(self.num_stages):
            heatmap.append(output[i][:, :self.num_joints])
            if self.with_ae_loss[i]:
                tagging.append(output[i][:, self.num_joints:])
        return heatmap, tagging

    def decode(self, heatmap: Sequence[torch.Tensor], tagging_heatmap: Sequence[torch.Tensor],
               mask: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """(val_k [N,K,M], tag_k [N,K,M,L], ind_k [N,K,M,2], heatmap_raw [N,K,H,W], tagging [N,K_tag,H,W,L]), CUDA fp32.

        ``heatmap`` / ``tagging_heatmap`` are the lists ``decouple_output`` makes; both must be channel slices of the same
        stage tensors (the kernels read each stage once, heat maps and tags together)."""
        stages = self._stages(heatmap, tagging_heatmap)
        full = stages[-1][0]
        dev = full.device
        n, k, h, w = full.shape[0], self.num_joints, full.shape[2], full.shape[3]
        if h * w < self.max_num:
            raise ValueError(f"max_num {self.max_num} exceeds the {h}x{w} heat-map pixels")
        if not torch.is_tensor(mask):
            raise TypeError("mask must be a torch.Tensor")
        if mask.dim() != 3 or mask.shape[0] != n:
            raise ValueError(f"mask must be [N, H, W] with N = {n}, got {tuple(mask.shape)}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"mask must be bool or uint8, got {mask.dtype}")
        mask = mask.to(dev).to(torch.uint8).contiguous()
        ktag = k if self.tag_per_joint else 1
        num_tags = sum(1 for _, has in stages if has)
        m = self.max_num
        f32 = dict(device=dev, dtype=torch.float32)
        heatmap_raw = torch.empty(n, k, h, w, **f32)
        tagging = torch.empty(n, ktag, h, w, num_tags, **f32)
        val_k = torch.empty(n, k, m, **f32)
        ind_k = torch.empty(n, k, m, 2, **f32)
        tag_k = torch.empty(n, k, m, num_tags, **f32)
        lib = _lib.load()
        ws_bytes = lib.mp_bottomup_workspace_bytes(n, k, h, w, m)
        ws = torch.empty((ws_bytes + 7) // 8, device=dev, dtype=torch.int64)
        descs = (_lib.BottomUpStage * len(stages))(*[
            _lib.BottomUpStage(data=t.data_ptr(), c=t.shape[1], h=t.shape[2], w=t.shape[3], has_tags=int(has)) for t, has in stages])
        stream = _lib.stream()
        nms = self.nms_kernel if self.use_nms else 1
        _lib.check(lib.mp_bottomup_parse_nms_topk(descs, len(stages), _lib.ptr(mask), mask.shape[1], mask.shape[2], n, k,
                                                  int(self.tag_per_joint), nms, m, _lib.ptr(heatmap_raw), _lib.ptr(tagging),
                                                  _lib.ptr(ws), ws_bytes, stream), "mp_bottomup_parse_nms_topk")
        _lib.check(lib.mp_bottomup_gather(_lib.ptr(heatmap_raw), _lib.ptr(tagging), _lib.ptr(ws), ws_bytes, n, k, h, w,
                                          int(self.tag_per_joint), num_tags, m, int(self.shift_coordinate), _lib.ptr(val_k),
                                          _lib.ptr(ind_k), _lib.ptr(tag_k), stream), "mp_bottomup_gather")
        return val_k, tag_k, ind_k, heatmap_raw, tagging

    def _stages(self, heatmap, tagging_heatmap):
        """[(stage tensor [N, C, Hs, Ws] contiguous fp32, has_tags)] in stage order, recovered from the decoupled slices."""
        if len(heatmap) != self.num_stages:
            raise ValueError(f"expected {self.num_stages} heat maps, got {len(heatmap)}")
        n_ae = sum(bool(a) for a in self.with_ae_loss[:self.num_stages])
        if len(tagging_heatmap) != n_ae:
            raise ValueError(f"expected {n_ae} tagging heat maps, got {len(tagging_heatmap)}")
        ktag = self.num_joints if self.tag_per_joint else 1
        stages, t_iter = [], iter(tagging_heatmap)
        for i, hm in enumerate(heatmap):
            if not torch.is_tensor(hm):
                raise TypeError("model outputs must be torch.Tensor")
            if hm.dim() != 4 or hm.shape[1] != self.num_joints:
                raise ValueError(f"stage {i} heat maps must be [N, {self.num_joints}, H, W], got {tuple(hm.shape)}")
            has = bool(self.with_ae_loss[i])
            parts = [hm]
            if has:
                tg = next(t_iter)
                if tg.dim() != 4 or tg.shape[1] != ktag or tg.shape[0] != hm.shape[0] or tg.shape[2:] != hm.shape[2:]:
                    raise ValueError(f"stage {i} tags must be [N, {ktag}, H, W] beside its heat maps, got {tuple(tg.shape)}")
                parts.append(tg)
            base = self._base_of(parts)
            if base is None:  # not slices of one contiguous stage tensor: rebuild it
                base = torch.cat([p.float() for p in parts], 1)
            base = _lib.require_cuda_f32(base, f"stage {i}")
            stages.append((base, has))
        n, h, w = stages[-1][0].shape[0], stages[-1][0].shape[2], stages[-1][0].shape[3]
        for i, (t, _) in enumerate(stages[:-1]):
            if t.shape[0] != n:
                raise ValueError(f"stage {i} batch {t.shape[0]} != {n}")
            if t.shape[2] > h or t.shape[3] > w:
                raise ValueError("the last stage must have the largest resolution")
        return stages

    @staticmethod
    def _base_of(parts):
        """The contiguous fp32 stage tensor whose leading channel slices ``parts`` are, else None."""
        first = parts[0]
        if first.dtype != torch.float32 or not first.is_cuda:
            return None
        n, c0, h, w = first.shape
        total = sum(p.shape[1] for p in parts)
        if first.stride() != (total * h * w, h * w, w, 1):
            return None
        offset = first.storage_offset()
        for p in parts[1:]:
            if p.dtype != torch.float32 or p.stride() != first.stride() or p.storage_offset() != offset + c0 * h * w:
                return None
            if p.untyped_storage().data_ptr() != first.untyped_storage().data_ptr():
                return None
            offset, c0 = p.storage_offset(), p.shape[1]
        return first.as_strided((n, total, h, w), first.stride(), first.storage_offset())
