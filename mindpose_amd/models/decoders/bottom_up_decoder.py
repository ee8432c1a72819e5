"""Bottom-up (associative-embedding) heat-map decoder on the MI355X HIP path.

Same constructor, call signature and outputs as the reference's ``BottomUpHeatMapAEDecoder``
(mindpose/models/decoders/bottom_up_decoder.py:13-203).  ``decode`` is two launches on the current stream
(``mp_bottomup_parse_nms_topk``, ``mp_bottomup_gather``): stage mean + mask + NMS + per-tile top-k in one, the merge to the
global top ``max_num`` and the tag gather in the other.

Reproduced reference quirk (``shift_coordinate=True``): the +-0.25 offsets are taken at the selected pixels in FLAT-INDEX order
(MindSpore's ``masked_select``) but added to ``ind_k``, which is in VALUE order, so entry m of ``ind_k`` gets the offset of the
m-th smallest selected flat index, not of its own pixel.  The drop-in contract is the reference's output, quirk included.

``decode_flip_aggregated`` is the flip test (the reference's ``_MultiRunNet``, engine/inferencer/bottomup_inferencer.py:252-297):
the same two launches, the first reading the mirrored run's outputs beside the plain ones (``mp_bottomup_parse_nms_topk_flip``).

``decode_multi_scale`` is the multi-scale test (this project's protocol; the reference ships none): the same two
launches again, the first averaging the heat maps of up to four runs at different input scales
(``mp_bottomup_parse_nms_topk_multi``); ``resize_bilinear`` makes the scaled inputs with the decoder's own resize.
"""
import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from ...register import register
from .decoder import Decoder

_MAX_NUM_LIMIT = 64  # csrc/bottomup_ops.hip kBuMaxM
_MAX_LOWER_STAGES = 3
_FLIP_MAX_JOINTS = 64  # csrc/bottomup_ops.hip kBuFlipMaxJoints
_MAX_TAGS = 4  # csrc/bottomup_ops.hip kBuMaxTags
_MAX_RUNS = 4  # csrc/bottomup_ops.hip kBuMaxRuns


def resize_bilinear(x: torch.Tensor, size: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``ops.ResizeBilinear(size)`` with ``align_corners=False, half_pixel_centers=False`` of a CUDA fp32 [N, C, H, W] tensor, one
    launch (``mp_resize_bilinear_nchw``): ``src = dst * (in / out)`` and the fp32 lerp of the decoder's stage resize, not
    ``F.interpolate``, whose ``align_corners=False`` uses half-pixel centres.  ``out``: a contiguous CUDA fp32 [N, C, oh, ow] tensor
    to write into (a plan's ``input_buffer``), which must not overlap ``x``."""
    x = _lib.require_cuda_f32(x, "x")
    if x.dim() != 4:
        raise ValueError(f"x must be [N, C, H, W], got {tuple(x.shape)}")
    oh, ow = (int(v) for v in size)
    n, c, h, w = x.shape
    if oh <= 0 or ow <= 0 or n * c == 0 or h * w == 0:
        raise ValueError(f"cannot resize {tuple(x.shape)} to {(oh, ow)}")
    if out is None:
        out = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32)
    elif not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != x.device or tuple(out.shape) != (n, c, oh, ow) \
            or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous fp32 tensor of shape {(n, c, oh, ow)} on {x.device}")
    elif out.data_ptr() == x.data_ptr():
        raise ValueError("out must not be x")
    _lib.check(_lib.load().mp_resize_bilinear_nchw(_lib.ptr(x), _lib.ptr(out), n * c, h, w, oh, ow, _lib.stream()),
               "mp_resize_bilinear_nchw")
    return out


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
        return self._launch(self._stages(heatmap, tagging_heatmap), mask)

    def decode_flip_aggregated(self, outputs: Sequence[torch.Tensor], flipped_outputs: Sequence[torch.Tensor],
                               flip_index: Sequence[int], mask: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """The flip test's aggregation and decode (reference: engine/inferencer/bottomup_inferencer.py:269-297) in the decoder's two
        launches.  ``outputs`` are the raw stage outputs A of ``net(image)``, ``flipped_outputs`` those of ``net(flip_W(image))``,
        B; ``flip_index`` f is the joint permutation of ``load_inference_cfg``.  Returns ``decode``'s five tensors with
        tagging [N, K, H, W, 2L] and tag_k [N, K, M, 2L], L = the number of tag stages.

        Per stage i, at stage resolution, before any resize (``ops.ResizeBilinear`` here has no half-pixel centres, so resizing and
        mirroring do not commute; every tap of the resize is the averaged value):

            heat_i[n, k, y, x] = (A_i[n, k, y, x] + B_i[n, f[k], y, Ws_i - 1 - x]) * 0.5        (one fp32 add, one fp32 multiply)

        and the last axis of tagging holds the plain tags A_i[n, K + k, y, x] of the tag stages in stage order, then the
        flipped-back tags B_i[n, K + f[k], y, Ws_i - 1 - x] in the same order.  ``decode`` of those lists follows unchanged: stage
        mean, the same un-mirrored mask, NMS, top-k, tag gather, shift quirk.  B is read mirrored inside the launch: there is no
        flip, gather, average or concat pass over the maps.

        Two oddities of the reference:

        1. It writes ``(heatmap + flipped_heatmap) * 0.5`` on Python lists, which concatenates the lists and then fails on
           ``list * float``: as written it runs for no ``num_stages``.  This builds the evident intent, the per-stage mean above.
        2. ``_flip_back`` indexes the tag tensors with the K-long ``flip_index`` too.  With ``tag_per_joint=False`` (one tag
           channel) that is out of range in the reference: ``ValueError`` here.  A ``flip_index`` that is not a permutation of
           ``range(num_joints)`` would silently give ``len(flip_index)`` channels there: ``ValueError`` here."""
        index = self.check_flip_index(flip_index)
        heatmap, tagging_heatmap = self.decouple_output(outputs)
        stages = self._stages(heatmap, tagging_heatmap)
        flipped = self._stages(*self.decouple_output(flipped_outputs))
        for i, ((a, _), (b, _)) in enumerate(zip(stages, flipped)):
            if a.shape != b.shape or a.device != b.device:
                raise ValueError(f"stage {i} of the mirrored run is {tuple(b.shape)}, of the plain run {tuple(a.shape)}")
        return self._launch(stages, mask, flipped, index)

    def decode_multi_scale(self, runs: Sequence[Sequence[torch.Tensor]], mask: torch.Tensor, base: int,
                           flipped_runs: Optional[Sequence[Sequence[torch.Tensor]]] = None,
                           flip_index: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, ...]:
        """The multi-scale test's aggregation and decode in the decoder's two launches.  ``runs[r]`` are the raw stage outputs of
        the network on the batch resized by scale factor r (``resize_bilinear``), ``runs[base]`` those of the batch itself;
        ``flipped_runs[r]`` / ``flip_index`` add the flip test, run by run, as ``decode_flip_aggregated`` defines it.  Returns
        ``decode``'s five tensors at the map size of ``runs[base]``.

        With t_{r,i} stage i of run r at stage resolution (under the flip test the mean with the mirrored run,
        ``(A + B[f][..., ::-1]) * 0.5``) and R the ``ops.ResizeBilinear`` to the base map (no half-pixel centres; the direct read for
        the base run's last stage)::

            v_r   = R(t_{r,last});  v_r = v_r + R(t_{r,i}) for i = 0 .. num_stages - 2;  v_r = v_r / num_stages  (more than one stage)
            total = v_0 + v_1 + ...  in list order;  total = total / len(runs)  (more than one run)

        ``total`` is masked and decoded as ``decode`` does its stage mean.  The tags are the base run's alone - L slots, 2L under
        the flip test, the plain ones first - and the tag channels of the other runs are never read.  One run is ``decode`` (or
        ``decode_flip_aggregated``) operation for operation.  A stage of another run may be smaller or larger than the map."""
        if not 1 <= len(runs) <= _MAX_RUNS:
            raise ValueError(f"the multi-scale test takes 1 to {_MAX_RUNS} runs, got {len(runs)}")
        if not isinstance(base, int) or not 0 <= base < len(runs):
            raise ValueError(f"base must index one of the {len(runs)} runs, got {base!r}")
        if (flipped_runs is None) != (flip_index is None):
            raise ValueError("flipped_runs and flip_index go together")
        index = None if flip_index is None else self.check_flip_index(flip_index)
        if flipped_runs is not None and len(flipped_runs) != len(runs):
            raise ValueError(f"{len(flipped_runs)} mirrored runs beside {len(runs)} runs")
        plain = [self._stages(*self.decouple_output(o)) for o in runs]
        mirrored = None if flipped_runs is None else [self._stages(*self.decouple_output(o)) for o in flipped_runs]
        dev, n = plain[base][-1][0].device, plain[base][-1][0].shape[0]
        for r, stages in enumerate(plain):
            for i, (a, _) in enumerate(stages):
                if a.shape[0] != n or a.device != dev:
                    raise ValueError(f"stage {i} of run {r} is {tuple(a.shape)} on {a.device}, the base run has batch {n} on {dev}")
                if mirrored is not None and (mirrored[r][i][0].shape != a.shape or mirrored[r][i][0].device != dev):
                    raise ValueError(f"stage {i} of mirrored run {r} is {tuple(mirrored[r][i][0].shape)}, of the plain run "
                                     f"{tuple(a.shape)}")
        return self._launch(plain[base], mask, None if mirrored is None else mirrored[base], index, runs=(plain, mirrored, base))

    def check_flip_index(self, flip_index) -> np.ndarray:
        """``flip_index`` as int32 [num_joints], after the checks of the flip test: ``ValueError`` unless it is a permutation of
        ``range(num_joints)`` and the decoder has one tag channel per joint, two tag slots per tag stage and a joint count the
        kernel carries."""
        if not self.tag_per_joint:
            raise ValueError("flip TTA needs tag_per_joint=True: the flip index permutes one tag channel per joint")
        index = np.asarray(flip_index.cpu() if torch.is_tensor(flip_index) else flip_index)
        if index.ndim != 1 or index.size != self.num_joints or index.dtype.kind not in "iu" or \
                not np.array_equal(np.sort(index), np.arange(self.num_joints)):
            raise ValueError(f"flip_index must be a permutation of range({self.num_joints}), got {index.tolist()}")
        if self.num_joints > _FLIP_MAX_JOINTS:
            raise ValueError(f"flip TTA carries at most {_FLIP_MAX_JOINTS} joints on the HIP path, got {self.num_joints}")
        if 2 * sum(bool(a) for a in self.with_ae_loss[:self.num_stages]) > _MAX_TAGS:
            raise ValueError(f"flip TTA doubles the tags: at most {_MAX_TAGS // 2} stages may carry them")
        return np.ascontiguousarray(index, dtype=np.int32)

    def _launch(self, stages, mask, flipped=None, flip_index=None, runs=None):
        """The two launches on ``stages`` (``_stages``); with ``flipped`` / ``flip_index`` the first one is the flip form.  ``runs`` =
        (the ``_stages`` of every run, those of their mirrored partners or None, the base run's position) makes it the multi-scale
        form, ``stages`` / ``flipped`` being the base run's."""
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
        num_tags = sum(1 for _, has in stages if has) * (1 if flipped is None else 2)
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

        def describe(items):
            return (_lib.BottomUpStage * len(items))(*[
                _lib.BottomUpStage(data=t.data_ptr(), c=t.shape[1], h=t.shape[2], w=t.shape[3], has_tags=int(has)) for t, has in items])

        stream = _lib.stream()
        nms = self.nms_kernel if self.use_nms else 1
        tail = (len(stages), _lib.ptr(mask), mask.shape[1], mask.shape[2], n, k, int(self.tag_per_joint), nms, m,
                _lib.ptr(heatmap_raw), _lib.ptr(tagging), _lib.ptr(ws), ws_bytes, stream)
        index = None if flip_index is None else flip_index.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if runs is not None:
            plain, mirrored, base = runs
            arrays = [(describe(p), None if mirrored is None else describe(mirrored[r])) for r, p in enumerate(plain)]  # kept alive
            table = (_lib.BottomUpRun * len(arrays))(*[_lib.BottomUpRun(stages=a, flipped=b) for a, b in arrays])
            _lib.check(lib.mp_bottomup_parse_nms_topk_multi(table, len(arrays), base, index, *tail), "mp_bottomup_parse_nms_topk_multi")
        elif flipped is None:
            _lib.check(lib.mp_bottomup_parse_nms_topk(describe(stages), *tail), "mp_bottomup_parse_nms_topk")
        else:
            _lib.check(lib.mp_bottomup_parse_nms_topk_flip(describe(stages), describe(flipped), index, *tail),
                       "mp_bottomup_parse_nms_topk_flip")
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
