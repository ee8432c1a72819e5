"""Associative-embedding grouping (reference: mindpose/utils/match.py:15-116), host numpy.

Joints are visited in ``joint_order``; the detections of a joint above ``vis_thr`` are assigned to the existing person groups by
the Hungarian algorithm on the L2 distance between their tag and each group's mean tag (rounded to integers with
``use_rounded_norm``), through ``scipy.optimize.linear_sum_assignment`` - the reference's own solver.  With rounded costs the
matrix is full of ties and another solver could return another optimum, so it is not replaced.  A detection without a match
closer than ``tag_thr`` opens a new group keyed by its first tag value (a later detection with the same key overwrites that
group, as the reference's dict does).

``match_by_tag_batch`` is the same function for the N images of a decoder output on the device: ONE launch of
``mp_bottomup_match_by_tag`` (bottomup_match.hip, one wave per image), which restates scipy's solver - tie order included - and
numpy's float32 reductions, so its arrays are bit-equal to the host function's.  ``match_by_tag_device`` is that launch without
the downloads, and ``finish_people_batch`` the rest of a batch on the persons it left on the device: scores, mean tags and the
missing-joint refinement by ``mp_bottomup_finish_people`` (bottomup_ops.hip), then two downloads.
"""
import ctypes
from typing import Callable, Dict, List, Sequence, Tuple, Union

import numpy as np
import scipy.optimize
import torch

from .. import _lib


def _assign(cost: np.ndarray) -> np.ndarray:
    """[num_pairs, 2] int32 (row, column) of a minimum-cost assignment."""
    rows, cols = scipy.optimize.linear_sum_assignment(cost)
    return np.array((rows, cols)).T.astype(np.int32)


def match_by_tag(val_k: np.ndarray, tag_k: np.ndarray, ind_k: np.ndarray, joint_order: List[int], vis_thr: float = 0.1,
                 tag_thr: float = 1, ignore_too_much: bool = False, use_rounded_norm: bool = True) -> np.ndarray:
    """val_k [K, M], tag_k [K, M, L], ind_k [K, M, 2 (x, y)] of one image -> [P, K, 3 + L] float32 (x, y, value, tags) per
    person group, in the order the groups were opened; an empty array when nothing passes ``vis_thr``."""
    num_joints, max_num, num_tags = tag_k.shape
    # per joint and candidate: x, y, value, tags
    candidates = np.concatenate((ind_k, val_k[..., None], tag_k), axis=2)
    empty_person = np.zeros((num_joints, 3 + num_tags), np.float32)
    people: Dict = {}      # group key -> [K, 3 + L] joints of that person
    group_tags: Dict = {}  # group key -> list of the tags assigned to it

    def open_group(key, joint, row, tag):
        people.setdefault(key, empty_person.copy())[joint] = row
        group_tags[key] = [tag]

    for step in range(num_joints):
        joint = joint_order[step]
        visible = candidates[joint][:, 2] > vis_thr
        tags = tag_k[joint][visible]
        if tags.shape[0] == 0:
            continue
        rows = candidates[joint][visible]

        if step == 0 or not people:
            for j in range(tags.shape[0]):
                open_group(tags[j, 0], joint, rows[j], tags[j])
            continue

        keys = list(people)
        means = [np.mean(np.stack(group_tags[key]), axis=0) for key in keys]
        if ignore_too_much and len(keys) == max_num:
            continue
        means = np.stack(means)

        dist = np.linalg.norm(rows[:, None, 3:] - means[None, :, :], ord=2, axis=2)
        cost = np.round(dist) if use_rounded_norm else dist.copy()
        n_new, n_groups = dist.shape
        if n_new > n_groups:  # more detections than groups: dummy columns that no real match undercuts
            cost = np.concatenate((cost, np.zeros((n_new, n_new - n_groups), np.float32) + 1e10), axis=1)

        for r, c in _assign(cost):
            if r < n_new and c < n_groups and dist[r][c] < tag_thr:
                key = keys[c]
                people[key][joint] = rows[r]
                group_tags[key].append(tags[r])
            else:
                open_group(tags[r, 0], joint, rows[r], tags[r])

    return np.array(list(people.values())).astype(np.float32)


_BATCH_BUFFERS: Dict = {}  # (device, N, K, M, L) -> people, (counts, status), workspace, workspace bytes


def match_on_device_supported(num_joints: int, max_num: int, num_tags: int) -> bool:
    """Whether ``match_by_tag_batch`` carries these extents (the entry's own limits, asked host-only)."""
    return bool(_lib.load().mp_bottomup_match_supported(num_joints, max_num, num_tags))


def _batch_buffers(device, n, k, m, num_tags):
    key = (device, n, k, m, num_tags)
    if key not in _BATCH_BUFFERS:
        if len(_BATCH_BUFFERS) >= 8:  # a few batch shapes recur (the last batch of an epoch, the two eval sizes); keep no history
            _BATCH_BUFFERS.clear()
        ws_bytes = _lib.load().mp_bottomup_match_workspace_bytes(n, k, m, num_tags)
        _BATCH_BUFFERS[key] = (torch.empty(n, k * m, k, 3 + num_tags, device=device, dtype=torch.float32),
                               torch.empty(2, n, device=device, dtype=torch.int32),
                               torch.empty((ws_bytes + 7) // 8, device=device, dtype=torch.int64), ws_bytes)
    return _BATCH_BUFFERS[key]


def match_by_tag_batch(val_k: torch.Tensor, tag_k: torch.Tensor, ind_k: torch.Tensor, joint_order: Sequence[int], vis_thr: float = 0.1,
                       tag_thr: float = 1, ignore_too_much: bool = False, use_rounded_norm: bool = True, download: bool = True
                       ) -> Union[List[np.ndarray], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """``match_by_tag`` of every image of val_k [N, K, M], tag_k [N, K, M, L], ind_k [N, K, M, 2] (CUDA fp32, the decoder's
    outputs) in one launch on the current stream -> N arrays [P_i, K, 3 + L], each bit-equal to ``match_by_tag`` of that image.
    Two downloads: the person counts with the status words, then the persons up to the largest count.  An image whose visible
    detections carry a NaN or infinite tag is grouped by the host function (which raises what scipy raises).
    ``download=False`` stops behind the launch and returns what ``match_by_tag_device`` returns (the inferencer's way in: one
    name stands for "the batch was grouped on the device", whatever follows)."""
    val_k, tag_k, ind_k = (_lib.require_cuda_f32(t, name) for t, name in ((val_k, "val_k"), (tag_k, "tag_k"), (ind_k, "ind_k")))
    if not download:
        return match_by_tag_device(val_k, tag_k, ind_k, joint_order, vis_thr=vis_thr, tag_thr=tag_thr, ignore_too_much=ignore_too_much,
                                   use_rounded_norm=use_rounded_norm)
    people, counts, status = match_by_tag_device(val_k, tag_k, ind_k, joint_order, vis_thr=vis_thr, tag_thr=tag_thr,
                                                 ignore_too_much=ignore_too_much, use_rounded_norm=use_rounded_norm)
    n = people.shape[0]
    if n == 0:
        return []
    host_match = host_match_of(val_k, tag_k, ind_k, joint_order, vis_thr=vis_thr, tag_thr=tag_thr, ignore_too_much=ignore_too_much,
                               use_rounded_norm=use_rounded_norm)
    counts, status = _meta_of(counts, status).cpu().numpy()
    counts = np.where(status == 0, counts, 0)  # (the kernel reports 0 persons for an image it hands over; not relied upon)
    top = int(counts.max())
    persons = people[:, :top].cpu().numpy() if top else None  # None: every image is empty or handed over - never indexed below
    out = []
    for i in range(n):
        if status[i] != 0:  # rare: three small downloads of this image alone
            out.append(host_match(i))
        elif counts[i] == 0:
            out.append(np.array([]).astype(np.float32))  # the host function's empty result
        else:
            out.append(persons[i, :counts[i]].copy())
    return out


def match_by_tag_device(val_k: torch.Tensor, tag_k: torch.Tensor, ind_k: torch.Tensor, joint_order: Sequence[int], vis_thr: float = 0.1,
                        tag_thr: float = 1, ignore_too_much: bool = False, use_rounded_norm: bool = True
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The grouping launch of ``match_by_tag_batch`` alone, on the current stream, with no download: the device tensors
    ``people`` [N, K * M, K, 3 + L] fp32, ``counts`` [N] and ``status`` [N] int32 as ``mp_bottomup_match_by_tag`` leaves them
    (include/mindpose_hip.h): image i has ``counts[i]`` persons at ``people[i, :counts[i]]`` when ``status[i] == 0``, the rows behind
    them are uninitialised memory, and ``status[i] != 0`` hands the image to the host function.  The three are VIEWS of buffers cached
    per batch shape: valid until the next call of that shape (``match_by_tag_batch`` included), which overwrites them.  N = 0 gives
    empty tensors without a launch."""
    val_k, tag_k, ind_k = (_lib.require_cuda_f32(t, name) for t, name in ((val_k, "val_k"), (tag_k, "tag_k"), (ind_k, "ind_k")))
    if val_k.dim() != 3 or tag_k.dim() != 4 or tag_k.shape[:3] != val_k.shape or ind_k.shape != val_k.shape + (2,):
        raise ValueError(f"expected val_k [N, K, M], tag_k [N, K, M, L], ind_k [N, K, M, 2], got {tuple(val_k.shape)}, "
                         f"{tuple(tag_k.shape)}, {tuple(ind_k.shape)}")
    n, k, m = val_k.shape
    num_tags = tag_k.shape[3]
    order = np.asarray(joint_order)
    if order.shape != (k,) or order.dtype.kind not in "iu" or not np.array_equal(np.sort(order), np.arange(k)):
        raise ValueError(f"joint_order must be a permutation of range({k}), got {list(joint_order)}")
    if n == 0:
        meta = torch.empty(2, 0, device=val_k.device, dtype=torch.int32)
        return torch.empty(0, k * m, k, 3 + num_tags, device=val_k.device, dtype=torch.float32), meta[0], meta[1]
    if not match_on_device_supported(k, m, num_tags):
        raise _lib.MindposeHipError(f"match_by_tag_batch carries K <= 64, M <= 64, L <= 4 and K * M <= 1024, got K = {k}, M = {m}, "
                                    f"L = {num_tags}")
    people, meta, ws, ws_bytes = _batch_buffers(val_k.device, n, k, m, num_tags)
    order_c = (ctypes.c_int * k)(*[int(j) for j in order])
    _lib.check(_lib.load().mp_bottomup_match_by_tag(
        _lib.ptr(val_k), _lib.ptr(tag_k), _lib.ptr(ind_k), n, k, m, num_tags, order_c, float(vis_thr), float(tag_thr),
        int(bool(ignore_too_much)), int(bool(use_rounded_norm)), _lib.ptr(people), _lib.ptr(meta[0]), _lib.ptr(meta[1]), _lib.ptr(ws),
        ws_bytes, _lib.stream()), "mp_bottomup_match_by_tag")
    return people, meta[0], meta[1]


def host_match_of(val_k: torch.Tensor, tag_k: torch.Tensor, ind_k: torch.Tensor, joint_order: Sequence[int], **kwargs
                  ) -> Callable[[int], np.ndarray]:
    """``host_match(i)``: the host ``match_by_tag`` of image i of a device batch alone (three small downloads), for the rare image
    the grouping kernel hands over; raises what the host function raises."""
    order = [int(j) for j in joint_order]
    return lambda i: match_by_tag(val_k[i].cpu().numpy(), tag_k[i].cpu().numpy(), ind_k[i].cpu().numpy(), order, **kwargs)


def _meta_of(counts: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
    """[2, N] int32 (counts, status) for ONE download: the tensor the two are rows of (``match_by_tag_device``'s), else a stack."""
    base = counts._base
    if base is not None and base is status._base and base.dim() == 2 and base.shape[0] == 2 and base.is_contiguous() \
            and counts.data_ptr() == base.data_ptr() and status.data_ptr() == base[1].data_ptr() and counts.shape == base.shape[1:]:
        return base
    return torch.stack((counts, status))


_FINISH_BUFFERS: Dict = {}  # (device, N, K, M, L) -> scores, workspace, workspace bytes


def _finish_buffers(device, n, k, m, num_tags):
    key = (device, n, k, m, num_tags)
    if key not in _FINISH_BUFFERS:
        if len(_FINISH_BUFFERS) >= 8:  # as _batch_buffers
            _FINISH_BUFFERS.clear()
        ws_bytes = _lib.load().mp_bottomup_finish_workspace_bytes(n, k, m, num_tags)
        _FINISH_BUFFERS[key] = (torch.empty(n, k * m, device=device, dtype=torch.float32),
                                torch.empty((ws_bytes + 7) // 8, device=device, dtype=torch.int64), ws_bytes)
    return _FINISH_BUFFERS[key]


def _require_device(t, name, dtype):
    """An in / out operand of the entry: it is never copied, so it must already be a contiguous CUDA tensor of ``dtype``."""
    if not t.is_cuda:
        raise _lib.MindposeHipError(f"{name} must be a CUDA tensor: the HIP path has no CPU fallback")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor, got {t.dtype}, contiguous = {t.is_contiguous()}")
    return t


def finish_people_batch(people: torch.Tensor, counts: torch.Tensor, status: torch.Tensor, heatmap: torch.Tensor, tagging: torch.Tensor,
                        refine: bool, host_match: Callable[[int], np.ndarray]) -> Tuple[List[np.ndarray], List[List[np.float32]]]:
    """The tail of a bottom-up batch on the persons ``match_by_tag_device`` left on the device: per-person score (mean joint value)
    and, with ``refine``, the missing-joint refinement against ``heatmap`` [N, K, H, W] and ``tagging`` [N, K or 1, H, W, L] (CUDA,
    the decoder's maps), through ``mp_bottomup_finish_people`` (two launches sized from the capacity K * M; ``people`` is updated
    in place).  The host reads nothing before the launches and makes exactly TWO downloads behind them: ``counts`` with ``status``
    in one copy, then ``people[:, :top]`` and ``scores[:, :top]`` packed into ONE buffer on the device (a ``torch.cat`` of
    [N, top, K * (3 + L)] and [N, top, 1]) - none when no image has a person.  Returns ``(keypoints, scores)`` as
    ``BottomUpHeatMapAEInferencer._parse`` does: N float32 arrays [P_i, K, 3 + L] (the host function's empty array for an image
    without persons) and N lists of ``np.float32``, bit-equal to the host path.  An image with ``status[i] != 0`` is grouped by
    ``host_match(i)`` (``host_match_of``); its scores are the host expression and its refinement the inferencer's
    ``_refine_on_device`` on that image alone, so the maps stay on the device."""
    for t, name in ((people, "people"), (counts, "counts"), (status, "status"), (heatmap, "heatmap"), (tagging, "tagging")):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a torch.Tensor")
    if people.dim() != 4 or heatmap.dim() != 4 or tagging.dim() != 5:
        raise ValueError(f"expected people [N, K * M, K, 3 + L], heatmap [N, K, H, W], tagging [N, K or 1, H, W, L], got "
                         f"{tuple(people.shape)}, {tuple(heatmap.shape)}, {tuple(tagging.shape)}")
    n, groups, k, width = people.shape
    num_tags = width - 3
    if k == 0 or groups == 0 or groups % k != 0 or num_tags < 1 or counts.shape != (n,) or status.shape != (n,) or heatmap.shape[:2] != (n, k) \
            or tagging.shape[0] != n or tagging.shape[1] not in (1, k) or tagging.shape[2:4] != heatmap.shape[2:] or tagging.shape[4] != num_tags:
        raise ValueError(f"expected people [N, K * M, K, 3 + L], counts [N], status [N], heatmap [N, K, H, W], tagging [N, K or 1, H, W, L], "
                         f"got {tuple(people.shape)}, {tuple(counts.shape)}, {tuple(status.shape)}, {tuple(heatmap.shape)}, "
                         f"{tuple(tagging.shape)}")
    people = _require_device(people, "people", torch.float32)
    counts, status = _require_device(counts, "counts", torch.int32), _require_device(status, "status", torch.int32)
    heatmap, tagging = _lib.require_cuda_f32(heatmap, "heatmap"), _lib.require_cuda_f32(tagging, "tagging")
    if n == 0:
        return [], []
    m, (h, w) = groups // k, heatmap.shape[2:]
    if not match_on_device_supported(k, m, num_tags):
        raise _lib.MindposeHipError(f"finish_people_batch carries K <= 64, M <= 64, L <= 4 and K * M <= 1024, got K = {k}, M = {m}, "
                                    f"L = {num_tags}")
    scores, ws, ws_bytes = _finish_buffers(people.device, n, k, m, num_tags)
    _lib.check(_lib.load().mp_bottomup_finish_people(
        _lib.ptr(people), _lib.ptr(counts), _lib.ptr(status), _lib.ptr(heatmap), _lib.ptr(tagging), n, k, m, h, w,
        int(tagging.shape[1] > 1 or k == 1), num_tags, int(bool(refine)), _lib.ptr(scores), _lib.ptr(ws), ws_bytes, _lib.stream()),
        "mp_bottomup_finish_people")
    counts_host, status_host = _meta_of(counts, status).cpu().numpy()
    counts_host = np.where(status_host == 0, np.clip(counts_host, 0, groups), 0)
    top = int(counts_host.max())
    packed = torch.cat((people[:, :top].reshape(n, top, k * width), scores[:, :top, None]), dim=2).cpu().numpy() if top else None
    keypoints, out_scores = [], []
    for i in range(n):
        if status_host[i] != 0:  # rare: the host function, then the host path's own tail for this image alone
            persons = host_match(i)
            out_scores.append([person[:, 2].mean() for person in persons])
            if refine:
                from ..engine.inferencer.bottomup_inferencer import BottomUpHeatMapAEInferencer  # (imports this module)
                BottomUpHeatMapAEInferencer._refine_on_device([persons], heatmap[i:i + 1], tagging[i:i + 1])
            keypoints.append(persons)
        elif counts_host[i] == 0:
            keypoints.append(np.array([]).astype(np.float32))  # the host function's empty result
            out_scores.append([])
        else:
            rows = packed[i, :counts_host[i]]
            keypoints.append(np.ascontiguousarray(rows[:, :k * width]).reshape(-1, k, width))
            out_scores.append(list(rows[:, k * width]))
    return keypoints, out_scores
