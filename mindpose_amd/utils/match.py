"""Associative-embedding grouping (reference: mindpose/utils/match.py:15-116), host numpy.

Joints are visited in ``joint_order``; the detections of a joint above ``vis_thr`` are assigned to the existing person groups by
the Hungarian algorithm on the L2 distance between their tag and each group's mean tag (rounded to integers with
``use_rounded_norm``), through ``scipy.optimize.linear_sum_assignment`` - the reference's own solver.  With rounded costs the
matrix is full of ties and another solver could return another optimum, so it is not replaced.  A detection without a match
closer than ``tag_thr`` opens a new group keyed by its first tag value (a later detection with the same key overwrites that
group, as the reference's dict does).

``match_by_tag_batch`` is the same function for the N images of a decoder output on the device: ONE launch of
``mp_bottomup_match_by_tag`` (bottomup_match.hip, one wave per image), which restates scipy's solver - tie order included - and
numpy's float32 reductions, so its arrays are bit-equal to the host function's.
"""
import ctypes
from typing import Dict, List, Sequence

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
                       tag_thr: float = 1, ignore_too_much: bool = False, use_rounded_norm: bool = True) -> List[np.ndarray]:
    """``match_by_tag`` of every image of val_k [N, K, M], tag_k [N, K, M, L], ind_k [N, K, M, 2] (CUDA fp32, the decoder's
    outputs) in one launch on the current stream -> N arrays [P_i, K, 3 + L], each bit-equal to ``match_by_tag`` of that image.
    Two downloads: the person counts with the status words, then the persons up to the largest count.  An image whose visible
    detections carry a NaN or infinite tag is grouped by the host function (which raises what scipy raises)."""
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
        return []
    if not match_on_device_supported(k, m, num_tags):
        raise _lib.MindposeHipError(f"match_by_tag_batch carries K <= 64, M <= 64, L <= 4 and K * M <= 1024, got K = {k}, M = {m}, "
                                    f"L = {num_tags}")
    people, meta, ws, ws_bytes = _batch_buffers(val_k.device, n, k, m, num_tags)
    order_c = (ctypes.c_int * k)(*[int(j) for j in order])
    _lib.check(_lib.load().mp_bottomup_match_by_tag(
        _lib.ptr(val_k), _lib.ptr(tag_k), _lib.ptr(ind_k), n, k, m, num_tags, order_c, float(vis_thr), float(tag_thr),
        int(bool(ignore_too_much)), int(bool(use_rounded_norm)), _lib.ptr(people), _lib.ptr(meta[0]), _lib.ptr(meta[1]), _lib.ptr(ws),
        ws_bytes, _lib.stream()), "mp_bottomup_match_by_tag")
    counts, status = meta.cpu().numpy()
    counts = np.where(status == 0, counts, 0)  # (the kernel reports 0 persons for an image it hands over; not relied upon)
    top = int(counts.max())
    persons = people[:, :top].cpu().numpy() if top else None  # None: every image is empty or handed over - never indexed below
    out = []
    for i in range(n):
        if status[i] != 0:  # rare: three small downloads of this image alone
            out.append(match_by_tag(val_k[i].cpu().numpy(), tag_k[i].cpu().numpy(), ind_k[i].cpu().numpy(), [int(j) for j in order],
                                    vis_thr=vis_thr, tag_thr=tag_thr, ignore_too_much=ignore_too_much, use_rounded_norm=use_rounded_norm))
        elif counts[i] == 0:
            out.append(np.array([]).astype(np.float32))  # the host function's empty result
        else:
            out.append(persons[i, :counts[i]].copy())
    return out
