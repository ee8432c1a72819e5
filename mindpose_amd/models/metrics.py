"""Training-time pose accuracy: the PCK of the output heat maps against the target heat maps that the HRNet training code and the
legacy mmpose API print beside the loss (``accuracy()`` of lib/core/evaluate.py, restated; the reference has no counterpart).

The metric runs as two launches (``mp_pose_pck_accuracy``, csrc/pose_metric.hip) on the heat maps a training step already holds,
accumulates in a device state block and is read once per epoch: nothing comes back to the host per step, so the launches can be
part of the captured step (``NetWithLoss(metric=...)``).  The exact definition is in include/mindpose_hip.h and DESIGN.md.
"""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib

__all__ = ["PoseAccuracy", "pose_pck_accuracy"]

STATE_HEAD_DTYPE = np.dtype([("steps", "<i8"), ("sum_cnt", "<i8"), ("sum_acc_cnt", "<f8"), ("last_avg_acc", "<f8"),
                             ("last_cnt", "<i8"), ("pad", "<i8")])  # mp_pose_pck_state; int64 hits[K], valid[K] follow


def state_bytes(num_joints: int) -> int:
    return STATE_HEAD_DTYPE.itemsize + 16 * int(num_joints)


def parse_state(raw: np.ndarray, num_joints: int) -> Tuple[np.void, np.ndarray, np.ndarray]:
    """(header, hits [K], valid [K]) of a downloaded state block."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    head = raw[:STATE_HEAD_DTYPE.itemsize].view(STATE_HEAD_DTYPE)[0]
    counts = raw[STATE_HEAD_DTYPE.itemsize:state_bytes(num_joints)].view("<i8")
    return head, counts[:num_joints].copy(), counts[num_joints:].copy()


class PoseAccuracy:
    def __init__(self, thr: float = 0.5) -> None:
        self.thr = float(thr)
        self._state: Optional[torch.Tensor] = None  # uint8 [48 + 16 K]
        self._flags: Optional[torch.Tensor] = None  # uint8 [N * K]: launch 1's valid / hit bits
        self._k = 0
        self._captured = False  # a captured graph holds the buffers' addresses: they are never replaced after that

    def _fit(self, n: int, k: int, device: torch.device) -> None:
        """State and flags for [n, k, ., .] maps on ``device``: allocated on first use or when the shape outgrows them - never
        while a stream capture is active, and never again once an ``update`` has been captured (the graph replays its launches
        on the addresses it was recorded with)."""
        fits_state = self._state is not None and self._k == k and self._state.device == device
        fits_flags = self._flags is not None and self._flags.numel() >= n * k and self._flags.device == device
        capturing = torch.cuda.is_current_stream_capturing()
        if not (fits_state and fits_flags):
            if capturing:
                raise RuntimeError(f"PoseAccuracy.update inside a stream capture with buffers that do not fit [{n}, {k}] maps: run "
                                   "one eager update with the step's shapes before capturing (GraphedTrainStep's warm-up passes do)")
            if self._captured:
                raise RuntimeError(f"PoseAccuracy.update with [{n}, {k}] maps that do not fit the buffers a captured graph holds "
                                   f"({self._flags.numel()} pairs, {self._k} joints): use another PoseAccuracy for another shape")
            if not fits_state:  # another joint count: a new epoch state
                self._state = torch.zeros(state_bytes(k), device=device, dtype=torch.uint8)
                self._k = k
            if not fits_flags:
                self._flags = torch.empty(n * k, device=device, dtype=torch.uint8)
        self._captured |= capturing

    def update(self, output: torch.Tensor, target: torch.Tensor) -> None:
        """Two launches on the current stream; no host read."""
        output, target = _lib.require_cuda_f32(output, "output"), _lib.require_cuda_f32(target, "target")
        if output.dim() != 4 or output.shape != target.shape:
            raise ValueError(f"output and target must be [N, K, H, W] heat maps of one shape, got {tuple(output.shape)} and "
                             f"{tuple(target.shape)}")
        n, k, h, w = output.shape
        self._fit(n, k, output.device)
        _lib.check(_lib.load().mp_pose_pck_accuracy(_lib.ptr(output), _lib.ptr(target), n, k, h, w, self.thr, self._flags.data_ptr(),
                                                    self._state.data_ptr(), _lib.stream()), "mp_pose_pck_accuracy")

    def reset(self) -> None:
        """Asynchronous memset of the state block."""
        if self._state is not None:
            self._state.zero_()

    def _read(self):
        if self._state is None:
            return np.zeros(1, dtype=STATE_HEAD_DTYPE)[0], np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        return parse_state(self._state.cpu().numpy(), self._k)  # the one synchronising download

    def compute(self) -> Dict[str, object]:
        """The epoch so far, one synchronising read: ``acc`` = sum(avg_acc * cnt) / sum(cnt) (0 when nothing counted), ``count`` =
        sum(cnt), ``steps``, per-joint ``hits`` and ``valid``; ``sum_acc_cnt`` is the numerator as accumulated."""
        head, hits, valid = self._read()
        count = int(head["sum_cnt"])
        sum_acc_cnt = float(head["sum_acc_cnt"])
        return dict(acc=sum_acc_cnt / count if count > 0 else 0.0, count=count, steps=int(head["steps"]),
                    hits=[int(v) for v in hits], valid=[int(v) for v in valid], sum_acc_cnt=sum_acc_cnt)

    def sums(self) -> Tuple[float, int, List[int], List[int]]:
        """The raw ``(sum_acc_cnt, sum_cnt, hits, valid)``: what is added across ranks before the division."""
        head, hits, valid = self._read()
        return float(head["sum_acc_cnt"]), int(head["sum_cnt"]), [int(v) for v in hits], [int(v) for v in valid]

    def last(self) -> Tuple[float, int]:
        """``(avg_acc, cnt)`` of the last update (synchronises; tests and tools)."""
        head, _, _ = self._read()
        return float(head["last_avg_acc"]), int(head["last_cnt"])


def pose_pck_accuracy(output: torch.Tensor, target: torch.Tensor, thr: float = 0.5) -> Tuple[np.ndarray, float, int]:
    """The eager one-off on CUDA tensors: ``(acc [K] float64, -1 where no pair of the joint is valid; avg_acc; cnt)``."""
    metric = PoseAccuracy(thr)
    metric.update(output, target)
    head, hits, valid = metric._read()
    acc = np.full(hits.shape, -1.0, dtype=np.float64)
    counted = valid > 0
    acc[counted] = hits[counted].astype(np.float64) / valid[counted].astype(np.float64)
    return acc, float(head["last_avg_acc"]), int(head["last_cnt"])
