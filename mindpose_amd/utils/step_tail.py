"""The step tail - overflow check, loss-scale update, skip decision, learning-rate lookup, parameter update - without a host
read-back: what ``_ArenaOptimizer.step`` decides on the host from ``self._overflow.item()`` is decided on the device by one
single-workgroup launch (``mp_train_tail_advance``, csrc/step_end.hip), and the update launches read their step-dependent
arguments from the block it fills.  The host may therefore queue step t+1 before step t has run - the loop that
``mindspore.Model.train(..., dataset_sink_mode=True)`` runs on the device (tools/train.py:233).

The tables are the very values the host path passes per step: ``np.float32(float(schedule(i)))`` is what ``ctypes.c_float`` makes
of ``float(self.lr)``, ``np.float32(beta ** (i + 1))`` what it makes of ``Adam._hyper()``'s bias-correction powers.
"""
from typing import Callable, Optional, Union

import numpy as np
import torch

from .. import _lib

STATE_DTYPE = np.dtype([("loss_scale", "<f8"), ("cur_iter", "<i8"), ("last_overflow_iter", "<i8"), ("skipped_steps", "<i8"),
                        ("applied_steps", "<i8")])  # mp_train_tail_state (include/mindpose_hip.h)
ARGS_DTYPE = np.dtype([("skip", "<i4"), ("grad_scale", "<f4"), ("lr", "<f4"), ("aux0", "<f4"), ("aux1", "<f4"),
                       ("first_step", "<f4")])  # mp_step_args


def lr_table(learning_rate: Union[float, Callable[[int], float]], total_steps: int) -> np.ndarray:
    """fp32 learning rate per applied update; a constant gives one entry (the device clamps the index to the last one)."""
    if not callable(learning_rate):
        return np.array([np.float32(float(learning_rate))], dtype=np.float32)
    if total_steps < 1:
        raise ValueError(f"total_steps must be >= 1 for a scheduled learning rate, got {total_steps}")
    return np.array([np.float32(float(learning_rate(i))) for i in range(total_steps)], dtype=np.float32)


def adam_aux_table(beta1: float, beta2: float, total_steps: int) -> np.ndarray:
    """[T][2] fp32: ``beta1 ** t``, ``beta2 ** t`` for t = i + 1 (``Adam._hyper()`` at ``global_step == i``)."""
    if total_steps < 1:
        raise ValueError(f"total_steps must be >= 1, got {total_steps}")
    return np.array([[np.float32(beta1 ** (i + 1)), np.float32(beta2 ** (i + 1))] for i in range(total_steps)], dtype=np.float32)


class ResidentStepTail:
    def __init__(self, optimizer, loss_scale_manager=None, total_steps: int = 1, scale_out: Optional[torch.Tensor] = None) -> None:
        """``optimizer``: an arena optimizer of utils/adamw.py (a ``create_optimizer`` one brings its schedule); ``total_steps``:
        the length of the run - of the learning-rate table of a schedule and of Adam's bias-correction table;
        ``scale_out``: the fp32 device scalar a captured step multiplies its loss by (``GraphedTrainStep.scale_t``), kept equal to
        the loss scale after every step.  The state starts from the manager's and the optimizer's current counters."""
        self.opt, self.mgr, self.scale_out = optimizer, loss_scale_manager, scale_out
        dev = optimizer.flat.device
        self.lr_host = lr_table(optimizer._schedule if optimizer._schedule is not None else optimizer.lr, total_steps)
        self.lr_dev = torch.from_numpy(self.lr_host).to(dev)
        self.aux_dev = None
        if optimizer.kind == 1:
            self.aux_dev = torch.from_numpy(adam_aux_table(optimizer.beta1, optimizer.beta2, total_steps)).to(dev)
        self.static_loss_scale = float(optimizer.loss_scale)
        self.state_dev = torch.zeros(STATE_DTYPE.itemsize, device=dev, dtype=torch.uint8)
        self.args_dev = torch.zeros(ARGS_DTYPE.itemsize, device=dev, dtype=torch.uint8)
        self.upload()

    def upload(self) -> None:
        """Device state := the manager's fields and ``optimizer.global_step`` (the inverse of ``sync``)."""
        st = np.zeros(1, dtype=STATE_DTYPE)
        mgr = self.mgr
        st["loss_scale"] = mgr.loss_scale if mgr is not None else 1.0
        st["cur_iter"] = mgr.cur_iter if mgr is not None else self.opt.global_step
        st["last_overflow_iter"] = mgr.last_overflow_iter if mgr is not None else -1
        st["skipped_steps"] = mgr.skipped_steps if mgr is not None else 0
        st["applied_steps"] = self.opt.global_step
        self.state_dev.copy_(torch.from_numpy(st.view(np.uint8)))
        if self.scale_out is not None and mgr is not None:
            self.scale_out.fill_(mgr.loss_scale)

    def launch(self) -> None:
        """Check (with a manager or clipping), advance, one update launch per non-empty decay group; no host read.  With the
        optimizer's ``clip_norm`` the check also sums the squares and the advance launch decides the clip coefficient; without a
        manager that pass runs for the norm alone and its flag is not handed on (never skip)."""
        lib = _lib.load()
        opt, mgr, stream = self.opt, self.mgr, _lib.stream()
        flag = opt.launch_check(lib, mgr is not None, stream)
        args = (flag, self.state_dev.data_ptr(), mgr.scale_factor if mgr is not None else 1.0, mgr.scale_window if mgr is not None else 1,
                float(opt.grads.mean_scale), self.static_loss_scale, self.lr_dev.data_ptr(), self.lr_dev.numel(),
                self.aux_dev.data_ptr() if self.aux_dev is not None else None, self.aux_dev.shape[0] if self.aux_dev is not None else 0,
                self.args_dev.data_ptr(), self.scale_out.data_ptr() if (self.scale_out is not None and mgr is not None) else None)
        if opt.clip_norm is not None:
            _lib.check(lib.mp_train_tail_advance_clip(*args, opt._clip_partials.data_ptr(), opt._clip_partials.numel(), opt.clip_norm,
                                                      opt._clip_state.data_ptr(), stream), "mp_train_tail_advance_clip")
        else:
            _lib.check(lib.mp_train_tail_advance(*args, stream), "mp_train_tail_advance")
        opt.launch_updates(lib, stream, self.args_dev.data_ptr())

    def read_state(self) -> np.ndarray:
        """One download of the state block (synchronises with the stream)."""
        return self.state_dev.cpu().numpy().view(STATE_DTYPE)[0]

    def read_args(self) -> np.ndarray:
        """The step-arguments block of the last launch (tests and tools; synchronises)."""
        return self.args_dev.cpu().numpy().view(ARGS_DTYPE)[0]

    def sync(self) -> None:
        """One download: the device's counters into the manager and ``optimizer.global_step``."""
        st = self.read_state()
        if self.mgr is not None:
            self.mgr.loss_scale = float(st["loss_scale"])
            self.mgr.cur_iter = int(st["cur_iter"])
            self.mgr.last_overflow_iter = int(st["last_overflow_iter"])
            self.mgr.skipped_steps = int(st["skipped_steps"])
        self.opt.global_step = int(st["applied_steps"])

