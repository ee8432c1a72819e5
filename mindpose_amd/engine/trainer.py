"""The training loop that ``mindspore.Model.train(num_epochs, dataset, callbacks, dataset_sink_mode=True)`` runs in the reference
(tools/train.py:176-233): epochs over the pipeline, every step the graph-captured forward / backward plus the optimizer tail
(``utils/graph_step.py``), the callback's hooks after each step and each epoch.

With ``resident`` (the default, ``MINDPOSE_TRAIN_RESIDENT=0`` switches it off) the step tail runs from device state
(``utils/step_tail.py``): the host reads nothing back per step and keeps at most two steps queued ahead of the device; the
loss-scale manager and ``optimizer.global_step`` are brought up to date at each epoch end, before the callbacks look at them.

With gradient clipping (the optimizer's ``clip_norm``) the epoch end also reads the device's gradient-norm statistics once, logs
them and hands them to the callbacks whose ``on_train_epoch_end`` takes a ``grad_norm`` keyword.
"""
import inspect
import logging
from typing import Iterable, Optional

import torch

from .. import _lib
from ..utils.graph_step import GraphedTrainStep

__all__ = ["Trainer"]

QUEUED_STEPS = 2  # steps the host may run ahead of the device

_logger = logging.getLogger(__name__)


def _takes_keyword(fn, name: str) -> bool:
    params = inspect.signature(fn).parameters
    return name in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


class Trainer:
    def __init__(self, net_with_loss: torch.nn.Module, optimizer, loss_scale_manager=None, resident: Optional[bool] = None) -> None:
        """``optimizer``: an arena optimizer built with ``overlap=False`` (``create_optimizer(..., overlap=False)``);
        ``resident``: None reads ``MINDPOSE_TRAIN_RESIDENT`` (default on)."""
        if optimizer.grads.overlap:
            raise ValueError("build the optimizer with overlap=False: the trainer runs the graph-captured step")
        self.nwl, self.opt, self.mgr = net_with_loss, optimizer, loss_scale_manager
        self.resident = _lib.env_on("MINDPOSE_TRAIN_RESIDENT") if resident is None else bool(resident)
        self.step: Optional[GraphedTrainStep] = None

    def last_lr(self) -> float:
        """The learning rate of the last applied update (the base rate before any)."""
        schedule = self.opt._schedule
        if schedule is None or self.opt.global_step == 0:
            return float(self.opt.lr)
        return float(schedule(self.opt.global_step - 1))

    def train(self, num_epochs: int, dataset, callbacks: Iterable = ()) -> None:
        """``dataset``: a pipeline of ``create_pipeline(is_train=True)``; its final columns are the positional inputs of
        ``NetWithLoss``.  The pipeline is closed on the way out, also on an exception."""
        callbacks = list(callbacks)
        total_steps = max(1, int(num_epochs) * int(dataset.get_dataset_size()))
        self.nwl.train()
        try:
            inflight = []  # one event per queued step, oldest first
            for epoch in range(1, int(num_epochs) + 1):
                for batch in dataset:
                    inputs = tuple(batch.values())
                    if self.step is None:  # static shapes: captured once, from the first batch
                        self.step = GraphedTrainStep(self.nwl, self.opt, inputs, loss_scale_manager=self.mgr,
                                                     resident=self.resident, total_steps=total_steps)
                    loss = self.step(*inputs)
                    for cb in callbacks:
                        cb.on_train_step_end(loss)
                    ev = torch.cuda.Event()
                    ev.record()
                    inflight.append(ev)
                    if len(inflight) > QUEUED_STEPS:
                        inflight.pop(0).synchronize()  # step t - 2: its input copies and meter updates are done with
                if self.step is not None:
                    self.step.sync()
                lr = self.last_lr()
                extra = {}
                metric = getattr(self.nwl, "metric", None)
                if metric is not None:  # the epoch's one read of the accuracy state; callbacks without the keyword see no change
                    extra["train_metrics"] = metric.compute()
                    metric.reset()
                grad_norm = None
                if self.opt.clip_norm is not None:  # the epoch's one read of the clip state, then a new period
                    grad_norm = self.opt.grad_clip_stats()
                    self.opt.reset_grad_clip_stats()
                    _logger.info(f"epoch = {epoch}, gradient norm: mean = {grad_norm['mean_norm']:.6g}, max = {grad_norm['max_norm']:.6g}, "
                                 f"clipped {grad_norm['clipped_steps']} of {grad_norm['measured_steps']} steps "
                                 f"(clip_norm = {self.opt.clip_norm:g})")
                for cb in callbacks:
                    more = {"grad_norm": grad_norm} if grad_norm is not None and _takes_keyword(cb.on_train_epoch_end, "grad_norm") else {}
                    cb.on_train_epoch_end(epoch, getattr(self.nwl, "net", self.nwl), lr, **extra, **more)
        finally:
            if hasattr(dataset, "close"):
                dataset.close()
