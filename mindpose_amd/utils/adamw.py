"""Optimizers of the reference's registry (mindpose/optim/optim_factory.py:9-14) on flat fp32 arenas.

"adamw" - what every recipe uses - is mindspore.nn.AdamWeightDecay = Adam WITHOUT bias correction, eps 1e-6, decoupled
weight decay, and - with ``filter_bias_and_bn`` - no decay for parameters whose name ends in beta / gamma / bias (:17-37).
"adam", "sgd", "momentum", "adagrad" follow the update rules MindSpore documents for those cells.

Natively the parameters, their gradients and the optimizer state are flat fp32 arenas ordered [decay | no-decay], so a step
is two launches of one streaming kernel (``mp_adamw_step`` / ``mp_optimizer_step``) regardless of the number of tensors (878
for HRNet-W32).

``clip_norm`` (off by default) clips the gradient by its global norm, MindSpore's ``clip_by_global_norm``: the sum of squares rides
on the overflow check's one read of the arena (``mp_grad_finite_norm``), the coefficient is decided on the device and is one more
factor of the gradient scale the update kernels apply while reading - no pass scales the gradients (include/mindpose_hip.h).
"""
import ctypes
import math
from typing import Dict, Iterable, Iterator, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .grad_allreduce import GradientAverager


def split_decay(named_params: Iterable[Tuple[str, torch.nn.Parameter]], filter_bias_and_bn: bool = True):
    decay, no_decay = [], []
    for name, p in named_params:
        if not p.requires_grad:
            continue
        if filter_bias_and_bn and name.endswith(("beta", "gamma", "bias")):
            no_decay.append(p)
        else:
            decay.append(p)
    return decay, no_decay


CLIP_STATE_DTYPE = np.dtype([("last_norm", "<f8"), ("norm_sum", "<f8"), ("norm_max", "<f8"), ("measured_steps", "<i8"),
                             ("clipped_steps", "<i8")])  # mp_grad_clip_state (include/mindpose_hip.h)
CLIP_RESOLVED_DTYPE = np.dtype([("flag", "<i4"), ("pad", "<i4"), ("norm", "<f8"), ("coef", "<f8")])  # mp_grad_clip_resolved


def check_clip_norm(clip_norm) -> Optional[float]:
    """``None`` (clipping off) or the norm as a float: positive, ``inf`` = measure only.  NaN, zero, negative values and anything
    that is not a number are refused."""
    if clip_norm is None:
        return None
    if isinstance(clip_norm, bool) or not isinstance(clip_norm, (int, float, np.integer, np.floating)):
        raise ValueError(f"clip_norm must be a positive number or inf, got {clip_norm!r}")
    value = float(clip_norm)
    if math.isnan(value) or value <= 0.0:
        raise ValueError(f"clip_norm must be a positive number or inf, got {clip_norm!r}")
    return value


def clip_coefficient(norm: float, clip_norm: float) -> float:
    """The definition in double, as the device states it: ``clip_norm / norm`` when the norm is finite and above ``clip_norm``,
    else exactly 1.0 (no epsilon)."""
    return clip_norm / norm if (math.isfinite(norm) and norm > clip_norm) else 1.0


class _ArenaOptimizer:
    """Parameters, gradients and optimizer state as flat fp32 arenas ordered [decay | no-decay]; ``_update`` of a subclass
    launches its streaming kernel on one group.  ``step`` = gradient mean over ranks (RCCL, overlapped with backward),
    optional dynamic-loss-scale check, update.  The pieces of a step end are stated once here; ``step`` (the decision on the
    host) and ``ResidentStepTail.launch`` (utils/step_tail.py, the decision on the device) put them together."""

    n_states = 2
    kind = 0            # ``kind`` of mp_optimizer_step (0: AdamWeightDecay, which has entries of its own)
    loss_scale = 1.0    # the static scale the MindSpore cells of ``_KernelOptimizer`` divide the gradient by
    time_comm = False   # bench.py's DP leg sets it: ``finish_grads`` records a pair of events around the all-reduce wait
    _schedule = None    # ``create_optimizer`` (utils/optim_factory.py) puts a scheduled learning rate here

    def __init__(self, net: torch.nn.Module, lr: float, weight_decay: float = 0.0, filter_bias_and_bn: bool = True,
                 bucket_mb: float = 32.0, process_group=None, overlap: bool = True, state_init: float = 0.0,
                 transport=None, force_collectives: bool = False, clip_norm: Optional[float] = None) -> None:
        self.clip_norm = check_clip_norm(clip_norm)  # refused before anything is rearranged
        decay, no_decay = split_decay(net.named_parameters(), filter_bias_and_bn)
        self.params = decay + no_decay
        self.n_decay = sum(p.numel() for p in decay)
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        # flat parameter arena: parameters become views (same values, same names)
        self.flat = torch.empty(total, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            n = p.numel()
            self.flat[off:off + n].copy_(p.detach().reshape(-1))
            p.data = self.flat[off:off + n].view_as(p)
            off += n
        self.states = [torch.full_like(self.flat, state_init) for _ in range(self.n_states)]
        self.lr, self.weight_decay = lr, weight_decay
        # gradients: one arena in the SAME order as the parameter arena (no gather before the update), bucketed
        # all-reduce overlapped with backward
        # the 1/world of the gradient mean is folded into the update kernels' gradient scale (mean="consumer"): no extra pass
        self.grads = GradientAverager(self.params, bucket_mb=bucket_mb, process_group=process_group, overlap=overlap,
                                      arena_order="given", mean="consumer", transport=transport,
                                      force_collectives=force_collectives)
        self._grad_flat = self.grads.arena
        self._overflow = torch.zeros(1, device=dev, dtype=torch.int32)  # device flag of the loss-scale overflow check
        self.global_step = 0
        self.comm_events = []
        self.clip_coef = 1.0  # the last step's clip coefficient: the last factor of the gradient scale (exactly 1.0 = none)
        if self.clip_norm is not None:
            n_partials = _lib.load().mp_grad_norm_partials(self._grad_flat.numel())
            self._clip_partials = torch.zeros(n_partials, device=dev, dtype=torch.float64)  # one per workgroup of the fused pass
            self._clip_state = torch.zeros(CLIP_STATE_DTYPE.itemsize, device=dev, dtype=torch.uint8)
            self._clip_resolved = torch.zeros(CLIP_RESOLVED_DTYPE.itemsize, device=dev, dtype=torch.uint8)

    def grad_clip_stats(self) -> Dict[str, float]:
        """One download of the clip-state block (synchronises): the gradient norms of the steps since the last reset that were
        not skipped."""
        if self.clip_norm is None:
            raise ValueError("gradient clipping is off: build the optimizer with clip_norm (inf measures only)")
        st = self._clip_state.cpu().numpy().view(CLIP_STATE_DTYPE)[0]
        n = int(st["measured_steps"])
        return {"last_norm": float(st["last_norm"]), "mean_norm": float(st["norm_sum"]) / n if n else 0.0,
                "max_norm": float(st["norm_max"]), "measured_steps": n, "clipped_steps": int(st["clipped_steps"])}

    def reset_grad_clip_stats(self) -> None:
        if self.clip_norm is not None:
            self._clip_state.zero_()

    def zero_grad(self) -> None:
        self.grads.begin_step()

    def close(self) -> None:
        """Release the gradient averager's hooks and communicator (call before ``destroy_process_group``)."""
        self.grads.close()

    # ---- the pieces of a step end ---------------------------------------------------------------------------------------------

    def finish_grads(self) -> None:
        """The gradients are final: queued (grouped) weight gradients land in the arena before anything reads it, and the
        bucket all-reduces have landed.  With ``time_comm`` (bench.py's DP leg) a pair of events brackets the device time from
        "all gradients are in the arena" to "the all-reduces have landed" as the compute stream sees it (the native transport
        runs them on its own stream; finish() makes this stream wait) - also in a resident step, which calls this too (today
        nothing sets both ``time_comm`` and ``resident``)."""
        from ..models.train_ops import flush_wgrad_jobs
        flush_wgrad_jobs()
        if self.time_comm and self.grads.active and self._grad_flat.is_cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.grads.finish()
            e1.record()
            self.comm_events.append((e0, e1))
        else:
            self.grads.finish()

    def launch_check(self, lib, scaling: bool, stream) -> Optional[int]:
        """The step's one read of the gradient arena before the update (flag zeroed first): with clipping the overflow check and
        the sum of squares as one pass, with loss scaling alone the check, else nothing.  Returns the flag's address for the
        launch that decides the step, or None when nothing may skip it (no loss scaling: a clipping pass then runs for the norm
        alone).  The sums are still scaled: inf / nan survive the scaling, so one read-only pass decides."""
        if self.clip_norm is None and not scaling:
            return None
        self._overflow.zero_()
        grad, flag = self._grad_flat, self._overflow.data_ptr()
        if self.clip_norm is not None:
            _lib.check(lib.mp_grad_finite_norm(grad.data_ptr(), grad.numel(), flag, self._clip_partials.data_ptr(), stream),
                       "mp_grad_finite_norm")
        else:
            _lib.check(lib.mp_grad_finite_check(grad.data_ptr(), grad.numel(), flag, stream), "mp_grad_finite_check")
        return flag if scaling else None

    def groups(self) -> Iterator[Tuple[int, int, float]]:
        """(start, count, weight decay) of the non-empty decay groups."""
        for start, count, wd in ((0, self.n_decay, self.weight_decay), (self.n_decay, self.flat.numel() - self.n_decay, 0.0)):
            if count:
                yield start, count, float(wd)

    def launch_updates(self, lib, stream, step_args: Optional[int] = None) -> None:
        """One update launch per group - lr / gradient scale / skip from the host, or (``step_args``: the address of the device
        step-arguments block of utils/step_tail.py) from the device.  The kernels write the master weights through raw pointers:
        fp16 packings made before are stale."""
        from ..models.train_ops import invalidate_packs
        for start, count, wd in self.groups():
            self._update(lib, start, count, wd, stream, step_args)
        invalidate_packs()

    def _decide(self, lib, flag: Optional[int], mgr) -> bool:
        """The host-driven decision, with the step's single read-back: the resolved block with clipping (a single-workgroup
        launch decides the coefficient with the device code of the resident tail), else the flag, else nothing.  Sets
        ``clip_coef``, advances the manager; returns whether the step applies."""
        overflow = False
        if self.clip_norm is not None:
            _lib.check(lib.mp_grad_clip_resolve(
                flag, self._clip_partials.data_ptr(), self._clip_partials.numel(), float(self.grads.mean_scale), float(mgr.loss_scale) if mgr is not None else 1.0,
                float(self.loss_scale), self.clip_norm, self._clip_state.data_ptr(), self._clip_resolved.data_ptr(), _lib.stream()),
                "mp_grad_clip_resolve")
            resolved = self._clip_resolved.cpu().numpy().view(CLIP_RESOLVED_DTYPE)[0]
            self.clip_coef = float(resolved["coef"])  # multiplies last, in ``_update``
            overflow = int(resolved["flag"]) != 0
        elif flag is not None:
            overflow = int(self._overflow.item()) != 0
        if mgr is not None:
            mgr.update_loss_scale(overflow)
        return not overflow

    def step(self, loss_scale_manager=None) -> bool:
        """All-reduce (mean) the gradients, then one streaming update per decay group.

        With a ``DynamicLossScaleManager`` (amp O2, tools/train.py:170-181) the gradients are first divided by the loss
        scale and checked: on overflow (inf / nan anywhere) the update is skipped and the scale halves, exactly one
        host read-back per step; returns whether the parameters were updated.  With ``clip_norm`` the check also sums the
        squares and a single-workgroup launch decides the clip coefficient: the read-back is its block instead of the flag."""
        lib, mgr = _lib.load(), loss_scale_manager
        self.finish_grads()
        # gradient scale the update kernels apply while reading the arena: 1 / loss_scale (amp O2) x 1 / world (gradient mean)
        self.grad_scale = self.grads.mean_scale
        if mgr is not None:
            self.grad_scale /= mgr.loss_scale
        self.clip_coef = 1.0
        flag = self.launch_check(lib, mgr is not None, _lib.stream())
        if not self._decide(lib, flag, mgr):
            return False
        self.launch_updates(lib, _lib.stream())
        self.global_step += 1
        return True


class AdamWeightDecay(_ArenaOptimizer):
    """mindspore.nn.AdamWeightDecay ("adamw"): Adam without bias correction, eps 1e-6, decoupled weight decay."""

    def __init__(self, net: torch.nn.Module, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-6,
                 weight_decay: float = 0.0, **arena_kwargs) -> None:
        super().__init__(net, lr, weight_decay, **arena_kwargs)
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self.exp_avg, self.exp_avg_sq = self.states

    def _update(self, lib, start, count, wd, stream, step_args=None):
        arenas = [t[start:].data_ptr() for t in (self.flat, self._grad_flat, self.exp_avg, self.exp_avg_sq)]
        betas = float(self.beta1), float(self.beta2), float(self.eps), wd
        if step_args is not None:
            _lib.check(lib.mp_adamw_step_resident(*arenas, count, *betas, step_args, stream), "mp_adamw_step_resident")
        else:
            _lib.check(lib.mp_adamw_step_scaled(*arenas, count, float(self.lr), *betas, float(self.grad_scale) * self.clip_coef, None,
                                                stream), "mp_adamw_step_scaled")


class _KernelOptimizer(_ArenaOptimizer):
    """The reference's other registered optimizers (optim_factory.py:9-14) through ``mp_optimizer_step``.  ``loss_scale`` is
    the static scale those MindSpore cells divide the gradient by; weight decay is their L2 term."""

    def __init__(self, net, lr, weight_decay=0.0, loss_scale: float = 1.0, **arena_kwargs) -> None:
        super().__init__(net, lr, weight_decay, **arena_kwargs)
        self.loss_scale = loss_scale

    def _hyper(self):
        raise NotImplementedError

    def _update(self, lib, start, count, wd, stream, step_args=None):
        """With ``step_args`` the step-dependent entries of ``_hyper()`` - Adam's beta^t, SGD's first_step - are read from the
        block too."""
        hyper = ctypes.byref((ctypes.c_float * 5)(*[float(v) for v in self._hyper()]))
        st = [s_[start:].data_ptr() for s_ in self.states] + [None, None]
        arenas = self.kind, self.flat[start:].data_ptr(), self._grad_flat[start:].data_ptr(), st[0], st[1], count
        if step_args is not None:
            _lib.check(lib.mp_optimizer_step_resident(*arenas, wd, hyper, step_args, stream), "mp_optimizer_step_resident")
        else:
            _lib.check(lib.mp_optimizer_step(*arenas, float(self.lr), float(self.grad_scale) / float(self.loss_scale) * self.clip_coef,
                                             wd, hyper, stream), "mp_optimizer_step")


class Adam(_KernelOptimizer):
    """mindspore.nn.Adam ("adam", the factory's default name): bias-corrected, eps 1e-8 inside the denominator, L2 decay."""

    kind = 1

    def __init__(self, net, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, **kw) -> None:
        super().__init__(net, lr, **kw)
        self.beta1, self.beta2, self.eps = beta1, beta2, eps

    def _hyper(self):
        t = self.global_step + 1
        return self.beta1, self.beta2, self.eps, self.beta1 ** t, self.beta2 ** t


class SGD(_KernelOptimizer):
    """mindspore.nn.SGD ("sgd")."""

    kind, n_states = 2, 1

    def __init__(self, net, lr: float = 0.1, momentum: float = 0.0, dampening: float = 0.0, nesterov: bool = False, **kw) -> None:
        super().__init__(net, lr, **kw)
        self.momentum, self.dampening, self.nesterov = momentum, dampening, nesterov

    def _hyper(self):
        return self.momentum, self.dampening, float(self.nesterov), float(self.global_step == 0), 0.0


class Momentum(_KernelOptimizer):
    """mindspore.nn.Momentum ("momentum")."""

    kind, n_states = 3, 1

    def __init__(self, net, lr: float, momentum: float, use_nesterov: bool = False, **kw) -> None:
        super().__init__(net, lr, **kw)
        self.momentum, self.use_nesterov = momentum, use_nesterov

    def _hyper(self):
        return self.momentum, float(self.use_nesterov), 0.0, 0.0, 0.0


class Adagrad(_KernelOptimizer):
    """mindspore.nn.Adagrad ("adagrad"): accumulator starts at ``accum`` (0.1)."""

    kind, n_states = 4, 1

    def __init__(self, net, lr: float = 1e-3, accum: float = 0.1, **kw) -> None:
        super().__init__(net, lr, state_init=accum, **kw)

    def _hyper(self):
        return 0.0, 0.0, 0.0, 0.0, 0.0
