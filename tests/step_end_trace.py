"""A launch trace of the step end - check, decision, updates - that runs without a device: what `mindpose_amd/utils/adamw.py`
(the host-driven ``step``) and `mindpose_amd/utils/step_tail.py` (``ResidentStepTail.launch``) hand to the C ABI, and the torch ops
around it, for three consecutive step ends.  Built on tests/train_trace.py (``recording()``: host tensors that claim to live on the
device, a recording library, the same pointer normalisation; scalars by value).

``CASES``: {AdamWeightDecay, Adam, SGD with momentum} x {a module with both decay groups, one with the no-decay group only - the
empty group launches nothing} x {host-driven, resident} x {no manager, DynamicLossScaleManager} x {no clipping, clip_norm = 1.0}.

Where a constant answer of the fake library does not fit, it is taught the answer here (the pointers are host addresses):
``mp_grad_norm_partials`` gives 4; ``mp_grad_clip_resolve`` writes its block - the flag it was handed, norm 2.0, coef 0.5 (1.0 on
an overflow); the SECOND check launch of a case raises the overflow flag, so the host-driven step under a manager skips its second
update and runs the third with the halved loss scale (the resident step's decision is the device's: its launches do not change).
"""
import ctypes

import numpy as np
import torch

from mindpose_amd.utils.adamw import CLIP_RESOLVED_DTYPE, SGD, Adam, AdamWeightDecay
from mindpose_amd.utils.loss_scale import DynamicLossScaleManager
from mindpose_amd.utils.step_tail import ResidentStepTail
from tests import train_trace

STEPS = 3


class _Params(torch.nn.Module):
    def __init__(self, shapes):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        for name, shape in shapes.items():
            self.register_parameter(name, torch.nn.Parameter(torch.randn(*shape, generator=g)))


MODULES = {
    "two_groups": {"weight": (5, 3), "scale": (7,), "bias": (5,)},  # "bias" is the no-decay group
    "no_decay_only": {"gamma": (6,), "bias": (6,)},
}
OPTIMIZERS = {
    "adamw": lambda net, **kw: AdamWeightDecay(net, lr=1e-3, weight_decay=0.05, **kw),
    "adam": lambda net, **kw: Adam(net, lr=2e-3, weight_decay=0.01, **kw),
    "sgd_momentum": lambda net, **kw: SGD(net, lr=0.1, momentum=0.9, dampening=0.1, weight_decay=0.01, loss_scale=4.0, **kw),
}


def _answers():
    checks = [0]

    def check(grad, count, flag, *rest):
        checks[0] += 1
        if checks[0] == 2:
            ctypes.c_int.from_address(flag).value = 1
        return 0

    def resolve(flag, partials, n_partials, mean_scale, loss_scale, static_loss_scale, clip_norm, clip_state, resolved, stream):
        raised = ctypes.c_int.from_address(flag).value if flag else 0
        block = (ctypes.c_char * CLIP_RESOLVED_DTYPE.itemsize).from_address(resolved)
        out = np.zeros(1, dtype=CLIP_RESOLVED_DTYPE)
        out["flag"], out["norm"], out["coef"] = raised, 2.0, 1.0 if raised else 0.5
        block[:] = out.tobytes()
        return 0

    return {"mp_grad_norm_partials": lambda count: 4, "mp_grad_finite_check": check, "mp_grad_finite_norm": check,
            "mp_grad_clip_resolve": resolve}


def _case(optimizer, module, resident, manager, clip):
    def run():
        net = _Params(MODULES[module])
        with train_trace.recording(answers=_answers()) as trace:
            opt = OPTIMIZERS[optimizer](net, clip_norm=1.0 if clip else None)
            mgr = DynamicLossScaleManager(init_loss_scale=1024.0, scale_factor=2.0, scale_window=2) if manager else None
            tail = ResidentStepTail(opt, mgr, total_steps=8, scale_out=torch.ones(())) if resident else None
            del trace.events[:]  # the trace is the step ends, not the construction
            trace.empties = 0
            for _ in range(STEPS):
                if tail is not None:
                    tail.launch()
                else:
                    opt.step(loss_scale_manager=mgr)
        return trace
    return run


CASES = {}
for _o in OPTIMIZERS:
    for _m in MODULES:
        for _r in (False, True):
            for _g in (False, True):
                for _c in (False, True):
                    CASES[f"{_o}-{_m}-{'resident' if _r else 'host'}-{'manager' if _g else 'plain'}-{'clip' if _c else 'noclip'}"] = \
                        _case(_o, _m, _r, _g, _c)


def trace_case(name):
    trace = CASES[name]()
    return trace.events, trace.empties


summarise, dump_text = train_trace.summarise, train_trace.dump_text
