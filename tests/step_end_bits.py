"""The output bits of the update entries of csrc/step_end.hip, as digests: what tests/golden/gen_step_end_golden.py records from the
library of the commit a change to those kernels starts from, and what tests/test_gpu_step_end_bits.py recomputes and compares.

Entries and rules: ``mp_adamw_step``; ``mp_adamw_step_scaled`` without a skip flag, with ``*skip == 0`` and with ``*skip == 1``;
``mp_adamw_step_resident`` with ``skip`` 0 and 1; ``mp_optimizer_step`` and ``mp_optimizer_step_resident`` for each of
``glue_matrix.OPT_VARIANTS``.  Counts: ``glue_matrix.OPT_COUNTS`` (the last crosses the grid cap with a ragged end).  Inputs:
four consecutive runs of ``glue_matrix.pattern_bits`` (finite values of every magnitude, denormals, -0) as parameter, gradient
and the two states; a state whose square root a rule takes is made non-negative.  One more case per entry at count 257 plants
+inf, -inf and NaN in the gradient: its record is the digest of the outputs that are not NaN and the indices of those that are,
so that a NaN payload cannot matter.

The resident entries get the step-dependent values through the step-arguments block, and the launch's own h3 / h4 are zero where
the block overrides them (Adam's beta^t, SGD's first_step); the block's unused fields hold 7.0.
"""
import ctypes
import hashlib

import numpy as np
import torch

from mindpose_amd import _lib
from mindpose_amd.utils.step_tail import ARGS_DTYPE
from tests import glue_matrix as gm

PLANT_COUNT = 257
PLANTS = {5: float("inf"), 100: float("-inf"), 256: float("nan")}
HP = gm.ADAMW_HYPER


def _inputs(count, kind, plant):
    """device tensors (param, grad, state1, state2) of a case; kind 0 is AdamWeightDecay"""
    words = gm.pattern_bits(4 * count, torch.float32)
    p, g, s1, s2 = (words[i * count:(i + 1) * count].clone() for i in range(4))
    s2 = s2.abs()  # AdamWeightDecay's and Adam's v
    if kind == 4:
        s1 = s1.abs()  # Adagrad's accumulator
    if plant:
        for i, v in PLANTS.items():
            g[i] = v
    return [t.cuda() for t in (p, g, s1, s2)]


def _step_args(dev, skip, grad_scale, lr, aux0=7.0, aux1=7.0, first_step=7.0):
    block = np.zeros(1, dtype=ARGS_DTYPE)
    block["skip"], block["grad_scale"], block["lr"] = skip, grad_scale, lr
    block["aux0"], block["aux1"], block["first_step"] = aux0, aux1, first_step
    return torch.from_numpy(block.view(np.uint8)).to(dev)


def _adamw(form):
    def launch(lib, count, t):
        p, g, m, v = (_lib.ptr(x) for x in t)
        betas = HP["b1"], HP["b2"], HP["eps"], HP["wd"]
        if form == "plain":
            return lib.mp_adamw_step(p, g, m, v, count, HP["lr"], *betas, _lib.stream()), None
        if form.startswith("scaled"):
            flag = None if form == "scaled-noflag" else torch.full((1,), int(form[-1]), dtype=torch.int32, device=t[0].device)
            return lib.mp_adamw_step_scaled(p, g, m, v, count, HP["lr"], *betas, gm.OPT_GRAD_SCALE, _lib.ptr(flag) if flag is not None else None,
                                            _lib.stream()), flag
        block = _step_args(t[0].device, int(form[-1]), gm.OPT_GRAD_SCALE, HP["lr"])
        return lib.mp_adamw_step_resident(p, g, m, v, count, *betas, _lib.ptr(block), _lib.stream()), block
    return 0, launch


def _optimizer(name, resident):
    kind, hyper = gm.OPT_VARIANTS[name]

    def launch(lib, count, t):
        p, g = _lib.ptr(t[0]), _lib.ptr(t[1])
        s1 = None if (kind == 2 and hyper[0] == 0.0) else _lib.ptr(t[2])
        s2 = _lib.ptr(t[3]) if kind == 1 else None
        if not resident:
            h = (ctypes.c_float * 5)(*hyper)
            return lib.mp_optimizer_step(kind, p, g, s1, s2, count, gm.OPT_LR, gm.OPT_GRAD_SCALE, gm.OPT_WD, ctypes.byref(h), _lib.stream()), None
        given = list(hyper)
        over = {}
        if kind == 1:
            over, given[3], given[4] = {"aux0": hyper[3], "aux1": hyper[4]}, 0.0, 0.0
        elif kind == 2:
            over, given[3] = {"first_step": hyper[3]}, 0.0
        block = _step_args(t[0].device, 0, gm.OPT_GRAD_SCALE, gm.OPT_LR, **over)
        h = (ctypes.c_float * 5)(*given)
        return lib.mp_optimizer_step_resident(kind, p, g, s1, s2, count, gm.OPT_WD, ctypes.byref(h), _lib.ptr(block), _lib.stream()), block
    return kind, launch


ENTRIES = {"mp_adamw_step": _adamw("plain"), "mp_adamw_step_scaled/no-flag": _adamw("scaled-noflag"),
           "mp_adamw_step_scaled/skip0": _adamw("scaled-skip0"), "mp_adamw_step_scaled/skip1": _adamw("scaled-skip1"),
           "mp_adamw_step_resident/skip0": _adamw("resident-skip0"), "mp_adamw_step_resident/skip1": _adamw("resident-skip1")}
for _name in gm.OPT_VARIANTS:
    ENTRIES[f"mp_optimizer_step/{_name}"] = _optimizer(_name, False)
    ENTRIES[f"mp_optimizer_step_resident/{_name}"] = _optimizer(_name, True)

CASES = [(entry, count, False) for entry in ENTRIES for count in gm.OPT_COUNTS] + [(entry, PLANT_COUNT, True) for entry in ENTRIES]


def case_id(entry, count, plant):
    return f"{entry}/{count}" + ("/nonfinite" if plant else "")


def _sha(a: np.ndarray) -> str:
    return hashlib.sha256(a.tobytes()).hexdigest()


def digest(entry, count, plant):
    """{"param" | "state1" | "state2": record} of one case: a SHA-256 of the output bytes, or {"finite", "nan"} for a planted case"""
    kind, launch = ENTRIES[entry]
    t = _inputs(count, kind, plant)
    rc, keep = launch(_lib.load(), count, t)
    _lib.check(rc, case_id(entry, count, plant))
    torch.cuda.synchronize()
    del keep
    out = {}
    for name, x in zip(("param", "state1", "state2"), (t[0], t[2], t[3])):
        a = x.cpu().numpy()
        if plant:
            nan = np.isnan(a)
            out[name] = {"finite": _sha(a[~nan]), "nan": np.flatnonzero(nan).tolist()}
        else:
            out[name] = _sha(a)
    return out
