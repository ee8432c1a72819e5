"""Gradient clipping by global norm, the parts that need no GPU: the recipe keys ``clip_grad`` / ``clip_value`` and their refusals,
``clip_norm`` through ``create_optimizer`` for every registered optimizer, the definition of the coefficient at its edges, and the
block layouts and exports of the C ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

from mindpose_amd import _lib
from mindpose_amd.cli.config import parse_args
from mindpose_amd.cli.train import grad_clip_norm
from mindpose_amd.utils import create_optimizer
from mindpose_amd.utils.adamw import CLIP_RESOLVED_DTYPE, CLIP_STATE_DTYPE, check_clip_norm, clip_coefficient
from mindpose_amd.utils.optim_factory import _OPTIMIZERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = os.path.join(ROOT, "tests", "golden", "recipes", "hrnet_w32_ascend.yaml")


def _args(*options):
    return parse_args(["--config", RECIPE] + (["--cfg-options", *options] if options else []))


def test_recipe_keys_default_off():
    args = _args()
    assert not hasattr(args, "clip_grad") and not hasattr(args, "clip_value")  # no recipe of the reference has the keys
    assert grad_clip_norm(args) is None
    assert grad_clip_norm(_args("clip_value=2.0")) is None  # the value alone switches nothing on
    assert grad_clip_norm(_args("clip_grad=False", "clip_value=2.0")) is None


def test_cfg_options_reach_the_keys():
    assert grad_clip_norm(_args("clip_grad=True")) == 15.0  # mindcv's default
    assert grad_clip_norm(_args("clip_grad=True", "clip_value=1.0")) == 1.0
    assert grad_clip_norm(_args("clip_grad=True", "clip_value=3")) == 3.0 and isinstance(grad_clip_norm(_args("clip_grad=True", "clip_value=3")), float)
    assert grad_clip_norm(_args("clip_grad:True", "clip_value:0.5")) == 0.5
    assert grad_clip_norm(_args("clip_grad=True", "clip_value=inf")) == math.inf  # measure only
    assert grad_clip_norm(_args("clip_grad=True", "clip_value=1e-3")) == 1e-3


@pytest.mark.parametrize("value", ["0", "0.0", "-1.0", "nan", "fifteen", "None", "True", "[1.0]", "-inf"])
@pytest.mark.parametrize("clip_grad", ["True", "False"])
def test_bad_clip_value_is_refused(value, clip_grad):
    with pytest.raises(ValueError, match="clip_value"):
        grad_clip_norm(_args(f"clip_grad={clip_grad}", f"clip_value={value}"))


def test_bad_clip_grad_is_refused():
    for value in ("1", "yes", "2.0"):
        with pytest.raises(ValueError, match="clip_grad"):
            grad_clip_norm(_args(f"clip_grad={value}"))


def test_bad_clip_value_is_refused_before_anything_is_opened(monkeypatch):
    """``train`` checks the keys first: nothing is seeded, no device or dataset is touched"""
    from mindpose_amd.cli import train as train_mod

    def fail(*a, **k):
        raise AssertionError("train() went on past a bad clip_value")

    for name in ("init_distributed", "create_dataset", "create_pipeline"):
        monkeypatch.setattr(train_mod, name, fail)
    with pytest.raises(ValueError, match="clip_value"):
        train_mod.train(_args("clip_grad=True", "clip_value=0"))


def test_check_clip_norm():
    assert check_clip_norm(None) is None and check_clip_norm(2) == 2.0 and check_clip_norm(math.inf) == math.inf
    assert check_clip_norm(np.float32(0.5)) == 0.5 and check_clip_norm(5e-324) == 5e-324
    for bad in (0, 0.0, -0.0, -1, -math.inf, math.nan, "1.0", True, [1.0]):
        with pytest.raises(ValueError, match="clip_norm"):
            check_clip_norm(bad)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(5, 3))
        self.bias = torch.nn.Parameter(torch.ones(7))


@pytest.mark.parametrize("name", sorted(_OPTIMIZERS))
def test_create_optimizer_forwards_clip_norm(name):
    extra = dict(momentum=0.9) if name.lower() == "momentum" else {}
    lib = _lib.load()
    opt = create_optimizer(_Net(), name=name, learning_rate=1e-3, weight_decay=0.1, overlap=False, clip_norm=2.5, **extra)
    try:
        assert opt.clip_norm == 2.5 and opt.clip_coef == 1.0
        assert opt._clip_partials.dtype == torch.float64 and opt._clip_partials.numel() == lib.mp_grad_norm_partials(opt._grad_flat.numel()) == 1
        assert opt._clip_state.numel() == CLIP_STATE_DTYPE.itemsize and opt._clip_resolved.numel() == CLIP_RESOLVED_DTYPE.itemsize
        assert opt.grad_clip_stats() == dict(last_norm=0.0, mean_norm=0.0, max_norm=0.0, measured_steps=0, clipped_steps=0)
    finally:
        opt.close()
    off = create_optimizer(_Net(), name=name, learning_rate=1e-3, overlap=False, **extra)
    try:
        assert off.clip_norm is None and not hasattr(off, "_clip_partials") and not hasattr(off, "_clip_state")
        with pytest.raises(ValueError, match="clipping is off"):
            off.grad_clip_stats()
        off.reset_grad_clip_stats()  # nothing to clear
    finally:
        off.close()
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="clip_norm"):
            create_optimizer(_Net(), name=name, learning_rate=1e-3, overlap=False, clip_norm=bad, **extra)
    inf = create_optimizer(_Net(), name=name, learning_rate=1e-3, overlap=False, clip_norm=math.inf, **extra)
    assert inf.clip_norm == math.inf
    inf.close()


def test_coefficient_at_its_edges():
    assert clip_coefficient(2.0, 2.0) == 1.0                       # norm == clip_norm: not clipped
    assert clip_coefficient(math.nextafter(2.0, 3.0), 2.0) < 1.0   # one ulp above: clipped, and the quotient is below 1
    assert clip_coefficient(4.0, 2.0) == 0.5
    assert clip_coefficient(1.0, 2.0) == 1.0 and clip_coefficient(0.0, 2.0) == 1.0
    assert clip_coefficient(math.inf, 2.0) == 1.0 and clip_coefficient(math.nan, 2.0) == 1.0  # a non-finite norm never clips
    assert clip_coefficient(1e300, math.inf) == 1.0 and clip_coefficient(math.inf, math.inf) == 1.0  # measure only
    base = 1.0 / 3.0 / 1024.0
    assert np.float32(base * clip_coefficient(1.0, 2.0)) == np.float32(base)  # unclipped: the scale itself, bit for bit


def test_partials_count_is_a_function_of_the_count_alone():
    lib = _lib.load()
    for count, want in ((0, 0), (1, 1), (3, 1), (4, 1), (4096, 1), (4099, 1), (4100, 2), (5003, 2), (2048 * 4096, 2048), (2048 * 4096 + 7, 2048),
                        (28_535_552, 2048), (2 ** 33 + 5, 2048)):
        assert lib.mp_grad_norm_partials(count) == want, count


def test_abi_layouts_and_refusals():
    header = open(os.path.join(ROOT, "include", "mindpose_hip.h")).read()
    for name in ("mp_grad_norm_partials", "mp_grad_finite_norm", "mp_train_tail_advance_clip", "mp_grad_clip_resolve"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTED_SYMBOLS, name
    assert CLIP_STATE_DTYPE.itemsize == 40 and CLIP_STATE_DTYPE.names == ("last_norm", "norm_sum", "norm_max", "measured_steps", "clipped_steps")
    assert CLIP_RESOLVED_DTYPE.itemsize == 24 and CLIP_RESOLVED_DTYPE.fields["norm"][1] == 8 and CLIP_RESOLVED_DTYPE.fields["coef"][1] == 16
    body = header[header.index("typedef struct mp_grad_clip_state"):header.index("} mp_grad_clip_state;")]
    assert re.findall(r"\b(?:double|int64_t)\s+(\w+);", body) == list(CLIP_STATE_DTYPE.names)
    lib = _lib.load()  # argument validation happens before any HIP call
    assert lib.mp_grad_finite_norm(None, 4, None, None, None) == -1
    assert lib.mp_grad_clip_resolve(None, None, 1, 1.0, 1.0, 1.0, 1.0, None, None, None) == -1
    assert lib.mp_train_tail_advance_clip(None, None, 2.0, 1, 1.0, 1.0, None, 1, None, 0, None, None, None, 0, 1.0, None, None) == -1
