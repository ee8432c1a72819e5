"""Checkpoints that hold an exponential moving average (EMA) of the weights under ``ema.<name>`` beside the live weights, the parts
that need no GPU: ``ema_parameters``, ``load_param_into_net(prefer_ema=True)``, ``cli/eval``'s loader and its ``ema`` key."""
import os

import numpy as np
import pytest
import torch

from mindpose_amd.cli import eval as eval_mod
from mindpose_amd.cli.config import parse_args
from mindpose_amd.utils import load_checkpoint, load_param_into_net, save_checkpoint
from mindpose_amd.utils.ckpt import EMA_PREFIX, ema_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = os.path.join(ROOT, "tests", "golden", "recipes", "hrnet_w32_ascend.yaml")
LIVE, AVG = np.arange(6, dtype=np.float32).reshape(2, 3), np.full((2, 3), 7.0, np.float32)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(2, 3))
        self.register_buffer("stat", torch.zeros(()))
        self.invalidated = 0

    def invalidate_plans(self):
        self.invalidated += 1


@pytest.fixture()
def files(tmp_path):
    both, plain = str(tmp_path / "both.ckpt"), str(tmp_path / "plain.ckpt")
    save_checkpoint({"w": LIVE, "stat": np.float32(3.0), "ema.w": AVG, "moment1.w": LIVE}, both)
    save_checkpoint({"w": LIVE, "stat": np.float32(3.0)}, plain)
    return both, plain


def test_ema_parameters_moves_the_average_onto_the_plain_names(files):
    state = load_checkpoint(files[0])
    moved = ema_parameters(state)
    assert EMA_PREFIX == "ema." and list(state) == ["w", "stat", "ema.w", "moment1.w"]
    assert moved.keys() == {"w", "stat", "moment1.w"} and np.array_equal(moved["w"], AVG)
    assert moved["stat"] == 3.0, "what has no averaged twin stays: both sets share the BatchNorm statistics"
    assert np.array_equal(state["w"], LIVE) and "ema.w" in state, "the argument was changed"
    with pytest.raises(ValueError, match="no `ema.` entries"):
        ema_parameters(load_checkpoint(files[1]))
    with pytest.raises(ValueError, match="no `ema.` entries"):
        ema_parameters({})


def test_load_param_into_net_prefers_ema_on_request(files):
    both, plain = files
    net = _Net()
    assert load_param_into_net(net, load_checkpoint(both)) == [] and np.array_equal(net.w.detach().numpy(), LIVE)  # `ema.w`: an unknown name
    assert load_param_into_net(net, load_checkpoint(both), prefer_ema=True) == []
    assert np.array_equal(net.w.detach().numpy(), AVG) and float(net.stat) == 3.0 and net.invalidated == 2
    wrapped = {"network.ema.w": AVG}  # the prefix is looked for where MindSpore puts it: in front of the parameter's own name
    with pytest.raises(ValueError, match="no `ema.` entries"):
        load_param_into_net(net, wrapped, prefer_ema=True)
    bad = {"w": LIVE, "ema.w": np.zeros((3, 2), np.float32)}
    with pytest.raises(RuntimeError, match="same shape"):
        load_param_into_net(net, bad, prefer_ema=True)
    assert load_param_into_net(net, bad) == ["stat"]  # without the request the misshapen average is never looked at
    net = _Net()
    with pytest.raises(ValueError, match="no `ema.` entries"):
        load_param_into_net(net, load_checkpoint(plain), prefer_ema=True)
    assert not net.w.detach().any() and net.invalidated == 0, "a refused load changed the network"


def test_cli_eval_loader(files):
    both, plain = files
    net = _Net()
    assert eval_mod.load_weights(net, both, ema=True) == [] and np.array_equal(net.w.detach().numpy(), AVG)
    assert eval_mod.load_weights(net, both, ema=False) == [] and np.array_equal(net.w.detach().numpy(), LIVE)
    assert eval_mod.load_weights(net, plain, ema=False) == []
    with pytest.raises(ValueError, match="no `ema.` entries"):
        eval_mod.load_weights(net, plain, ema=True)


def _args(*options):
    return parse_args(["--config", RECIPE, "--ckpt", "x.ckpt"] + (["--cfg-options", *options] if options else []), need_ckpt=True)


def test_cli_eval_key(monkeypatch):
    assert not hasattr(_args(), "ema")  # no recipe of the reference has the key
    assert eval_mod.use_ema(_args()) is False and eval_mod.use_ema(_args("ema=False")) is False
    assert eval_mod.use_ema(_args("ema=True")) is True and eval_mod.use_ema(_args("ema:True")) is True

    def fail(*a, **k):
        raise AssertionError("eval() went on past a bad `ema`")

    monkeypatch.setattr(eval_mod, "val_pipeline", fail)
    monkeypatch.setattr(torch.cuda, "current_device", fail)
    for value in ("1", "0", "yes", "0.9999", "None", "[True]"):
        with pytest.raises(ValueError, match="`ema` is True or False"):
            eval_mod.use_ema(_args(f"ema={value}"))
        with pytest.raises(ValueError, match="`ema` is True or False"):
            eval_mod.eval(_args(f"ema={value}"))  # refused before anything is opened


def test_cli_eval_hands_the_key_to_the_loader(monkeypatch):
    seen = []

    class _Stop(Exception):
        pass

    class _Dataset:
        closed = False

        def close(self):
            self.closed = True

    class _Network:
        def to(self, dev):
            return self

    def load(net, ckpt, ema):
        seen.append((ckpt, ema))
        raise _Stop()

    dataset = _Dataset()
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(eval_mod, "val_pipeline", lambda args: dataset)
    monkeypatch.setattr(eval_mod, "network", lambda args, pretrained: _Network())
    monkeypatch.setattr(eval_mod, "load_weights", load)
    for options, want in ((("ema=True",), True), ((), False), (("ema=False",), False)):
        with pytest.raises(_Stop):
            eval_mod.eval(_args(*options))
        assert seen[-1] == ("x.ckpt", want) and dataset.closed


def test_cli_train_refuses_the_key_it_cannot_serve(monkeypatch):
    """training keeps no average yet: `ema=True` is refused before anything is opened, not silently ignored"""
    from mindpose_amd.cli import train as train_mod

    def fail(*a, **k):
        raise AssertionError("train() went on past `ema=True`")

    for name in ("init_distributed", "create_dataset", "create_pipeline"):
        monkeypatch.setattr(train_mod, name, fail)
    args = parse_args(["--config", RECIPE, "--cfg-options", "ema=True"])
    with pytest.raises(ValueError, match="`ema`.*not built yet"):
        train_mod.train(args)
