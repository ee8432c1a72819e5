"""``cli/eval --cfg-options ema=True`` on the GPU: a checkpoint that holds an exponential moving average of the weights under
``ema.<name>`` beside the live weights is evaluated on the average - the network it loads gives, bit for bit, the heat maps of a
network that holds the averaged weights under the plain names (and the file's BatchNorm statistics, which both sets share) - and on
the live weights without the key; a file without the entries is refused."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd.cli import eval as eval_mod  # noqa: E402
from mindpose_amd.cli.config import parse_args  # noqa: E402
from mindpose_amd.utils import load_checkpoint, save_checkpoint  # noqa: E402
from mindpose_amd.utils.ckpt import ema_parameters  # noqa: E402

DEV = torch.device("cuda:0")


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """both.ckpt: a synthetic network's state and, under ``ema.<name>``, the trained parameters of a second one (another seed);
    moved.ckpt: the second one's parameters under the plain names with the first one's statistics; plain.ckpt: the first alone."""
    tmp = str(tmp_path_factory.mktemp("eval_ema"))
    live = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0)
    other = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=1)
    state = {k: v.detach().cpu().numpy() for k, v in live.state_dict().items()}
    names = [k for k, _ in live.named_parameters()]
    both = dict(state)
    both.update({"ema." + k: v.detach().cpu().numpy() for k, v in other.named_parameters()})
    out = dict(tmp=tmp, names=names, **{k: os.path.join(tmp, k + ".ckpt") for k in ("both", "moved", "plain")})
    save_checkpoint(both, out["both"])
    save_checkpoint(ema_parameters(both), out["moved"])
    save_checkpoint(state, out["plain"])
    return out


def _heatmaps(ckpt, ema):
    net = mp.create_network("hrnet_w32", "hrnet_head").to(DEV)
    assert eval_mod.load_weights(net, ckpt, ema) == []
    net.eval()
    x = torch.randn(2, 3, 256, 192, generator=torch.Generator().manual_seed(4)).to(DEV)
    out = net(x).clone()
    torch.cuda.synchronize()
    return net, out


def test_the_loaded_network_is_the_network_of_the_averaged_weights(files, monkeypatch):
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")  # every network records the same plan
    state = load_checkpoint(files["both"])
    assert sorted(k[len("ema."):] for k in state if k.startswith("ema.")) == sorted(files["names"])
    net, avg = _heatmaps(files["both"], True)
    for name, p in net.named_parameters():
        assert p.detach().cpu().numpy().tobytes() == state["ema." + name].tobytes(), name
    for name, b in net.named_buffers():
        if name in state:
            assert np.array_equal(b.detach().cpu().numpy(), state[name]), f"{name}: the statistics are the file's own"
    _, moved = _heatmaps(files["moved"], False)
    _, live = _heatmaps(files["both"], False)
    _, plain = _heatmaps(files["plain"], False)
    assert _same_bits(avg, moved), "with the key: not the network of the averaged weights"
    assert _same_bits(live, plain), "without the key: not the network of the live weights"
    assert not _same_bits(avg, live) and torch.isfinite(avg).all() and torch.isfinite(live).all()
    with pytest.raises(ValueError, match="no `ema.` entries"):
        _heatmaps(files["plain"], True)


def test_cli_eval_with_and_without_the_key(files, monkeypatch):
    """the recipe runner's evaluation on the synthetic COCO folder of tests/test_gpu_trainer.py"""
    from tests.test_gpu_trainer import _argv, _coco_folder
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")
    tmp = files["tmp"]
    data = dict(train_root=os.path.join(tmp, "val"), val_root=os.path.join(tmp, "val"))
    data["val_label"] = data["train_label"] = _coco_folder(data["val_root"], 5, 6, "val.json")
    loads, real_load = [], eval_mod.load_weights

    def load_weights(net, ckpt, ema):
        loads.append((os.path.basename(ckpt), ema))
        return real_load(net, ckpt, ema)

    monkeypatch.setattr(eval_mod, "load_weights", load_weights)

    def run(name, ckpt, *options):
        argv = _argv(data, os.path.join(tmp, name), ckpt) + ["amp_level=O0", *options]
        return eval_mod.eval(parse_args(argv, need_ckpt=True))

    avg, moved = run("avg", files["both"], "ema=True"), run("moved", files["moved"])
    live, plain = run("live", files["both"]), run("plain", files["plain"], "ema=False")
    assert loads == [("both.ckpt", True), ("moved.ckpt", False), ("both.ckpt", False), ("plain.ckpt", False)]
    assert len(avg) == 10 and avg == moved, "with the key: not the result of the averaged weights"
    assert live == plain, "without the key: not the result of the live weights"
    with pytest.raises(ValueError, match="no `ema.` entries"):
        run("refused", files["plain"], "ema=True")
