"""The graph-captured step with the device-resident tail against the host-driven one, and the recipe runner end to end
(mindpose_amd/cli/train.py, cli/eval.py) on a synthetic COCO folder.  All comparisons are bit for bit: both forms run the same
captured graphs and the same update arithmetic."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd.utils import AdamWeightDecay, DynamicLossScaleManager, GraphedTrainStep, load_checkpoint  # noqa: E402

DEV = torch.device("cuda:0")
RECIPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recipes", "hrnet_w32_ascend.yaml")


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- graphed step ----------------------------------------------------------------------------------------------------------------------
def _batches(n=4, steps=6, bad=2):
    g = torch.Generator().manual_seed(3)
    tgt = mp.TopDownGenerateTarget(config=dict(image_size=[192, 256], heatmap_size=[48, 64]), sigma=2.0)
    out = []
    for it in range(steps):
        x = torch.randn(n, 3, 256, 192, generator=g)
        if it == bad:
            x[1, 2, 100, 50] = float("inf")  # this step overflows: its update is skipped and the loss scale halves
        kp = torch.rand(n, 17, 3, generator=g) * torch.tensor([192.0, 256.0, 2.0])
        target, weight = tgt(kp.to(DEV))
        out.append((x.to(DEV), target, weight))
    return out


def _run_steps(resident, batches, monkeypatch):
    torch.manual_seed(0)
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(DEV).train()
    mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.create_network_with_loss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True)
    opt = AdamWeightDecay(net, lr=1e-3, weight_decay=0.05, filter_bias_and_bn=True, overlap=False)
    mgr = DynamicLossScaleManager(2.0 ** 12, 2.0, 2)  # grows on clean steps, halves on the planted overflow
    step = GraphedTrainStep(nwl, opt, batches[0], loss_scale_manager=mgr, resident=resident, total_steps=len(batches))
    reads = [0]
    real_item, real_cpu = torch.Tensor.item, torch.Tensor.cpu

    def item(self):
        reads[0] += 1
        return real_item(self)

    def cpu(self, *a, **k):
        reads[0] += 1
        return real_cpu(self, *a, **k)

    losses = []
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "item", item)
        m.setattr(torch.Tensor, "cpu", cpu)
        for b in batches:
            losses.append(step(*b).detach().clone())  # stays on the device
        reads_in_loop = reads[0]
    step.sync()
    torch.cuda.synchronize()
    out = dict(flat=opt.flat.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), losses=torch.stack(losses), reads=reads_in_loop,
               mgr=(mgr.loss_scale, mgr.cur_iter, mgr.last_overflow_iter, mgr.skipped_steps), global_step=opt.global_step)
    opt.close()
    return out


def test_resident_graphed_step_equals_the_host_driven_one(monkeypatch):
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")
    batches = _batches()
    host = _run_steps(False, batches, monkeypatch)
    res = _run_steps(True, batches, monkeypatch)
    # the planted overflow was skipped (the loss scale may have cost further steps: both forms must agree on them)
    assert host["mgr"][3] >= 1 and host["mgr"][2] >= 2 and host["global_step"] == len(batches) - host["mgr"][3] > 0, host["mgr"]
    assert host["reads"] >= len(batches)  # the host-driven step reads its flag back every step (the wrapper sees it)
    assert res["reads"] == 0, f"{res['reads']} host read(s) between the first and the last resident step"
    assert _same_bits(host["losses"], res["losses"]), (host["losses"], res["losses"])
    for key in ("flat", "m", "v"):
        assert _same_bits(host[key], res[key]), key
    assert res["mgr"] == host["mgr"] and res["global_step"] == host["global_step"]


# ---- the recipe runner, end to end ---------------------------------------------------------------------------------------------------------
def _coco_folder(root, n_img, seed, name):
    """Synthetic COCO key-point folder as tests/test_gpu_loader.py builds it: arrays saved under .jpg names."""
    rng = np.random.RandomState(seed)
    os.makedirs(root, exist_ok=True)
    images, anns = [], []
    for i in range(n_img):
        h = 120 + 8 * i
        with open(os.path.join(root, f"{i}.jpg"), "wb") as f:
            np.save(f, rng.randint(0, 256, (h, 160, 3)).astype(np.uint8))
        images.append(dict(id=i + 1, file_name=f"{i}.jpg", width=160, height=h))
        kp = np.concatenate([rng.uniform(20, 100, (17, 2)), rng.randint(1, 3, (17, 1))], axis=1)
        anns.append(dict(id=i + 1, image_id=i + 1, category_id=1, iscrowd=0, bbox=[15.0, 12.0, 100.0, 90.0], area=9000.0,
                         num_keypoints=17, keypoints=kp.reshape(-1).tolist()))
    path = os.path.join(root, name)
    with open(path, "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=1, name="person")]), f)
    return path


def _argv(data, outdir, ckpt=None):
    argv = ["--config", RECIPE, "--outdir", outdir]
    if ckpt:
        argv += ["--ckpt", ckpt]
    return argv + ["--cfg-options", "batch_size=4", "num_epochs=2", "warmup=1", "lr_scheduler_setting.milestones=[2]",
                   "backbone_pretrained=False", "val_interval=1", "num_parallel_workers=1", f"train_root={data['train_root']}",
                   f"train_label={data['train_label']}", f"val_root={data['val_root']}", f"val_label={data['val_label']}"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The synthetic COCO folders: 9 training images, 5 validation images."""
    tmp = str(tmp_path_factory.mktemp("runner"))
    out = dict(tmp=tmp, train_root=os.path.join(tmp, "train"), val_root=os.path.join(tmp, "val"))
    out["train_label"] = _coco_folder(out["train_root"], 9, 5, "train.json")
    out["val_label"] = _coco_folder(out["val_root"], 5, 6, "val.json")
    return out


@pytest.fixture(scope="module")
def runs(data):
    """One resident training run, one host-driven one and one evaluation of the first run's checkpoint, shared by the tests."""
    from mindpose_amd.cli.config import parse_args
    from mindpose_amd.cli.eval import eval as run_eval
    from mindpose_amd.cli.train import train
    tmp = data["tmp"]
    saved = {k: os.environ.get(k) for k in ("MINDPOSE_AUTOTUNE", "MINDPOSE_TRAIN_RESIDENT")}
    os.environ["MINDPOSE_AUTOTUNE"] = "0"
    try:
        out = {}
        for name, resident in (("resident", "1"), ("host", "0")):
            os.environ["MINDPOSE_TRAIN_RESIDENT"] = resident
            out[name] = os.path.join(tmp, name)
            train(parse_args(_argv(data, out[name])))
        ckpt = os.path.join(out["resident"], "saved_model", "hrnet_w32_ascend_last.ckpt")
        out["eval"] = run_eval(parse_args(_argv(data, os.path.join(tmp, "eval"), ckpt), need_ckpt=True))
        out["eval_dir"] = os.path.join(tmp, "eval")
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def _summary(outdir):
    with open(os.path.join(outdir, "summary", "summary.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_runner_summary(runs):
    from mindpose_amd.utils.lr import WarmupMultiStepDecayLR
    recs = _summary(runs["resident"])
    assert [r["epoch"] for r in recs] == [1, 2] and [r["step"] for r in recs] == [2, 4]  # 9 images, batch 4, drop_remainder
    schedule = WarmupMultiStepDecayLR(1e-3, 2, 2, [2], warmup=1)
    stats = ["AP", "AP .5", "AP .75", "AP (M)", "AP (L)", "AR", "AR .5", "AR .75", "AR (M)", "AR (L)"]
    for r in recs:
        assert np.isfinite(r["train/loss"]), r
        vals = [k for k in r if k.startswith("val/")]
        assert len(vals) == 10 and sorted(vals) == sorted("val/" + s for s in stats), vals
        # the learning rate of the last applied update: at most step - 1, earlier when updates were skipped for overflow
        assert r["train/lr"] in [float(schedule(i)) for i in range(r["step"])], r
    host = _summary(runs["host"])
    assert host == recs  # the host-driven run logs the same losses, rates and statistics


def test_runner_checkpoint_loads_back_name_for_name(runs):
    ckpt = load_checkpoint(os.path.join(runs["resident"], "saved_model", "hrnet_w32_ascend_last.ckpt"))
    net = mp.create_network("hrnet_w32", "hrnet_head")
    own = net.state_dict()
    assert sorted(ckpt) == sorted(own)
    assert all(tuple(ckpt[k].shape) == tuple(own[k].shape) for k in own)
    assert os.path.exists(os.path.join(runs["resident"], "saved_model", "hrnet_w32_ascend_best.ckpt")) or \
        _summary(runs["resident"])[-1]["val/AP"] == 0.0  # best.ckpt is written when some epoch's AP beats 0


def test_runner_eval_gives_the_callbacks_ap(runs):
    assert runs["eval"]["AP"] == _summary(runs["resident"])[-1]["val/AP"]
    with open(os.path.join(runs["eval_dir"], "result.json")) as f:
        assert json.load(f) == {k: float(v) for k, v in runs["eval"].items()}


def test_runner_host_driven_run_writes_the_same_checkpoint(runs):
    a, b = (load_checkpoint(os.path.join(runs[k], "saved_model", "hrnet_w32_ascend_last.ckpt")) for k in ("resident", "host"))
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_runner_refuses_bottomup_training_and_a_missing_pretrained_file(data):
    from mindpose_amd.cli.config import parse_args
    from mindpose_amd.cli.train import train
    higher = os.path.join(os.path.dirname(RECIPE), "higher_hrnet_w32_ascend.yaml")
    with pytest.raises(ValueError, match="bottom-up training data is not implemented"):
        train(parse_args(["--config", higher, "--outdir", os.path.join(data["tmp"], "bu")]))
    argv = [a for a in _argv(data, os.path.join(data["tmp"], "pre")) if a != "backbone_pretrained=False"]  # the recipe's True, and its URL
    with pytest.raises(FileNotFoundError, match="pretrained weights"):
        train(parse_args(argv))
