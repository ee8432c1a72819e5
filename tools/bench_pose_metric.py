#!/usr/bin/env python3
"""What the training-time accuracy metric (models/metrics.py, csrc/pose_metric.hip) costs on the amp-O2 HRNet-W32 training step at
the benchmark's shape (N = 128, 256 x 192).  The steps named by ``--order`` are built side by side from the same synthetic
initialisation (tools/bench_train_tail.py's resident step), in that order, and timed in ALTERNATED rounds, wall time per step with
one synchronise per round; median and min - max over the rounds:
   off, off2   the step without the metric - the baseline; off2 is a second, identical one: two steps of one process differ by their
               place in the build order alone, and off2 - off says by how much
   on          the metric's two launches on the step's stream, between network and loss

The two launches alone are timed with device events over back-to-back updates, once on one pair of [N, 17, 64, 48] tensors (the
maps come from the Infinity Cache after the first call) and once rotating over enough pairs to exceed it (the maps come from HBM);
bytes = 2 maps x N x 17 x 64 x 48 x 4, the rate is quoted against the 8 TB/s of the data sheet.
   python tools/bench_pose_metric.py [--batch 128] [--rounds 7] [--steps 30] [--order off,on,off2] [--no-launches] [--json out.json]
``--order on --no-launches`` runs one form alone for a kernel trace of the step (tools/timeline.py --marker gaussian_target);
``--order none`` only times the launches."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mindpose_amd as mp  # noqa: E402
from mindpose_amd.utils import AdamWeightDecay, DynamicLossScaleManager, GraphedTrainStep  # noqa: E402

CACHE_BYTES = 256 << 20  # Infinity Cache


def build(with_metric, batch, total_steps, dev):
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(dev).train()
    mp.models.auto_mixed_precision(net, "O2")
    metric = mp.PoseAccuracy() if with_metric else None
    nwl = mp.NetWithLoss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True, metric=metric)
    opt = AdamWeightDecay(net, lr=1e-3, weight_decay=0.05, filter_bias_and_bn=True, overlap=False)
    tgt = mp.TopDownGenerateTarget(config=dict(image_size=[192, 256], heatmap_size=[48, 64]), sigma=2.0)
    gen = torch.Generator(device="cpu").manual_seed(1000)
    image = torch.randn(batch, 3, 256, 192, generator=gen).to(dev)
    kp = torch.empty(batch, 17, 3)
    kp[..., 0] = torch.rand(batch, 17, generator=gen) * 232 - 20
    kp[..., 1] = torch.rand(batch, 17, generator=gen) * 296 - 20
    kp[..., 2] = (torch.rand(batch, 17, generator=gen) < 0.7).float()
    kp = kp.to(dev)
    t0, w0 = tgt(kp)
    step = GraphedTrainStep(nwl, opt, (image, t0, w0), loss_scale_manager=DynamicLossScaleManager(), resident=True,
                            total_steps=total_steps)

    def run(steps):
        for _ in range(steps):
            target, weight = tgt(kp)  # as the benchmark's step: the targets are made on the device every step
            step(image, target, weight)

    return run, metric


def time_launches(batch, dev, calls=200):
    """Device time of one update (both launches), microseconds: maps in the Infinity Cache / maps from HBM."""
    shape = (batch, 17, 64, 48)
    pair_bytes = 2 * batch * 17 * 64 * 48 * 4
    pairs = CACHE_BYTES // pair_bytes + 2
    gen = torch.Generator(device="cpu").manual_seed(7)
    data = [(torch.randn(shape, generator=gen).to(dev), torch.rand(shape, generator=gen).to(dev)) for _ in range(pairs)]
    metric = mp.PoseAccuracy()
    out = {"bytes": pair_bytes, "pairs_rotated": pairs}
    for name, rotate in (("cache_us", False), ("hbm_us", True)):
        for i in range(pairs):  # warm up: code objects, the metric's buffers
            metric.update(*data[i])
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(calls):
            metric.update(*data[i % pairs if rotate else 0])
        end.record()
        torch.cuda.synchronize()
        out[name] = start.elapsed_time(end) * 1e3 / calls
        out[name.replace("_us", "_fraction_of_8TBps")] = pair_bytes / (out[name] * 1e-6) / 8e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--order", default="off,on,off2", help="comma list of off, on, off2 (or none): the steps to build and time, in "
                    "this order")
    ap.add_argument("--no-launches", action="store_true", help="skip the launch timing (a kernel trace of the step alone)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    total = a.warmup + a.rounds * a.steps
    forms = {} if a.order == "none" else {name: name == "on" for name in a.order.split(",")}
    if not set(forms) <= {"off", "on", "off2"}:
        ap.error(f"--order {a.order}: names are off, on, off2")
    built = {name: build(with_metric, a.batch, total, dev) for name, with_metric in forms.items()}
    for run, _ in built.values():
        run(a.warmup)
    torch.cuda.synchronize()
    ms = {name: [] for name in built}
    for _ in range(a.rounds):
        for name, (run, _) in built.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    out = {"batch": a.batch, "rounds": a.rounds, "steps_per_round": a.steps}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v,
                     "img_per_s": a.batch * 1e3 / statistics.median(v)}
    if "off" in ms:  # against the baseline (or the mean of the two baselines)
        base = statistics.mean(out[name]["median_ms"] for name in ("off", "off2") if name in ms)
        out["baseline_spread_ms"] = out["off"]["max_ms"] - out["off"]["min_ms"]
        for name in ("on", "off2"):
            if name in ms:
                out[f"{name}_minus_baseline_ms"] = out[name]["median_ms"] - (out["off"]["median_ms"] if name == "off2" else base)
    if "on" in built:
        out["accuracy"] = {k: v for k, v in built["on"][1].compute().items() if k in ("acc", "count", "steps")}
    if not a.no_launches:
        out["launches"] = time_launches(a.batch, dev)
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
