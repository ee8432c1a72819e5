#!/usr/bin/env python3
"""Host-driven against device-resident step tail (utils/step_tail.py) on the amp-O2 HRNet-W32 training step at the benchmark's
shape (N = 128, 256 x 192): both forms are built side by side from the same synthetic initialisation and timed in ALTERNATED rounds
(so clock and thermal drift hit both alike), wall time per step with one synchronise per round; median and min - max over the
rounds.  The reference point is the host-driven step of the same run.
   python tools/bench_train_tail.py [--batch 128] [--rounds 7] [--steps 30] [--form both|host|resident] [--json out.json]
``--form host`` / ``resident`` runs one form alone (for a kernel trace: tools/timeline.py --marker gaussian_target shows the gap
between a step's last update launch and the next step's first kernel)."""
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


def build(resident, batch, total_steps, dev):
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(dev).train()
    mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.create_network_with_loss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True)
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
    step = GraphedTrainStep(nwl, opt, (image, t0, w0), loss_scale_manager=DynamicLossScaleManager(), resident=resident,
                            total_steps=total_steps)

    def run(steps):
        for _ in range(steps):
            target, weight = tgt(kp)  # as the benchmark's step: the targets are made on the device every step
            step(image, target, weight)

    return run, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--form", choices=["both", "host", "resident"], default="both")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    total = a.warmup + a.rounds * a.steps
    forms = {"host": False, "resident": True} if a.form == "both" else {a.form: a.form == "resident"}
    runs = {name: build(resident, a.batch, total, dev)[0] for name, resident in forms.items()}
    for run in runs.values():
        run(a.warmup)
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    out = {"batch": a.batch, "rounds": a.rounds, "steps_per_round": a.steps}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v,
                     "img_per_s": a.batch * 1e3 / statistics.median(v)}
    if len(ms) == 2:
        out["resident_over_host"] = out["resident"]["median_ms"] / out["host"]["median_ms"]
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
