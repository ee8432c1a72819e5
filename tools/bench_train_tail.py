#!/usr/bin/env python3
"""Host-driven against device-resident step tail (utils/step_tail.py) on the amp-O2 HRNet-W32 training step at the benchmark's
shape (N = 128, 256 x 192): both forms are built side by side from the same synthetic initialisation and timed in ALTERNATED rounds
(so clock and thermal drift hit both alike), wall time per step with one synchronise per round; median and min - max over the
rounds.  The reference point is the host-driven step of the same run.
   python tools/bench_train_tail.py [--part both|step|update] [--batch 128] [--rounds 7] [--steps 30] [--form both|host|resident] [--json out.json]
``--form host`` / ``resident`` runs one form alone (for a kernel trace: tools/timeline.py --marker gaussian_target shows the gap
between a step's last update launch and the next step's first kernel).
``--part update`` times the update launches alone (csrc/step_end.hip): ``mp_adamw_step_scaled`` and ``mp_adamw_step_resident`` on
arenas of HRNet-W32's size (parameters, gradients and two moments: 456 MB, larger than the Infinity Cache), device events around
each launch, the two alternated within every round; median and min - max over the rounds' medians, in microseconds."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.utils import AdamWeightDecay, DynamicLossScaleManager, GraphedTrainStep  # noqa: E402
from mindpose_amd.utils.step_tail import ARGS_DTYPE  # noqa: E402


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


def bench_update(a, dev):
    lib, stream = _lib.load(), _lib.stream()
    count = sum(p.numel() for p in mp.create_network("hrnet_w32", "hrnet_head").parameters() if p.requires_grad)
    gen = torch.Generator(device="cpu").manual_seed(7)
    p, g, m = (torch.randn(count, generator=gen).to(dev) for _ in range(3))
    v = torch.rand(count, generator=gen).to(dev)
    block = np.zeros(1, dtype=ARGS_DTYPE)
    block["grad_scale"], block["lr"] = 0.125, 1e-6
    block = torch.from_numpy(block.view(np.uint8)).to(dev)
    arenas = [t.data_ptr() for t in (p, g, m, v)]
    forms = {
        "mp_adamw_step_scaled": lambda: lib.mp_adamw_step_scaled(*arenas, count, 1e-6, 0.9, 0.999, 1e-6, 0.05, 0.125, None, stream),
        "mp_adamw_step_resident": lambda: lib.mp_adamw_step_resident(*arenas, count, 0.9, 0.999, 1e-6, 0.05, block.data_ptr(), stream),
    }
    us = {name: [] for name in forms}
    for r in range(a.rounds + 2):  # two warm-up rounds
        for name, fn in forms.items():
            per = []
            for _ in range(a.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(fn(), name)
                e1.record()
                e1.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3)
            if r >= 2:
                us[name].append(statistics.median(per))
    out = {"count": count, "launches_per_round": a.launches}
    for name, t in us.items():
        out[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["both", "step", "update"], default="both")
    ap.add_argument("--launches", type=int, default=20, help="update part: launches per entry and round")
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
    if a.part == "update":
        forms = {}
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
    if a.part != "step":
        out["update"] = bench_update(a, dev)
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
