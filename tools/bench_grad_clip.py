#!/usr/bin/env python3
"""What gradient clipping by global norm costs; prints ONE JSON line.

   python tools/bench_grad_clip.py [--part kernel|step|both] [--amp O2|O0] [--batch 128] [--rounds 7] [--steps 30] [--json out.json]

- kernel: the fused overflow check + sum of squares (``mp_grad_finite_norm``) beside the plain overflow check
  (``mp_grad_finite_check``) on an arena of HRNet-W32's size (the count is taken from the network).  Device events around each
  launch, the two alternated within every round, median and min - max over the rounds, and the fraction of 8 TB/s each reaches on
  the bytes both read (4 per value).  Every launch reads another of ``--arenas`` copies (default 4, together larger than the
  256 MiB Infinity Cache), so no launch finds its arena in a cache; ``--arenas 1`` shows the cached rate.  The tail launches
  (``mp_train_tail_advance`` / ``mp_train_tail_advance_clip`` on the partials of that count) are timed the same way.
- step: the graphed HRNet-W32 256 x 192 training step at ``--batch`` with the device-resident tail, built four times side by side from
  the same synthetic initialisation - clipping off twice (the difference of two identical runs is the noise floor), ``clip_norm =
  inf`` (measure only) and a finite ``clip_norm`` that clips every step - and timed in alternated rounds, wall time per step with
  one synchronise per round; median and min - max.  ``--amp O0`` is the fp32 step, which without clipping runs no pass over the
  arena at all: its difference is the cost of one arena read.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.utils import DynamicLossScaleManager, GraphedTrainStep, create_optimizer  # noqa: E402

PEAK_BYTES_PER_US = 8e12 / 1e6  # 8 TB/s


def summary(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # microseconds


def bench_kernel(a, dev):
    lib, stream = _lib.load(), _lib.stream()
    count = sum(p.numel() for p in mp.create_network("hrnet_w32", "hrnet_head").parameters() if p.requires_grad)
    gen = torch.Generator(device="cpu").manual_seed(7)
    one = torch.randn(count, generator=gen)
    arenas = [(one * (i + 1)).to(dev) for i in range(a.arenas)]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    n_part = lib.mp_grad_norm_partials(count)
    parts = torch.zeros(n_part, dtype=torch.float64, device=dev)

    def plain(arena):
        _lib.check(lib.mp_grad_finite_check(arena.data_ptr(), count, flag.data_ptr(), stream), "mp_grad_finite_check")

    def fused(arena):
        _lib.check(lib.mp_grad_finite_norm(arena.data_ptr(), count, flag.data_ptr(), parts.data_ptr(), stream), "mp_grad_finite_norm")

    st = torch.zeros(40, dtype=torch.uint8, device=dev)
    st.view(torch.float64)[0] = 1024.0
    args, cs = torch.zeros(24, dtype=torch.uint8, device=dev), torch.zeros(40, dtype=torch.uint8, device=dev)
    lr = torch.tensor([1e-3], dtype=torch.float32, device=dev)
    tail_args = (flag.data_ptr(), st.data_ptr(), 2.0, 2000, 1.0, 1.0, lr.data_ptr(), 1, None, 0, args.data_ptr(), None)

    def tail_plain(_):
        _lib.check(lib.mp_train_tail_advance(*tail_args, stream), "mp_train_tail_advance")

    def tail_clip(_):
        _lib.check(lib.mp_train_tail_advance_clip(*tail_args, parts.data_ptr(), n_part, 1.0, cs.data_ptr(), stream), "mp_train_tail_advance_clip")

    forms = {"finite_check": plain, "finite_norm": fused, "tail_advance": tail_plain, "tail_advance_clip": tail_clip}
    us = {name: [] for name in forms}
    turn = 0
    for r in range(a.rounds + 2):  # two warm-up rounds
        for name, fn in forms.items():
            per = []
            for _ in range(a.launches):
                arena = arenas[turn % len(arenas)]
                turn += 1
                per.append(timed(lambda: fn(arena)))
            if r >= 2:
                us[name].append(statistics.median(per))
    out = {"count": count, "bytes": count * 4, "arenas": a.arenas, "partials": n_part, "launches_per_round": a.launches}
    for name, v in us.items():
        out[name] = {"us": summary(v)}
        if name.startswith("finite"):
            out[name]["fraction_of_8TBps"] = count * 4 / statistics.median(v) / PEAK_BYTES_PER_US
    out["fused_minus_plain_us"] = out["finite_norm"]["us"]["median"] - out["finite_check"]["us"]["median"]
    return out


def build_step(clip_norm, amp, batch, total_steps, dev):
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(dev).train()
    if amp != "O0":
        mp.models.auto_mixed_precision(net, amp)
    nwl = mp.create_network_with_loss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True)
    opt = create_optimizer(net, name="adamw", learning_rate=1e-3, weight_decay=0.05, overlap=False, clip_norm=clip_norm)
    tgt = mp.TopDownGenerateTarget(config=dict(image_size=[192, 256], heatmap_size=[48, 64]), sigma=2.0)
    gen = torch.Generator(device="cpu").manual_seed(1000)
    image = torch.randn(batch, 3, 256, 192, generator=gen).to(dev)
    kp = torch.empty(batch, 17, 3)
    kp[..., 0] = torch.rand(batch, 17, generator=gen) * 232 - 20
    kp[..., 1] = torch.rand(batch, 17, generator=gen) * 296 - 20
    kp[..., 2] = (torch.rand(batch, 17, generator=gen) < 0.7).float()
    kp = kp.to(dev)
    t0, w0 = tgt(kp)
    mgr = DynamicLossScaleManager() if amp != "O0" else None
    step = GraphedTrainStep(nwl, opt, (image, t0, w0), loss_scale_manager=mgr, resident=True, total_steps=total_steps)

    def run(steps):
        for _ in range(steps):
            target, weight = tgt(kp)  # as the benchmark's step: the targets are made on the device every step
            step(image, target, weight)

    return run, opt


def bench_step(a, dev):
    total = a.warmup + a.rounds * a.steps
    forms = {"off_a": None, "off_b": None, "measure_only": math.inf, "clipped": a.clip_norm}
    built = {name: build_step(clip, a.amp, a.batch, total, dev) for name, clip in forms.items()}
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
    out = {"amp": a.amp, "batch": a.batch, "rounds": a.rounds, "steps_per_round": a.steps, "clip_norm": a.clip_norm}
    for name, v in ms.items():
        out[name] = {"ms": summary(v), "rounds_ms": v}
        opt = built[name][1]
        if opt.clip_norm is not None:
            out[name]["grad_norm"] = opt.grad_clip_stats()
    base = out["off_a"]["ms"]["median"]
    out["off_b_minus_off_a_ms"] = out["off_b"]["ms"]["median"] - base
    out["measure_only_minus_off_a_ms"] = out["measure_only"]["ms"]["median"] - base
    out["clipped_minus_off_a_ms"] = out["clipped"]["ms"]["median"] - base
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernel", "step", "both"], default="both")
    ap.add_argument("--amp", choices=["O0", "O2", "O3"], default="O2")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20, help="kernel part: launches per form and round")
    ap.add_argument("--arenas", type=int, default=4, help="kernel part: copies of the arena the launches rotate over")
    ap.add_argument("--clip-norm", type=float, default=1e-3, help="step part: the finite clip_norm (small: every step is clipped)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    if a.part in ("kernel", "both"):
        out["kernel"] = bench_kernel(a, dev)
    if a.part in ("step", "both"):
        out["step"] = bench_step(a, dev)
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
