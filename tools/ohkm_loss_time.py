#!/usr/bin/env python3
"""Device times of the OHKM joint MSE (``joint_ohkm_mse``, csrc/joints_loss.hip) beside the joint MSE at the training shape
(N = 128, K = 17, 64 x 48, topk = 8); prints ONE JSON line.

  python tools/ohkm_loss_time.py [--rounds 7] [--calls 100] [--step-rounds 5] [--step-steps 20] [--json out.json]

Launches.  ``mse_fwd`` / ``mse_bwd`` (``mp_joints_mse_fwd`` / ``_bwd``) and ``ohkm_fwd`` / ``ohkm_bwd`` (``mp_joints_ohkm_fwd`` /
``_bwd``) are timed by device events around ``calls`` back-to-back calls, in ALTERNATED rounds (mse_fwd, ohkm_fwd, mse_bwd, ohkm_bwd,
and again); median and min - max over the rounds, microseconds per call.  Each is timed twice: on one set of tensors (the maps
come from the Infinity Cache after the first call) and rotating over enough sets to exceed it (the maps come from HBM).  Bytes from
the shapes: both forwards read pred and target (2 maps); the MSE backward reads two maps and writes one (3), the OHKM backward
reads two maps of the topk selected rows of K and writes every row: (2 topk / K + 1) maps, 0.65 of the MSE backward's at 8 of 17.

Step.  ``--step-rounds`` > 0 also times the graph-captured amp-O2 HRNet-W32 step at N = 128 (the resident step of
tools/bench_train_tail.py) with either loss, built side by side in one process and timed in alternated rounds, wall time per step
with one synchronise per round.  ``MINDPOSE_AUTOTUNE`` defaults to 0 here (both steps take the library's heuristic picks; set it to 1 for
the tuned step)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models.loss.ohkm import launch_ohkm_fwd  # noqa: E402
from mindpose_amd.utils import AdamWeightDecay, DynamicLossScaleManager, GraphedTrainStep  # noqa: E402

N, K, H, W, TOPK = 128, 17, 64, 48, 8
CACHE_BYTES = 256 << 20  # Infinity Cache
MAP_BYTES = N * K * H * W * 4


def _sets(count, dev):
    gen = torch.Generator(device="cpu").manual_seed(7)
    out = []
    for _ in range(count):
        target = torch.rand(N, K, H, W, generator=gen)
        amp = 0.05 + torch.rand(N, K, 1, 1, generator=gen)
        pred = target + amp * torch.randn(N, K, H, W, generator=gen)
        weight = (torch.rand(N, K, generator=gen) < 0.7).float()
        out.append(dict(pred=pred.to(dev), target=target.to(dev), weight=weight.to(dev), grad=torch.empty(N, K, H, W, device=dev)))
    return out


def _calls(sets, dev):
    """name -> fn(i): one call on set i."""
    lib = _lib.load()
    hw = H * W
    ws_bytes = lib.mp_joints_mse_workspace_bytes(N, K)
    ws = torch.empty(ws_bytes // 4, device=dev)
    loss, go = torch.empty(1, device=dev), torch.ones(1, device=dev)
    for s in sets:  # the selection the OHKM backward reads
        s["sel"] = launch_ohkm_fwd(s["pred"], s["target"], s["weight"], TOPK)[2]
    ows_bytes = lib.mp_joints_ohkm_workspace_bytes(N, K)
    ows = torch.empty(ows_bytes // 8, device=dev, dtype=torch.float64)
    row_sum, sel = torch.empty(N, K, device=dev), torch.empty(N, K, device=dev, dtype=torch.uint8)
    p = _lib.ptr

    def mse_fwd(i):
        s = sets[i]
        _lib.check(lib.mp_joints_mse_fwd(p(s["pred"]), p(s["target"]), p(s["weight"]), p(loss), p(ws), ws_bytes, N, K, hw, _lib.stream()), "mse_fwd")

    def mse_bwd(i):
        s = sets[i]
        _lib.check(lib.mp_joints_mse_bwd(p(s["pred"]), p(s["target"]), p(s["weight"]), p(go), p(s["grad"]), N, K, hw, _lib.stream()), "mse_bwd")

    def ohkm_fwd(i):
        s = sets[i]
        _lib.check(lib.mp_joints_ohkm_fwd(p(s["pred"]), p(s["target"]), p(s["weight"]), p(loss), p(row_sum), p(sel), p(ows), ows_bytes,
                                          N, K, hw, TOPK, _lib.stream()), "ohkm_fwd")

    def ohkm_bwd(i):
        s = sets[i]
        _lib.check(lib.mp_joints_ohkm_bwd(p(s["pred"]), p(s["target"]), p(s["weight"]), p(s["sel"]), p(go), p(s["grad"]), N, K, hw, TOPK,
                                          _lib.stream()), "ohkm_bwd")

    return dict(mse_fwd=mse_fwd, ohkm_fwd=ohkm_fwd, mse_bwd=mse_bwd, ohkm_bwd=ohkm_bwd)


def _stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def time_launches(rounds, calls, dev):
    nbytes = dict(mse_fwd=2 * MAP_BYTES, ohkm_fwd=2 * MAP_BYTES, mse_bwd=3 * MAP_BYTES, ohkm_bwd=int((2 * TOPK / K + 1) * MAP_BYTES))
    count = CACHE_BYTES // (3 * MAP_BYTES) + 2
    sets = _sets(count, dev)
    fns = _calls(sets, dev)
    out = dict(sets_rotated=count, bytes=nbytes)
    for mode, rotate in (("cache", False), ("hbm", True)):
        us = {name: [] for name in fns}
        for fn in fns.values():  # warm up: code objects
            for i in range(count):
                fn(i)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in fns.items():
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for c in range(calls):
                    fn(c % count if rotate else 0)
                end.record()
                end.synchronize()
                us[name].append(start.elapsed_time(end) * 1e3 / calls)
        out[mode + "_us"] = {name: _stats(v) for name, v in us.items()}
        if rotate:
            out["hbm_fraction_of_8TBps"] = {name: round(nbytes[name] / (statistics.median(v) * 1e-6) / 8e12, 3) for name, v in us.items()}
        out[mode + "_ohkm_over_mse"] = {d: round(statistics.median(us["ohkm_" + d]) / statistics.median(us["mse_" + d]), 3) for d in ("fwd", "bwd")}
    return out


def build_step(loss, total_steps, dev):
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0).to(dev).train()
    mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.NetWithLoss(net, loss, has_extra_inputs=True)
    opt = AdamWeightDecay(net, lr=1e-3, weight_decay=0.05, filter_bias_and_bn=True, overlap=False)
    tgt = mp.TopDownGenerateTarget(config=dict(image_size=[192, 256], heatmap_size=[48, 64]), sigma=2.0)
    gen = torch.Generator(device="cpu").manual_seed(1000)
    image = torch.randn(N, 3, 256, 192, generator=gen).to(dev)
    kp = torch.empty(N, 17, 3)
    kp[..., 0] = torch.rand(N, 17, generator=gen) * 232 - 20
    kp[..., 1] = torch.rand(N, 17, generator=gen) * 296 - 20
    kp[..., 2] = (torch.rand(N, 17, generator=gen) < 0.7).float()
    kp = kp.to(dev)
    t0, w0 = tgt(kp)
    step = GraphedTrainStep(nwl, opt, (image, t0, w0), loss_scale_manager=DynamicLossScaleManager(), resident=True, total_steps=total_steps)

    def run(steps):
        for _ in range(steps):
            target, weight = tgt(kp)  # as the benchmark's step: the targets are made on the device every step
            step(image, target, weight)

    return run


def time_steps(rounds, steps, warmup, dev):
    total = warmup + rounds * steps
    built = dict(joint_mse=build_step(mp.create_loss("joint_mse", use_target_weight=True), total, dev),
                 joint_ohkm_mse=build_step(mp.create_loss("joint_ohkm_mse", use_target_weight=True, topk=TOPK), total, dev))
    for run in built.values():
        run(warmup)
    torch.cuda.synchronize()
    ms = {name: [] for name in built}
    for _ in range(rounds):
        for name, run in built.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {name: dict(_stats(v), rounds_ms=[round(x, 3) for x in v]) for name, v in ms.items()}
    out["ohkm_minus_mse_ms"] = round(statistics.median(ms["joint_ohkm_mse"]) - statistics.median(ms["joint_mse"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--step-rounds", type=int, default=5, help="0 skips the training step")
    ap.add_argument("--step-steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: these are device times")
    dev = torch.device("cuda:0")
    out = dict(n=N, k=K, h=H, w=W, topk=TOPK, rounds=a.rounds, calls=a.calls, launches=time_launches(a.rounds, a.calls, dev))
    if a.step_rounds > 0:
        os.environ.setdefault("MINDPOSE_AUTOTUNE", "0")
        out["step_ms"] = time_steps(a.step_rounds, a.step_steps, a.step_warmup, dev)
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
