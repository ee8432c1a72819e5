"""HigherHRNet-W32 bottom-up inference timings on one GPU; prints ONE JSON line.

  python tools/bench_bottomup.py [--steps 20]

- forward: network plan (tuner on) at N = 1 and N = 32 for fp32 and amp O2, with the algorithmic GFLOP per image recomputed from the
  plan's recorded MACs (2 FLOP per MAC);
- decoder: BottomUpHeatMapAEDecoder (two launches) at the eval map size 256 x 416 (N = 1) and 256 x 256 (N = 32), microseconds per
  image and the fraction of 8 TB/s reached on its algorithmic bytes (reads: 17 full-resolution heat maps + 34 half-resolution
  channels; writes: heatmap_raw + tagging);
- match_by_tag: host milliseconds per image on the decoder's output of random maps.
Forward sizes are the recipe's eval images: 512 x 512 (N = 1 and 32) and 512 x 832 (N = 1).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mindpose_amd as mp  # noqa: E402
from mindpose_amd.utils.match import match_by_tag  # noqa: E402

DEV = torch.device("cuda:0")
HBM = 8e12
JOINT_ORDER = [0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16]


def _time(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps  # ms


def forward(amp, n, h, w, steps):
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
    if amp != "O0":
        mp.models.auto_mixed_precision(net, amp)
    image = net.input_buffer((n, 3, h, w), DEV)
    image.copy_(torch.randn(n, 3, h, w))
    ms = _time(lambda: net(image), steps)
    plan = net.get_plan((n, 3, h, w), DEV)
    return dict(amp=amp, n=n, h=h, w=w, ms=round(ms, 4), img_s=round(n * 1000 / ms, 1),
                gflop_per_image=round(2 * plan.total_macs / n / 1e9, 2))


def decoder(n, h, w, steps):
    g = torch.Generator().manual_seed(0)
    outs = [torch.rand(n, 34, h // 2, w // 2, generator=g).to(DEV), torch.rand(n, 17, h, w, generator=g).to(DEV)]
    mask = torch.ones(n, 2 * h, 2 * w, dtype=torch.bool, device=DEV)
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    ms = _time(lambda: dec(outs, mask), steps)
    nbytes = n * 4 * (17 * h * w + 34 * (h // 2) * (w // 2) + 2 * 17 * h * w)
    val, tag, ind, _, _ = dec(outs, mask)
    t0 = time.perf_counter()
    for i in range(n):
        match_by_tag(val[i].cpu().numpy(), tag[i].cpu().numpy(), ind[i].cpu().numpy(), JOINT_ORDER)
    match_ms = (time.perf_counter() - t0) * 1000 / n
    return dict(n=n, h=h, w=w, us_per_image=round(ms * 1000 / n, 2), hbm_fraction=round(nbytes / (ms * 1e-3) / HBM, 3),
                mb_per_image=round(nbytes / n / 1e6, 2), match_ms_per_image=round(match_ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    res = dict(workload="higher_hrnet_w32_bottomup",
               forward=[forward(a, n, h, w, args.steps) for a in ("O0", "O2") for n, h, w in ((1, 512, 512), (32, 512, 512), (1, 512, 832))],
               decoder=[decoder(1, 256, 416, args.steps), decoder(32, 256, 256, args.steps)])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
