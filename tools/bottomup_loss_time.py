"""Device times of the bottom-up training ends at the recipe's shapes (N = 32, stages 128 x 128 and 256 x 256, K = 17, M = 30);
prints ONE JSON line.

  python tools/bottomup_loss_time.py [--steps 50]

Sections (each timed by device events around ``steps`` back-to-back calls after a warm-up, beside the SAME formula composed from
stock torch ops on the same GPU):
- mse_fwd_128 / mse_fwd_256, mse_bwd_128 / mse_bwd_256: ``mp_joints_mse_mask_fwd`` / ``_bwd`` on the views AEMultiLoss passes
  (heat-map channels of the stage tensor, a corner of the padded [N, 2, 17, 256, 256] target and of the mask).  HBM-bound: bytes =
  pred + target + mask read (+ gradient written), reported as a fraction of 8 TB/s.
- ae_fwd, ae_bwd: ``mp_ae_loss_fwd`` / ``_bwd`` on the 17 tag planes of the 128 x 128 stage.  The forward is a gather of <= 510
  values per image (latency-bound, no bandwidth figure); the backward writes the 17 tag planes (bytes = that write).  The torch
  composition is the gather form (index the M*K tags, reduce), not the reference's [N, M, K, H, W] scatter, which does not fit.
- target: ``mp_bottomup_target`` for both stages (write-only: the padded target + tag_ind).  The torch composition evaluates the
  Gaussians densely over [N, M, K, H, W] per stage in chunks and takes the maximum over persons.

``--only NAME`` runs one section in this process; without it every section runs in a child process of its own under a time limit
(``--section-timeout`` seconds), and a section that fails or overruns ends the run.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mindpose_amd as mp  # noqa: E402
from mindpose_amd.models.loss.ae import launch_ae_bwd, launch_ae_fwd  # noqa: E402
from mindpose_amd.models.loss.mse import launch_mse_mask_bwd, launch_mse_mask_fwd  # noqa: E402

HBM = 8e12
N, K, M = 32, 17, 30
SECTIONS = ["mse_fwd_128", "mse_fwd_256", "mse_bwd_128", "mse_bwd_256", "ae_fwd", "ae_bwd", "target"]


def _time(fn, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000 / steps  # us


def _report(ours_us, torch_us, nbytes=None):
    out = dict(us=round(ours_us, 2), torch_us=round(torch_us, 2), torch_over_ours=round(torch_us / ours_us, 2))
    if nbytes:
        out["mbytes"] = round(nbytes / 1e6, 2)
        out["hbm_fraction"] = round(nbytes / (ours_us * 1e-6) / HBM, 3)
    return out


def _mse_inputs(size, dev):
    g = torch.Generator().manual_seed(0)
    stage = torch.randn(N, 2 * K if size == 128 else K, size, size, generator=g).to(dev)
    target = torch.rand(N, 2, K, 256, 256, generator=g).to(dev)
    mask = (torch.rand(N, 2, 256, 256, generator=g) > 0.2).float().to(dev)
    i = 0 if size == 128 else 1
    return stage, stage[:, :K], target[:, i, :, :size, :size], mask[:, i, :size, :size]


def mse(size, backward, steps, dev):
    stage, pv, tv, mv = _mse_inputs(size, dev)
    plane = N * K * size * size * 4
    if not backward:
        ours = _time(lambda: launch_mse_mask_fwd(pv, tv, mv), steps)
        ref = _time(lambda: (((pv - tv) ** 2) * mv[:, None]).mean(), steps)
        return _report(ours, ref, 2 * plane + N * size * size * 4)
    grad = torch.empty_like(stage)
    go = torch.ones(1, device=dev)
    scale = 2.0 / (N * K * size * size)
    ours = _time(lambda: launch_mse_mask_bwd(pv, tv, mv, go, grad[:, :K]), steps)
    ref = _time(lambda: grad[:, :K].copy_((pv - tv) * mv[:, None] * (go * scale)), steps)
    return _report(ours, ref, 3 * plane + N * size * size * 4)


def _ae_inputs(dev):
    rng = np.random.RandomState(0)
    g = torch.Generator().manual_seed(0)
    stage = torch.randn(N, 2 * K, 128, 128, generator=g).to(dev)
    ind = np.zeros((N, M, K, 2), np.int32)
    for n in range(N):
        for m in range(rng.randint(1, M + 1)):
            vis = rng.rand(K) < 0.75
            ind[n, m, :, 0] = np.where(vis, rng.randint(0, 128 * 128, K), 0)
            ind[n, m, :, 1] = vis
    return stage, stage[:, K:], torch.from_numpy(ind).to(dev)


def _ae_torch(tags, ind):
    """ae.py's formulas on the gathered tags (flags are 0 / 1 here)."""
    n, k, h, w = tags.shape
    f = ind[..., 1].float()                                                        # [N, M, K]
    t = torch.gather(tags.reshape(n, 1, k, h * w).expand(n, ind.shape[1], k, h * w), 3, ind[..., 0:1].long())[..., 0] * f
    k_n = f.sum(dim=2)
    h_n = t.sum(dim=2) / (k_n + 0.01)
    pull = (((h_n[..., None] - t) * f) ** 2).sum(dim=2) / (k_n + 0.01)
    valid = (k_n > 0).float()
    cnt = valid.sum(dim=1)
    pull = pull.sum(dim=1) / (cnt + 0.01)
    d = h_n[:, :, None] - h_n[:, None, :]
    push = (torch.exp(-(d ** 2)) * valid[:, :, None] * valid[:, None, :]).sum(dim=(1, 2)) - cnt
    push = 0.5 * push / (cnt * (cnt - 1) + 0.01)
    return torch.stack([push.mean(), pull.mean()])


def ae(backward, steps, dev):
    stage, tags, ind = _ae_inputs(dev)
    if not backward:
        return _report(_time(lambda: launch_ae_fwd(tags, ind), steps), _time(lambda: _ae_torch(tags, ind), steps))
    grad = torch.empty_like(stage)
    go = torch.ones(2, device=dev)
    ours = _time(lambda: launch_ae_bwd(tags, ind, go, grad[:, K:]), steps)
    leaf = stage.clone().requires_grad_(True)

    def ref():
        leaf.grad = None
        _ae_torch(leaf[:, K:], ind).sum().backward()

    return _report(ours, _time(ref, steps), N * K * 128 * 128 * 4)


def target(steps, dev):
    rng = np.random.RandomState(0)
    sizes = [(128, 128), (256, 256)]
    t = mp.BottomUpGenerateTarget(config=dict(image_size=[512, 512], max_image_size=[512, 512], heatmap_sizes=sizes, flip_pairs=[[1, 2]],
                                              pixel_std=200.0, tag_per_joint=True))
    counts = rng.randint(1, M + 1, N)
    base = np.concatenate([rng.uniform(-4, 132, (N, 1, M, K, 2)), (rng.rand(N, 1, M, K, 1) < 0.75)], axis=4)
    kp = np.concatenate([base, base * np.array([2.0, 2.0, 1.0])], axis=1).astype(np.float32)
    kp_dev = torch.from_numpy(kp).to(dev)
    ours = _time(lambda: t.generate_batch(kp_dev, counts), steps)
    live = (torch.arange(M, device=dev)[None, :] < torch.from_numpy(counts).to(dev)[:, None])

    def ref():
        out = torch.zeros(N, 2, K, 256, 256, device=dev)
        for s, (w, h) in enumerate(sizes):
            xs, ys = torch.arange(w, device=dev, dtype=torch.float32), torch.arange(h, device=dev, dtype=torch.float32)
            for n0 in range(0, N, 4):  # chunks: [4, M, K, H, W] fp32 at 256 x 256 is 2 GB
                p = kp_dev[n0:n0 + 4, s]
                mu = torch.round(p[..., :2])
                on = (p[..., 2] > 0) & live[n0:n0 + 4, :, None]
                dx = (xs[None, None, None, :] - mu[..., 0:1]).abs() <= 6
                dy = (ys[None, None, None, :] - mu[..., 1:2]).abs() <= 6
                ex = torch.exp(-((xs[None, None, None, :] - p[..., 0:1]) ** 2) / 8.0) * dx * on[..., None]
                ey = torch.exp(-((ys[None, None, None, :] - p[..., 1:2]) ** 2) / 8.0) * dy
                out[n0:n0 + 4, s, :, :h, :w] = (ey[..., :, None] * ex[..., None, :]).amax(dim=1)
        return out

    nbytes = N * 2 * K * 256 * 256 * 4 + N * 2 * M * K * 2 * 4
    return _report(ours, _time(ref, max(3, steps // 10), warmup=2), nbytes)


def run_section(name, steps):
    dev = torch.device("cuda:0")
    if name.startswith("mse_"):
        return mse(int(name[-3:]), "bwd" in name, steps, dev)
    if name.startswith("ae_"):
        return ae(name == "ae_bwd", steps, dev)
    return target(steps, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only", choices=SECTIONS)
    ap.add_argument("--section-timeout", type=int, default=120)
    args = ap.parse_args()
    if args.only:
        if not torch.cuda.is_available():
            sys.exit("no GPU: these are device times")
        print(json.dumps({args.only: run_section(args.only, args.steps)}))
        return
    result = {}
    for name in SECTIONS:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name, "--steps", str(args.steps)],
                              capture_output=True, text=True, timeout=args.section_timeout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stdout + proc.stderr)
            sys.exit(f"section {name} failed ({proc.returncode}): stopping")
        result.update(json.loads(proc.stdout.strip().splitlines()[-1]))
    print(json.dumps(dict(n=N, k=K, m=M, steps=args.steps, sections=result)))


if __name__ == "__main__":
    main()
