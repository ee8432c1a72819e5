"""Digest of the launch plans the builder records, for comparing two trees (or two commits) EXACTLY: a change that claims to leave
behaviour alone must leave every line of this output byte-identical.

    python tools/plan_digest.py [--only SUBSTRING] > digest.jsonl

One JSON line per case (network, head, amp level, input shape): every plan entry as ``[layer_info[i], entry_info(i)]`` (the python-side
record and the launch geometry the native side chose) and the sha256 of the output(s) for a seeded input; then one last line with
the tuner's whole table, sorted keys with their picks (at the end and not per case: a process that replays a persisted cache holds
every key from its first lookup on, the process that timed them collected them case by case).  The cases walk every way a conv
becomes a plan entry: the top-down networks at 1, 32 and 128 crops in fp32 and amp O2, the fp32 and fp16 transposed-conv head of
ResNet-50, HRNet-W48 at 384 x 288, and HigherHRNet at the bottom-up sizes (column-banded convs and transposed convs, ragged bands
included).  Per-case wall time goes to stderr.

Run both sides with one library file (``MINDPOSE_HIP_LIB``: the tune-cache stamp hashes it) and either ``MINDPOSE_AUTOTUNE=0`` (no
timing decides anything) or one shared ``MINDPOSE_TUNE_CACHE`` file that the first side wrote.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mindpose_amd as mp  # noqa: E402

try:
    from mindpose_amd.models.tuner import _TUNE_CACHE  # noqa: E402
except ImportError:  # the other side of a comparison may be a tree from before the tuner had a module of its own
    from mindpose_amd.models.layers import _TUNE_CACHE  # noqa: E402

CASES = [("hrnet_w32", "hrnet_head", amp, (n, 3, 256, 192)) for n in (1, 32, 128) for amp in ("O0", "O2")]
CASES += [("resnet50", "simple_baseline_head", amp, (128, 3, 256, 192)) for amp in ("O0", "O2")]
CASES += [("hrnet_w48", "hrnet_head", "O2", (128, 3, 384, 288))]
CASES += [("hrnet_w32", "higher_hrnet_head", amp, (1, 3, h, w)) for h, w in ((512, 512), (512, 832), (576, 704)) for amp in ("O0", "O2")]


def digest(backbone, head, amp, shape, dev):
    net = mp.init_synthetic(mp.create_network(backbone, head), seed=0).to(dev).eval()
    if amp != "O0":
        mp.models.auto_mixed_precision(net, amp)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(7)).to(dev)
    out = net(x)
    torch.cuda.synchronize()
    outs = out if isinstance(out, (list, tuple)) else [out]
    plan = net.get_plan(x.shape, dev)
    return dict(case=[backbone, head, amp, list(shape)],
                entries=[[plan.layer_info[i], plan.entry_info(i)] for i in range(len(plan))],
                sha256=[hashlib.sha256(o.cpu().contiguous().numpy().tobytes()).hexdigest() for o in outs])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", default="", help="run the cases whose 'backbone head amp NxCxHxW' name contains this")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    t_all = time.time()
    for backbone, head, amp, shape in CASES:
        name = f"{backbone} {head} {amp} {'x'.join(map(str, shape))}"
        if args.only not in name:
            continue
        t0 = time.time()
        print(json.dumps(digest(backbone, head, amp, shape, dev), sort_keys=True), flush=True)
        print(f"{name}: {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if not args.only:
        print(json.dumps(dict(tuner=sorted((k, v) for k, v in _TUNE_CACHE.items() if isinstance(k, str)))))
    print(f"all cases: {time.time() - t_all:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
