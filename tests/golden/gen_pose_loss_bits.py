"""Generate tests/golden/pose_loss_bits.json: per group of tests/pose_loss_bits.py the SHA-256 of every output the top-down decode,
target and loss entries leave behind (for an output with NaNs: the digest of its other values and the index runs of the NaNs).

The file pins the BITS of those kernels, so it is recorded on the GPU from the library of the commit a change to them STARTS from,
never from the changed kernels: build the parent commit in a worktree and point this script at that library,

    git worktree add ../parent HEAD~1 && make -C ../parent/mindpose_amd/csrc -j8
    MINDPOSE_HIP_LIB=$PWD/../parent/mindpose_amd/csrc/libmindpose_hip.so python tests/golden/gen_pose_loss_bits.py

(the C ABI of the entries is the same on both sides; only the library differs).
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mindpose_amd import _lib  # noqa: E402
from tests import pose_loss_bits  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(HERE, "pose_loss_bits.json"))
    args = ap.parse_args()
    print(f"library: {_lib.LIB_PATH}")
    golden = {group: pose_loss_bits.digest(group) for group in pose_loss_bits.GROUPS}
    with open(args.out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(golden)} groups -> {args.out}")


if __name__ == "__main__":
    main()
