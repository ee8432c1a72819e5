"""Generate tests/golden/step_end_update_digests.json: per case of tests/step_end_bits.py the SHA-256 of the parameter and state
bytes an update entry leaves behind (for the cases with inf / NaN planted in the gradient: the digest of the outputs that are not
NaN and the indices of those that are).

The file pins the BITS of the update kernels, so it is recorded on the GPU from the library of the commit a change to them STARTS
from, never from the changed kernels: build the parent commit in a worktree and point this script at that library,

    git worktree add ../parent HEAD~1 && make -C ../parent/mindpose_amd/csrc -j8
    MINDPOSE_HIP_LIB=$PWD/../parent/mindpose_amd/csrc/libmindpose_hip.so python tests/golden/gen_step_end_golden.py

(the C ABI of the entries is the same on both sides; only the library differs).
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mindpose_amd import _lib  # noqa: E402
from tests import step_end_bits  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(HERE, "step_end_update_digests.json"))
    args = ap.parse_args()
    print(f"library: {_lib.LIB_PATH}")
    golden = {step_end_bits.case_id(*case): step_end_bits.digest(*case) for case in step_end_bits.CASES}
    with open(args.out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(golden)} cases -> {args.out}")


if __name__ == "__main__":
    main()
