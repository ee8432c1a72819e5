"""Generate tests/golden/f16_conv_bits.json: per (case, variant, knob set) of tests/f16_conv_bits.py the SHA-256 over the bytes the fp16
convolution kernels leave behind - output tensor, partial sums and the operand-route activation tensor of every mode the pair serves
(stored per (case, knob set) as digest -> the variants that share it).

The file pins the BITS of the four kernels of csrc/conv_f16*.hip, so it is recorded on the GPU from the library of the commit a change
to them STARTS from, never from the changed kernels: build the parent commit in a worktree and point this script at that library,

    git worktree add ../parent HEAD~1 && make -C ../parent/mindpose_amd/csrc -j8
    MINDPOSE_HIP_LIB=$PWD/../parent/mindpose_amd/csrc/libmindpose_hip.so python tests/golden/gen_f16_conv_bits.py

(the C ABI of the entries is the same on both sides; only the library differs).
"""
import argparse
import json
import os
import sys

os.environ.setdefault("MINDPOSE_EXPERIMENT_KNOBS", "1")  # the MP_* knobs of the knob sets are honoured only then
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mindpose_amd import _lib  # noqa: E402
from tests import f16_conv_bits as cb  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(HERE, "f16_conv_bits.json"))
    args = ap.parse_args()
    print(f"library: {_lib.LIB_PATH}")
    golden = {}
    for group in cb.GROUPS:
        golden[group] = {}
        keys = []
        for ci, env in cb.runs(group):
            run = cb.digests(group, ci, env)
            keys += list(run)
            if run:
                golden[group][cb.run_id(ci, env)] = cb.pack(run)
        assert sorted(keys) == sorted(cb.expected_keys(group)) and keys, group
        print(f"{group}: {len(keys)} records", flush=True)
    with open(args.out, "w") as f:  # one (case, knob set) per line
        f.write("{\n" + ",\n".join(f" {json.dumps(g)}: {{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in runs.items()) + "\n }"
                                   for g, runs in golden.items()) + "\n}\n")


if __name__ == "__main__":
    main()
