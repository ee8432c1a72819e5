"""Generate tests/golden/wgrad_bits.json: per row of the three tables of tests/wgrad_matrix.py and per job the SHA-256 of the weight
gradient the kernels leave behind, with accumulate = 0 and with accumulate = 1 (tests/wgrad_bits.py).

The file pins the BITS of the kernels of csrc/conv_wgrad.hip and csrc/wgrad_f16.hip, so it is recorded on the GPU from the library of
the commit a change to them STARTS from, never from the changed kernels: build the parent commit in a worktree and point this script
at that library,

    git worktree add ../parent HEAD~1 && make -C ../parent/mindpose_amd/csrc -j8
    MINDPOSE_HIP_LIB=$PWD/../parent/mindpose_amd/csrc/libmindpose_hip.so python tests/golden/gen_wgrad_bits.py

(the C ABI of the entries is the same on both sides; only the library differs).
"""
import argparse
import json
import os
import sys

os.environ.setdefault("MINDPOSE_EXPERIMENT_KNOBS", "1")  # the MP_* knobs of the rows are honoured only then
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mindpose_amd import _lib  # noqa: E402
from tests import wgrad_bits as wb  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(HERE, "wgrad_bits.json"))
    args = ap.parse_args()
    print(f"library: {_lib.LIB_PATH}")
    golden = {}
    for table, rows in wb.TABLES.items():
        golden[table] = {wb.run_id(table, i): wb.digests(table, i) for i in range(len(rows))}
        assert len(golden[table]) == len(rows), f"{table}: two rows share an id"
        print(f"{table}: {len(rows)} rows", flush=True)
    with open(args.out, "w") as f:  # one row per line
        f.write("{\n" + ",\n".join(f" {json.dumps(t)}: {{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n }"
                                   for t, rows in golden.items()) + "\n}\n")


if __name__ == "__main__":
    main()
