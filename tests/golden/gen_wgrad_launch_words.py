"""Generate tests/golden/wgrad_launch_words.json: per record of tests/wgrad_launch_words.py the SHA-256 over the launch words of its
queries, the number of launches the library accepts over all of them, and for seven records the word lists themselves.

The file pins the geometry and the dispatch of the weight-gradient family (csrc/conv_wgrad.hip, csrc/wgrad_f16.hip), so it is recorded
from the library of the commit a change to that host code STARTS from, never from the changed code: build the parent commit in a
worktree and point this script at that library (no GPU needed; the entry is host-only),

    git worktree add ../parent HEAD~1 && make -C ../parent/mindpose_amd/csrc -j8
    MINDPOSE_HIP_LIB=$PWD/../parent/mindpose_amd/csrc/libmindpose_hip.so python tests/golden/gen_wgrad_launch_words.py

(a parent older than the ``mp_conv_wgrad_launch_words`` entry needs that entry added to its two files first).
"""
import argparse
import json
import os
import sys

os.environ.setdefault("MINDPOSE_EXPERIMENT_KNOBS", "1")  # the MP_* knobs of the records are honoured only then
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mindpose_amd import _lib  # noqa: E402
from tests import wgrad_launch_words as lw  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=lw.GOLDEN_PATH)
    args = ap.parse_args()
    print(f"library: {_lib.LIB_PATH}")
    golden = lw.record_all()
    print(f"{len(golden['sha256'])} records, {golden['accepted']} accepted launches")
    assert golden["accepted"] > len(golden["sha256"]) and sorted(golden["words"]) == sorted(lw.FULL)
    with open(args.out, "w") as f:  # one record per line
        f.write('{\n "accepted": ' + str(golden["accepted"]) + ',\n "sha256": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in golden["sha256"].items()))
        f.write('\n },\n "words": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in sorted(golden["words"].items())))
        f.write("\n }\n}\n")


if __name__ == "__main__":
    main()
