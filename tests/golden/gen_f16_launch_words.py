"""Generate tests/golden/f16_launch_words.json: per (desc, knob set) of tests/f16_launch_words.py the SHA-256 over the launch records
of every (variant, residuals, statistics mode) combination, the number of accepted combinations per kernel family over all of
them, and for six descs the word lists themselves.

The file pins the tile geometry of the fp16 convolution family (csrc/conv_f16*.hip), so it is recorded from the library of the commit
a change to that host code STARTS from, never from the changed code: build the parent commit in a worktree and point this script at
that library (no GPU needed; the entry is host-only),

    git worktree add ../parent HEAD~1 && make -C ../parent/mindpose_amd/csrc -j8
    MINDPOSE_HIP_LIB=$PWD/../parent/mindpose_amd/csrc/libmindpose_hip.so python tests/golden/gen_f16_launch_words.py

(a parent older than the ``mp_f16_conv_launch_words`` entry needs that one function of csrc/conv_f16.hip copied in first).
"""
import argparse
import json
import os
import sys

os.environ.setdefault("MINDPOSE_EXPERIMENT_KNOBS", "1")  # the MP_* knobs of the knob sets are honoured only then
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mindpose_amd import _lib  # noqa: E402
from tests import f16_launch_words as lw  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=lw.GOLDEN_PATH)
    args = ap.parse_args()
    print(f"library: {_lib.LIB_PATH}")
    golden = lw.record_all()
    totals = golden["served_total"]
    print(f"{len(golden['sha256'])} descs x {len(lw.KNOBS)} knob sets; accepted combinations per family: {totals}")
    assert all(n > 0 for n in totals.values()), "a family serves nothing: the golden would compare refusals only"
    assert sorted(golden["words"]) == sorted(lw.FULL) and all(golden["words"].values())
    with open(args.out, "w") as f:  # one desc / one variant's word lists per line
        f.write('{\n "served_total": ' + json.dumps(totals, sort_keys=True) + ',\n "sha256": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in golden["sha256"].items()))
        f.write('\n },\n "words": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {{\n" + ",\n".join(f"   {json.dumps(v)}: {json.dumps(w, separators=(',', ':'))}" for v, w in ws.items()) + "\n  }"
                           for k, ws in sorted(golden["words"].items())))
        f.write("\n }\n}\n")


if __name__ == "__main__":
    main()
