"""Generate tests/golden/step_end_launch_trace.json: per case of tests/step_end_trace.py the number of events, the count per library
function / torch op, the number of ``empty*`` allocations and the SHA-256 of the trace's canonical JSON (the format of
train_launch_trace.json).

The file pins what the step end launches (`mindpose_amd/utils/adamw.py`, `mindpose_amd/utils/step_tail.py`), so it is recorded from
the commit a change to those modules STARTS from, never from the changed modules: check the parent commit out into a worktree, copy
tests/train_trace.py, tests/step_end_trace.py and this script into it and run it THERE (no GPU and no built library needed):

    git worktree add ../parent HEAD~1 && cp tests/train_trace.py tests/step_end_trace.py ../parent/tests/ && cp tests/golden/gen_step_end_trace.py ../parent/tests/golden/
    (cd ../parent && python tests/golden/gen_step_end_trace.py --out "$OLDPWD/tests/golden/step_end_launch_trace.json")

``--dump DIR`` writes every case's full trace as text (one event per line) instead; run it on both trees and ``diff -r`` the two
directories to see where a digest disagrees.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import step_end_trace  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(HERE, "step_end_launch_trace.json"))
    ap.add_argument("--dump", metavar="DIR", help="write the full traces as text into DIR and leave the golden file alone")
    ap.add_argument("cases", nargs="*", help="case names (default: all)")
    args = ap.parse_args()
    names = args.cases or list(step_end_trace.CASES)
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    golden = {}
    for name in names:
        events, empties = step_end_trace.trace_case(name)
        if args.dump:
            with open(os.path.join(args.dump, name + ".txt"), "w") as f:
                f.write(step_end_trace.dump_text(events))
                f.write(f"# empty* allocations: {empties}\n")
        golden[name] = step_end_trace.summarise(events, empties)
        print(f"{name}: {golden[name]['events']} events, {empties} empty*, {golden[name]['sha256'][:12]}")
    if not args.dump:
        with open(args.out, "w") as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
