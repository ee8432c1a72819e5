"""Generate tests/golden/match_by_tag.npz: inputs and outputs of the REFERENCE's ``match_by_tag`` (mindpose/utils/match.py).

Run ONLY in the build container (needs /root/reference):  python tests/golden/gen_match_golden.py

The reference module imports only numpy / scipy, so it is loaded by file path (``mindpose/__init__.py``, which imports MindSpore,
is bypassed).  No reference source or bytecode is written anywhere; only inputs, arguments and the returned arrays are saved.
About 64 cases: clustered tags, rounded-norm ties, more detections than groups, ``ignore_too_much``, empty joints, L = 1 and 2.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/mindpose/utils/match.py"
JOINT_ORDER = [0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16]


def load_reference_match():
    spec = importlib.util.spec_from_file_location("_ref_match", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod.match_by_tag


def make_case(rng, kind, num_tags):
    k = 17
    m = int(rng.choice([5, 10, 30]))
    if kind == "ignore":
        m = 3
    persons = int(rng.integers(1, m + 3))
    centres = rng.normal(0, 3, (persons, num_tags)).astype(np.float32)
    if kind == "ties":  # integer-spaced tags: rounded distances tie everywhere
        centres = rng.integers(-3, 4, (persons, num_tags)).astype(np.float32)
    val = rng.random((k, m)).astype(np.float32)
    tag = np.zeros((k, m, num_tags), np.float32)
    who = rng.integers(0, persons, (k, m))
    noise = 0.05 if kind == "ties" else float(rng.choice([0.1, 0.4, 0.8]))
    tag[:] = centres[who] + rng.normal(0, noise, (k, m, num_tags)).astype(np.float32)
    if kind == "ties":
        tag = np.round(tag * 2) / 2
    ind = np.stack((rng.integers(0, 128, (k, m)), rng.integers(0, 128, (k, m))), axis=2).astype(np.float32)
    if kind == "added":  # the first joints of the order see one detection, later ones many: num_added > num_grouped
        val[JOINT_ORDER[0], 1:] = 0.0
        val[JOINT_ORDER[1], :] = 0.0
        val[JOINT_ORDER[2:6]] = np.maximum(val[JOINT_ORDER[2:6]], 0.5)
    if kind == "empty":
        dead = rng.choice(k, int(rng.integers(1, k)), replace=False)
        val[dead] = 0.0
    if kind == "allempty":
        val[:] = 0.05
    return val, tag, ind, m


def main():
    match_by_tag = load_reference_match()
    rng = np.random.default_rng(20240611)
    kinds = ["plain", "ties", "added", "ignore", "empty", "allempty"]
    out = {}
    i = 0
    for rep in range(6):
        for kind in kinds:
            for num_tags in (1, 2):
                if kind == "allempty" and rep > 1:
                    continue
                val, tag, ind, _ = make_case(rng, kind, num_tags)
                order = JOINT_ORDER if rep % 2 == 0 else list(rng.permutation(17))
                args = dict(vis_thr=float(rng.choice([0.1, 0.2])), tag_thr=float(rng.choice([1.0, 0.5])),
                            ignore_too_much=kind == "ignore" or bool(rep % 3 == 2), use_rounded_norm=kind == "ties" or rep % 2 == 0)
                res = match_by_tag(val, tag, ind, order, **args)
                out[f"c{i}_val"], out[f"c{i}_tag"], out[f"c{i}_ind"] = val, tag, ind
                out[f"c{i}_order"] = np.asarray(order, np.int64)
                out[f"c{i}_args"] = np.array([args["vis_thr"], args["tag_thr"], float(args["ignore_too_much"]),
                                              float(args["use_rounded_norm"])], np.float64)
                out[f"c{i}_out"] = res
                i += 1
    out["count"] = np.array(i)
    np.savez_compressed(os.path.join(HERE, "match_by_tag.npz"), **out)
    print(f"{i} cases")


if __name__ == "__main__":
    main()
