"""The launches of the weight-gradient family (csrc/conv_wgrad.hip, csrc/wgrad_f16.hip) as numbers, and their digests: what
tests/golden/gen_wgrad_launch_words.py records from the library of the commit a change to the family's host code starts from, and what
tests/test_wgrad_launch_words_cpu.py recomputes.

``mp_conv_wgrad_launch_words`` (include/mindpose_hip.h, host-only; `wgrad_matrix.launch_words` names its words) runs the geometry as
the entry points do and writes the return code, every non-pointer field of the kernel parameter block, grid, block, LDS bytes, the
chosen kernel and the chosen slab reduce.  One SHA-256 per (case, knob set) over

  * the rows of the three tables of tests/wgrad_matrix.py under their knobs - fp16 rows through the single-layer entry and as a
    grouped launch of one, grouped rows with their job count;
  * the layer shapes of tools/bench_wgrad32.py and tools/bench_wgrad16.py at N = 128: the single-layer entry, grouped launches of
    one and of eight layers;
  * the 600 seeded random shapes of `wgrad_matrix.random_draws` under their knob draws, fp32 and fp16 in one digest.
"""
import ast
import hashlib
import os

from tests import wgrad_matrix as wm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_PATH = os.path.join(HERE, "golden", "wgrad_launch_words.json")
BENCH_N = 128
# records whose word lists are stored beside the digest, so that a mismatch can be read: the two fp32 kernels and the four fp16 forms
FULL = ["f32/n5_390to500_k3s1_20x12", "f32/n11_512to500_k3s1_8x6", "f16/n5_40to24_k3s1_40x12-WGS4", "f16/n5_72to80_k3s1_20x12-WGS8",
        "f16/n5_3to64_k3s2_40x24-WGS3", "f16/n3_16to24_k3s2_12x200-WGS2-DMA0", "f16_grouped/n5_72to80_k3s1_20x12-WGS16"]


def bench_shapes(tool):
    """SHAPES of tools/<tool>.py - (cin, cout, h, w, k, stride) - as cases at N = 128, read without running the tool"""
    with open(os.path.join(os.path.dirname(HERE), "tools", tool + ".py")) as f:
        tree = ast.parse(f.read())
    shapes = next(ast.literal_eval(node.value) for node in tree.body
                  if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "SHAPES")
    return [(BENCH_N, cin, cout, k, st, h, w) for cin, cout, h, w, k, st in shapes]


def queries():
    """{record name: [(case, half, n_jobs, knob environment)]}, in a fixed order"""
    out = {}
    for case, knobs, _ in wm.F32_CASES:
        out["f32/" + wm.case_id(case, knobs)] = [(case, 0, 0, knobs)]
    for case, knobs, _ in wm.F16_CASES:
        out["f16/" + wm.case_id(case, knobs)] = [(case, 1, jobs, wm.env16(knobs)) for jobs in (0, 1)]
    for case, knobs, jobs in wm.F16_GROUPED_CASES:
        out["f16_grouped/" + wm.case_id(case, knobs)] = [(case, 1, jobs, wm.env16(knobs))]
    for case in bench_shapes("bench_wgrad32"):
        out["bench32/" + wm.case_id(case, {})] = [(case, 0, 0, {})]
    for case in bench_shapes("bench_wgrad16"):
        out["bench16/" + wm.case_id(case, {})] = [(case, 1, jobs, {}) for jobs in (0, 1, 8)]
    for i, (case, simple, knobs, jobs) in enumerate(wm.random_draws(600)):
        out[f"random/{i}"] = [(case, 0, 0, {"MP_WGRAD_SIMPLE": "1"} if simple else {}), (case, 1, 0 if jobs == 1 else jobs, wm.env16(knobs))]
    return out


def record(name, qs):
    """(SHA-256 over the words of a record's queries, launches among them that the library accepts, the word lists)"""
    h = hashlib.sha256()
    lists = [wm.launch_words(case, half, jobs, **env) for case, half, jobs, env in qs]
    for (case, half, jobs, env), w in zip(qs, lists):
        h.update(f"{half}/{jobs}:{','.join(map(str, w))};".encode())
    return h.hexdigest(), sum(w[0] == 0 for w in lists), lists


def record_all():
    """The golden file's content: {"sha256": {record: digest}, "accepted": launches the library accepts, "words": {record of FULL:
    word lists}}"""
    golden = {"sha256": {}, "accepted": 0, "words": {}}
    for name, qs in queries().items():
        digest, accepted, lists = record(name, qs)
        golden["sha256"][name] = digest
        golden["accepted"] += accepted
        if name in FULL:
            golden["words"][name] = lists
    return golden
