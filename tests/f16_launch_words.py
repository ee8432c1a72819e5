"""The launch records of the fp16 convolution family as numbers, and their digests: what tests/golden/gen_f16_launch_words.py records
from the library of the commit a change to the family's host code starts from, and what tests/test_f16_launch_words_cpu.py recomputes.

``mp_f16_conv_launch_words`` (include/mindpose_hip.h, host-only) builds a launch exactly as the entry points do and writes the two
return codes (build, dry dispatch) and - after an accepted build - kernel size, stride, variant, LDS bytes and every field of the
kernel parameter block.  A desc is crossed with variants -1 .. 47, the (residuals, statistics mode) pairs of ``MODES`` and the knob
sets of ``KNOBS``; one SHA-256 per (desc, knob set) covers all those records.

Descs: every case of the five tables of tests/f16_matrix.py, the four single-phase transposed-conv descs of tests/test_gpu_f16.py and
every distinct desc of tests/golden/bench_plan_picks.json (the real workload shapes).
"""
import ctypes
import hashlib
import json
import os

from mindpose_amd import _lib
from tests import f16_matrix as fm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_PATH = os.path.join(HERE, "golden", "f16_launch_words.json")

VARIANTS = list(range(-1, 48))
MODES = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (0, 2), (1, 2)]  # (n_res, stats mode)
KNOBS = {"none": {}, "mt_groups1": {"MP_F16_MT_GROUPS": 1}, "mt_groups3": {"MP_F16_MT_GROUPS": 3}, "ws_groups2": {"MP_F16_WS_GROUPS": 2},
         "ws_groups5": {"MP_F16_WS_GROUPS": 5}, "wreg_slow_dma": {"MP_F16_WREG_SLOW_DMA": 1}}
FAMILIES = {"tile": fm.TILE_VARIANTS, "mt": fm.MT_VARIANTS, "wreg": fm.WREG_VARIANTS, "ws": fm.WS_VARIANTS}
# (desc, knob set) whose word lists are stored beside the digest, so that a mismatch can be read: one per kernel family - under the
# knob that makes the family serve the small shape - the stride-2 weights-in-registers form and a four-phase launch
FULL = {"conv/11": "none", "conv/7": "mt_groups3", "wreg/5": "none", "ws/2": "ws_groups2", "wreg_s2/6": "none", "phases4/1": "none"}
CAP = 96
DESC_FIELDS = [name for name, _ in _lib.ConvDesc._fields_]


def _deconv_phase_desc(n, cin, cout, h, w, py, px):  # as tests/test_gpu_f16.py
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=2, kw=2, stride=1, pad_top=1 - py, pad_left=1 - px, conv_h=h, conv_w=w,
                         out_h=2 * h, out_w=2 * w, out_mul=2, out_rep=1, out_off_y=py, out_off_x=px, relu=1, flags=0)


def descs():
    """{name: ConvDesc}, in a fixed order"""
    out = {}
    for table, cases, desc_of in (("conv", fm.CONV_CASES, fm.conv_case_desc), ("wreg", fm.WREG_CASES, fm.conv_case_desc),
                                  ("ws", fm.WS_CASES, fm.conv_case_desc), ("wreg_s2", fm.WREG_S2_CASES, fm.s2_case_desc),
                                  ("phases4", fm.PHASES4_CASES, fm.phases4_case_desc)):
        for i, case in enumerate(cases):
            out[f"{table}/{i}"] = desc_of(case)
    for py in (0, 1):
        for px in (0, 1):
            out[f"deconv_phase/{py}{px}"] = _deconv_phase_desc(3, 64, 48, 16, 12, py, px)
    with open(os.path.join(HERE, "golden", "bench_plan_picks.json")) as f:
        picks = json.load(f)["f16"]
    seen = {}
    for rec in picks:
        key = tuple(rec["desc"][k] for k in DESC_FIELDS)
        if key not in seen:
            seen[key] = True
            out[f"bench/{len(seen) - 1}"] = _lib.ConvDesc(**rec["desc"])
    return out


def family_of(variant):
    return next((name for name, ids in FAMILIES.items() if variant in ids), "heuristic")


def words(desc, variant, n_res, stats):
    buf = (ctypes.c_int64 * CAP)()
    n = _lib.load().mp_f16_conv_launch_words(ctypes.byref(desc), variant, n_res, stats, buf, CAP)
    assert n >= 2, f"mp_f16_conv_launch_words returned {n}"
    return list(buf[:n])


def record(desc, knob_set, full=False):
    """(SHA-256 over every combination's words, {family: accepted combinations}, {variant: {"n_res/stats": words}} if full) of one
    (desc, knob set)"""
    h = hashlib.sha256()
    served = {name: 0 for name in list(FAMILIES) + ["heuristic"]}
    lists = {}
    with fm.knobs(**KNOBS[knob_set]):
        for v in VARIANTS:
            for n_res, stats in MODES:
                w = words(desc, v, n_res, stats)
                h.update(f"{v}/{n_res}/{stats}:{','.join(map(str, w))};".encode())
                if w[0] == 0 and w[1] == 0:
                    served[family_of(v)] += 1
                if full:
                    lists.setdefault(str(v), {})[f"{n_res}/{stats}"] = w
    return h.hexdigest(), served, lists


def pack_words(lists):
    """The stored form of a desc's word lists: per variant the first mode's list whole ("base"), every other mode as {position: value}
    where it differs from the base (a list of another length - a refusal - whole).  Variants no mode of which builds are left out:
    their lists are the two return codes, which the digest covers."""
    out = {}
    for v, modes in lists.items():
        if all(len(w) == 2 for w in modes.values()):
            continue
        base = modes[f"{MODES[0][0]}/{MODES[0][1]}"]
        out[v] = {"base": base}
        for m, w in modes.items():
            if w is not base:
                out[v][m] = w if len(w) != len(base) else {str(i): x for i, (x, b) in enumerate(zip(w, base)) if x != b}
    return out


def record_all():
    """The golden file's content: {"sha256": {desc: {knob set: digest}}, "served_total": {family: accepted combinations}, "words":
    {desc of FULL: packed word lists without knobs}}.  A knob set that is absent from a desc's digests has the digest of "none"
    (a knob that this desc's launches do not look at)."""
    golden = {"sha256": {}, "served_total": {name: 0 for name in list(FAMILIES) + ["heuristic"]}, "words": {}}
    for name, d in descs().items():
        golden["sha256"][name] = {}
        for ks in KNOBS:
            full = FULL.get(name) == ks
            digest, served, lists = record(d, ks, full)
            if ks == "none" or digest != golden["sha256"][name]["none"]:
                golden["sha256"][name][ks] = digest
            for family, n in served.items():
                golden["served_total"][family] += n
            if full:
                golden["words"][name] = pack_words(lists)
    return golden
