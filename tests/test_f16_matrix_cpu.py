"""Floors under the generated (shape, tile variant) matrix of the fp16 convolution tests (tests/f16_matrix.py).

The GPU tests collect only the pairs `mp_f16_conv_supported` reports as served, so a kernel family that silently stopped serving its
shapes would shrink the matrix instead of failing it.  These host-only checks (the query runs the entry point's own checks and the
family's dispatch without a launch - no GPU needed) pin the matrix from below:
  * every forced variant id serves at least one case of its family's table, every case is served by at least one variant;
  * the (shape, variant) pairs the tuner picked for the three bench plans on an MI355X (tests/golden/bench_plan_picks.json, written
    by tools/dump_plan_picks.py) are still served by the forced-variant entry;
  * the statistics builds the weight-stationary kernel leaves out for register budget are exactly the listed ones;
  * the edge matrix (second half of tests/f16_matrix.py): every forced variant of every family meets every class of tile
    geometry of its family (`fm.classes`, read from `mp_f16_conv_launch_words`) and every launch kind its family takes in at least
    one collected pair; the only holes are the rows of EXEMPT, each with its reason from the configure code and each proven out of
    reach on the family's search grid.
"""
import json
import os

import pytest

from tests import f16_matrix as fm

HERE = os.path.dirname(os.path.abspath(__file__))


def _coverage(cases, variants, desc_of, res_of=lambda c: 0, stats=0, **env):
    pairs = fm.served_pairs(cases, variants, desc_of, res_of, stats, **env)
    by_variant = {v: 0 for v in variants}
    by_case = {i: 0 for i in range(len(cases))}
    for pr in pairs:
        case, v = pr.values
        by_variant[v] += 1
        by_case[cases.index(case)] += 1
    return pairs, by_variant, by_case


FAMILIES = [
    # name, cases, variants, desc_of, res_of, knob sets (a pair counts when ANY knob set serves it), floor on the matrix size
    ("one-tile", fm.CONV_CASES, fm.TILE_VARIANTS, fm.conv_case_desc, fm.conv_case_res, [{}], 120),
    ("multi-tile", fm.CONV_CASES, fm.MT_VARIANTS, fm.conv_case_desc, fm.conv_case_res, [dict(MP_F16_MT_GROUPS=1), dict(MP_F16_MT_GROUPS=3)], 95),
    ("weights-in-registers", fm.WREG_CASES, fm.WREG_VARIANTS, fm.conv_case_desc, fm.conv_case_res, [{}], 90),
    ("weights-in-registers stride 2", fm.WREG_S2_CASES, fm.WREG_S2_VARIANTS, fm.s2_case_desc, fm.s2_case_res, [{}], 28),
    ("weight-stationary", fm.WS_CASES, fm.WS_VARIANTS, fm.conv_case_desc, fm.conv_case_res, [dict(MP_F16_WS_GROUPS=2), dict(MP_F16_WS_GROUPS=5)], 17),
    ("four-phase data gradient", fm.PHASES4_CASES, [0, 4], fm.phases4_case_desc, lambda c: 0, [{}], 8),
]


@pytest.mark.parametrize("family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_forced_variant_serves_a_case_and_every_case_is_served(family):
    name, cases, variants, desc_of, res_of, knob_sets, floor = family
    v_total = {v: 0 for v in variants}
    c_total = {i: 0 for i in range(len(cases))}
    for env in knob_sets:
        pairs, by_variant, by_case = _coverage(cases, variants, desc_of, res_of, 0, **env)
        assert len(pairs) >= floor, f"{name} {env}: the served matrix shrank to {len(pairs)} pairs (floor {floor})"
        for v, k in by_variant.items():
            v_total[v] += k
        for i, k in by_case.items():
            c_total[i] += k
    assert not [v for v, k in v_total.items() if k == 0], f"{name}: variants that serve none of the family's cases"
    assert not [i for i, k in c_total.items() if k == 0], f"{name}: cases no variant of the family serves"


# ---- the edge matrix (tests/f16_matrix.py second half) ---------------------------------------------------------------

# (family, variant, class, why) - the ONLY (variant, class) holes the floor below lets through.  Each sentence states the reason from
# the configure code; test_exempt_classes_are_out_of_reach proves every row on the family's search grid, so a hole that a case could
# close cannot sit here.
_ONE_CHUNK = "24 is the build without a chunk loop (one_chunk in kF16Variants): f16_configure and launch_f16_ks refuse n_chunks != 1"
_CT16 = "its cout tile is 16 wide and Cout_pad16 is a multiple of 16 (f16_geom_tensors): the last cout tile is always whole"
_NBUF = "a two-workgroups-per-CU build: the nbuf loop of f16_configure_mt stops at 2 unless occ == 1, these never fall back to one input buffer"
EXEMPT = [
    ("tile", 24, "chunks:2", _ONE_CHUNK), ("tile", 24, "chunks:odd", _ONE_CHUNK), ("tile", 24, "chunks:even", _ONE_CHUNK),
    ("tile", 24, "chunks:c8in-tail", _ONE_CHUNK),
    ("tile", 20, "cout:partial-tile", _CT16), ("tile", 21, "cout:partial-tile", _CT16),
    ("mt", 22, "cout:partial-tile", _CT16), ("mt", 23, "cout:partial-tile", _CT16),
    ("mt", 10, "nbuf:1", _NBUF), ("mt", 11, "nbuf:1", _NBUF), ("mt", 12, "nbuf:1", _NBUF), ("mt", 13, "nbuf:1", _NBUF),
    ("mt", 14, "nbuf:1", _NBUF), ("mt", 22, "nbuf:1", _NBUF),
    ("ws", 44, "res:1", "ws_build_fits (conv_f16_ws.hip) leaves the residual form of 44 out: 128 couts x 96 px with residual registers does not "
                        "fit the register file (test_weight_stationary_statistics_builds pins the same list)"),
]


def _reached(family):
    """{variant: classes met in a collected pair}, {variant: kinds}"""
    cls = {v: set() for v in fm.FAMILY_VARIANTS[family]}
    kinds = {v: set() for v in fm.FAMILY_VARIANTS[family]}
    for kind, _, v, _, c in fm.edge_pairs(family):
        cls[v] |= c
        kinds[v].add(kind)
    return cls, kinds


@pytest.mark.parametrize("family", list(fm.FAMILY_CASES))
def test_every_forced_variant_meets_every_class_and_launch_kind_of_its_family(family):
    cls, kinds = _reached(family)
    exempt = {(v, c) for f, v, c, _ in EXEMPT if f == family}
    holes = [(v, c) for v in fm.FAMILY_VARIANTS[family] for c in fm.FAMILY_CLASSES[family] if c not in cls[v] and (v, c) not in exempt]
    assert not holes, f"{family}: (variant, class) no collected pair reaches: {holes}"
    stale = [(v, c) for v, c in exempt if c in cls[v]]
    assert not stale, f"{family}: exempt rows that a collected pair reaches after all (delete them): {stale}"
    no_kind = [(v, k) for v in fm.FAMILY_VARIANTS[family] for k in fm.FAMILY_KINDS[family] if k not in kinds[v]]
    assert not no_kind, f"{family}: (variant, launch kind) without a collected pair: {no_kind}"


def test_edge_matrix_size():
    """Pairs per family, pinned exactly (DESIGN 4.4a records the same counts): a family that stopped serving a case shrinks the matrix,
    one that serves a new pair grows it - either way the count is looked at."""
    got = {family: len(fm.edge_pairs(family)) for family in fm.FAMILY_CASES}
    print(got)
    assert got == {"tile": 251, "mt": 283, "wreg": 310, "wreg_s2": 120, "ws": 57}, got
    # every case of every table is served by some variant of a family that takes the table (the multi-tile kernel has no 1x1
    # stride-2 build: those cases of the shared table are the one-tile family's)
    for family, cases in fm.FAMILY_CASES.items():
        served = {(kind, case) for f, t in fm.FAMILY_CASES.items() if t is cases for kind, case, *_ in fm.edge_pairs(f)}
        assert not [kc for kc in cases if kc not in served], family


@pytest.mark.parametrize("family", sorted({f for f, *_ in EXEMPT}))
def test_exempt_classes_are_out_of_reach(family):
    """No case of the family's search grid (fm.search_grid: maps of every raggedness, N 2 ... 6, channels 8 ... 264, every launch kind)
    puts an exempt variant into its exempt class, under any knob set the pairs are collected with."""
    rows = {}
    for f, v, c, why in EXEMPT:
        if f == family:
            assert len(why) > 40
            rows.setdefault(v, set()).add(c)
    n = {v: 0 for v in rows}
    for kind, case in fm.search_grid(family):
        for env in fm.FAMILY_KNOBS[family]:
            for v, exempt in rows.items():
                got = fm.pair_classes(kind, case, v, family, **env)
                n[v] += got is not None
                assert not (got and got & exempt), f"{family} variant {v} reaches {sorted(got & exempt)} with {kind} {case} under {env}"
    assert min(n.values()) >= 100, f"the grid barely reaches an exempt variant ({n} served cases per variant): it proves nothing"


def test_statistics_cases_keep_their_classes():
    """The cases the statistics tests of tests/test_gpu_bn_fuse.py run on from tests/test_gpu_f16_variants.py reach - with the
    forward-statistics build, under the knob that test sets - a
    short last image group and a ragged last row band on EVERY one-tile and multi-tile variant, and a multi-chunk C8in tail on every
    one-tile variant that has a chunk loop."""
    exempt = {(f, v, c) for f, v, c, _ in EXEMPT}
    for family, variants in (("tile", fm.TILE_VARIANTS), ("mt", fm.MT_VARIANTS)):
        for cls in ("group:ragged", "rows:ragged", "chunks:c8in-tail"):
            if cls not in fm.FAMILY_CLASSES[family]:
                continue
            shown = set()
            for case in fm.STATS_EDGE_CASES:
                for v in variants:
                    w = fm.launch_words(fm.conv_desc(*case), v, 0, 1, MP_F16_MT_GROUPS=7)
                    if w is not None and w["st_mode"] == 1 and cls in fm.classes(w, family, 0):
                        shown.add(v)
            missing = [v for v in variants if v not in shown and (family, v, cls) not in exempt]
            assert not missing, f"{family} {cls}: variants {missing} do not show it on any statistics case with statistics mode 1"


def test_weight_stationary_statistics_builds():
    """Training builds (mp_f16_conv2d_fwd_stats): every weight-stationary shape has the forward-statistics build without a residual
    (what Chain16Fn launches); the builds left out because they do not fit the register file (conv_f16_ws.hip ws_build_fits) are
    exactly: backward statistics of 38 / 39 / 42 / 44, forward statistics + residual of 39 / 42 / 44, and the residual form of 44."""
    got = {}
    for stats, n_res in [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]:
        served = set()
        for g in (2, 5):
            for pr in fm.served_pairs(fm.WS_CASES, fm.WS_VARIANTS, fm.conv_case_desc, lambda c: n_res, stats, MP_F16_WS_GROUPS=g):
                served.add(pr.values[1])
        got[(stats, n_res)] = sorted(set(fm.WS_VARIANTS) - served)
    assert got == {(0, 0): [], (0, 1): [44], (1, 0): [], (1, 1): [39, 42, 44], (2, 0): [38, 39, 42, 44], (2, 1): [38, 39, 42, 44]}, got


def test_four_phase_data_gradient_is_not_offered_by_the_other_families():
    for fam in (fm.WREG_VARIANTS, fm.WS_VARIANTS):
        assert not fm.served_pairs(fm.PHASES4_CASES, fam, fm.phases4_case_desc)


def test_bench_plan_picks_are_still_served():
    """The tuner's choices for the fp16 conv launches of the bench plans (amp-O2 HRNet-W32 N = 128; config 5: HRNet-W48 384x288, 2N = 128;
    the amp-O2 training step N = 128 incl. statistics modes) as recorded on an MI355X: each (shape, variant, residuals, statistics mode)
    must still be accepted by the forced-variant entry.  A kernel that drops out of the candidate set would otherwise only make the
    bench slower under a green suite."""
    path = os.path.join(HERE, "golden", "bench_plan_picks.json")
    with open(path) as fh:
        picks = json.load(fh)
    assert len(picks["f16"]) >= 40
    families = set()
    for pk in picks["f16"]:
        d = fm._lib.ConvDesc(**pk["desc"])
        assert fm.supported(d, pk["variant"], pk["n_res"], pk["stats"]), f"no longer served: {pk}"
        v = pk["variant"]
        families.add("ws" if v in fm.WS_VARIANTS else "wreg" if v in fm.WREG_VARIANTS else "mt" if v in fm.MT_VARIANTS else "tile")
    assert {"ws", "wreg"} <= families, families  # the round-4 kernels carry the bench plans
