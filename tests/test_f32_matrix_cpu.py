"""Floors under the generated (case, tile variant) matrix of the fp32 direct convolution (tests/f32_matrix.py).

tests/test_gpu_conv_variants.py collects only the pairs `mp_conv_supported` reports as served, and what a pair exercises - rows per
tile, image groups, chunk count, staging width, epilogue branch - is decided per launch by `configure()` (csrc/conv_api.hip), so a
change of the tile geometry could move every case of the tables off a code path under a green suite.  These host-only checks read
each served pair's geometry back from the library (`f32_matrix.geometry`: a plan entry on fake pointers, never run) and require,
for EACH of the tile variants 0 ... 7, at least one pair in every class of CLASSES.  The floors are conditions on the tables: when
a geometry moves, a case changes, not a floor.
"""
import functools

import pytest

from tests import f32_matrix as fm


@functools.lru_cache(maxsize=None)
def _geometries(variant):
    """[(id, kind, case, descriptor, geometry)] over every launch of every case the variant serves."""
    out = []
    for kind, ci, case in fm.all_cases():
        if not fm.serves(kind, case, variant):
            continue
        for li, la in enumerate(fm.launches(kind, case)):
            g = fm.geometry(la.desc, variant)
            if g is not None:
                out.append((f"{fm.pair_id(kind, ci, variant)}/{li}", kind, case, la.desc, g))
    return out


def _form(d):
    return f"k{d.kh}" + (f"s{d.stride}" if d.kh in (1, 3) else "")


CLASSES = {
    # name: predicate(kind, case, descriptor, geometry)
    "ragged last row tile": lambda k, c, d, g: g["tiles_y"] > 1 and d.conv_h % g["R"] != 0,
    "ragged last image group": lambda k, c, d, g: g["G"] > 1 and d.n % g["G"] != 0,
    "one chunk": lambda k, c, d, g: g["n_chunks"] == 1,
    "two chunks": lambda k, c, d, g: g["n_chunks"] == 2,
    "odd chunk count >= 3": lambda k, c, d, g: g["n_chunks"] >= 3 and g["n_chunks"] % 2 == 1,
    "vector staging": lambda k, c, d, g: g["vec_staging"],
    "scalar staging": lambda k, c, d, g: not g["vec_staging"],
    "cin % 4 != 0 in several chunks": lambda k, c, d, g: d.cin % 4 != 0 and g["n_chunks"] > 1,
    "cout % CT != 0": lambda k, c, d, g: d.cout % g["ct"] != 0,
    "cout % 16 != 0": lambda k, c, d, g: d.cout % 16 != 0,
    "epilogue plain16": lambda k, c, d, g: g["epilogue"] == "plain16",
    "epilogue whole-image16": lambda k, c, d, g: g["epilogue"] == "whole-image16",
    "epilogue up2": lambda k, c, d, g: g["epilogue"] == "up2",
    "epilogue up4": lambda k, c, d, g: g["epilogue"] == "up4",
    "epilogue up8": lambda k, c, d, g: g["epilogue"] == "up8",
    "epilogue phase": lambda k, c, d, g: g["epilogue"] == "phase",
    "epilogue scalar-plain": lambda k, c, d, g: g["epilogue"] == "scalar-plain",
    "epilogue scalar-up": lambda k, c, d, g: g["epilogue"] == "scalar-up",
    "epilogue scalar-phase": lambda k, c, d, g: g["epilogue"] == "scalar-phase",
    "two residuals": lambda k, c, d, g: fm.n_res(k, c) == 2,
    "k1s1": lambda k, c, d, g: _form(d) == "k1s1",
    "k1s2": lambda k, c, d, g: _form(d) == "k1s2",
    "k2": lambda k, c, d, g: _form(d) == "k2",
    "k3s1": lambda k, c, d, g: _form(d) == "k3s1",
    "k3s2": lambda k, c, d, g: _form(d) == "k3s2",
    # the descriptors only the training step builds
    "pad-0 2x2 phase (reads one row and column past the input)": lambda k, c, d, g: k == "dgrad_k3s2",
    "1x1 scatter into a zeroed gradient": lambda k, c, d, g: k == "dgrad_k1s2",
    "stride-1 data gradient": lambda k, c, d, g: k == "dgrad_s1",
    "transposed-conv data gradient": lambda k, c, d, g: k == "deconv_dgrad",
}
STEM_VARIANTS = (1, 6)  # the tile variants the 7x7 kernel is built for (configure())


@pytest.mark.parametrize("variant", fm.TILE_VARIANTS)
def test_every_tile_variant_meets_every_class(variant):
    geoms = _geometries(variant)
    assert all(g["variant"] == variant for *_, g in geoms)
    missing = [name for name, pred in CLASSES.items() if not any(pred(k, c, d, g) for _, k, c, d, g in geoms)]
    assert not missing, f"variant {variant}: no served pair in the classes {missing}"


@pytest.mark.parametrize("variant", STEM_VARIANTS)
def test_stem_variants_serve_a_7x7_with_a_ragged_row_tile(variant):
    assert any(d.kh == 7 and CLASSES["ragged last row tile"](k, c, d, g) for _, k, c, d, g in _geometries(variant))
    assert not any(d.kh == 7 for v in fm.TILE_VARIANTS if v not in STEM_VARIANTS for *_, d, _ in _geometries(v))


@pytest.mark.parametrize("variant", [-1] + fm.TILE_VARIANTS)
def test_derived_geometry_agrees_with_the_reported_blocks_and_lds(variant):
    """The derived part of `geometry` (rows and pitch of the staged input, chunk count, tile counts) reproduces the block count and
    the LDS bytes the library reports for every launch - the staging width and the class predicates stand on that derivation."""
    geoms = _geometries(variant)
    assert geoms
    wrong = [(name, g) for name, _, _, _, g in geoms if not g["consistent"]]
    assert not wrong, wrong[:4]
    assert all(g["lds"] <= (52 if g["light"] and d.kh <= 3 and g["CK"] > 4 else 150) * 1024 for *_, d, g in geoms)


def test_the_heuristic_serves_every_case():
    unserved = [fm.pair_id(kind, ci, -1) for kind, ci, case in fm.all_cases() if not fm.serves(kind, case, -1)]
    assert not unserved, unserved
    for kind, ci, case in fm.all_cases():  # ... with a tile variant of the direct kernel
        assert all(fm.geometry(la.desc, -1) is not None for la in fm.launches(kind, case)), (kind, case)


def test_every_case_is_served_by_several_tile_variants():
    """Every case is served by at least three tile variants (7x7: the two built), and the other forms (8: streaming 1x1, 10: blocked
    GEMM, 11 / 12: small-problem) enter as extra pairs where they accept a case; no floor on those."""
    for kind, ci, case in fm.all_cases():
        served = [v for v in fm.TILE_VARIANTS if fm.serves(kind, case, v)]
        is_stem = kind == "conv" and case[3] == 7
        assert served == list(STEM_VARIANTS) if is_stem else len(served) >= 3, (kind, case, served)
    assert len(fm.pairs()) >= 8 * len(fm.all_cases()) * 3 // 4
