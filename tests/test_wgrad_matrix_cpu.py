"""The weight-gradient case tables (tests/wgrad_matrix.py) reach the paths they are there for.

Every row names its properties - kernel or form, tiles per workgroup, short tile into a used buffer, k-steps, LDS buffers, reduce
kernel and tail; they are recomputed here from the restated geometry, and the restatement is held against the library's own
workspace queries (host-only: no GPU).  A geometry change that moves a row off its path fails here and names the row.
"""
import pytest

from tests import wgrad_matrix as wm

F32 = [pytest.param(c, k, want, id=wm.case_id(c, k)) for c, k, want in wm.F32_CASES]
F16 = [pytest.param(c, k, want, id=wm.case_id(c, k)) for c, k, want in wm.F16_CASES]


def _geo32(case, knobs):
    return wm.geometry32(*case, simple=knobs.get("MP_WGRAD_SIMPLE") == "1")


def _geo16(case, knobs, n_jobs=1):
    return wm.geometry16(*case, n_jobs=n_jobs, **wm.geo16_kwargs(knobs))


def _check_common(geo, want, per_wg, cin, cout):
    if "reduce" in want:
        assert (geo.reduce, geo.reduce_rounds, geo.reduce_tail) == (want["reduce"], want["rounds"], want["tail"])
        assert geo.reduce_tail[1] > 0, "the reduce row must run the tail loop"
    else:
        assert max(per_wg) >= 3, "a buffer is refilled only from the third tile of a workgroup on"
    if "R" in want:
        assert geo.R == want["R"]
    if "rows" in want:
        assert geo.rows == want["rows"]
    if "splits" in want:
        assert geo.splits == want["splits"]
    assert wm.stale_short_tile(geo) or not want.get("stale"), "no short tile lands in a buffer that held a full one"
    if want.get("ragged_channels"):
        assert cin % 32 or cout % 32


@pytest.mark.parametrize("case,knobs,want", F32)
def test_fp32_row_reaches_its_path(case, knobs, want):
    geo = _geo32(case, knobs)
    assert geo.splits == wm.lib_splits32(case, **knobs)
    wm.check_geometry_against_launch(geo, wm.launch_words(case, 0, **knobs), 0)
    per_wg = tuple(len(t) for t in geo.tile_lists)
    _check_common(geo, want, per_wg, case[1], case[2])
    if "kernel" in want:
        assert geo.kernel == want["kernel"]
    if "n_tiles" in want:
        assert geo.n_tiles == want["n_tiles"]
    if "per_wg" in want:
        assert per_wg == want["per_wg"]
    if want.get("forced"):
        assert wm.geometry32(*case).kernel == "pipe", "MP_WGRAD_SIMPLE must change the kernel of this row"


@pytest.mark.parametrize("case,knobs,want", F16)
def test_fp16_row_reaches_its_path(case, knobs, want):
    geo = _geo16(case, knobs)
    assert geo.splits == wm.lib_splits16(case, **wm.env16(knobs))
    wm.check_geometry_against_launch(geo, wm.launch_words(case, 1, **wm.env16(knobs)), 1)
    per_split = tuple(len(t) for t in geo.tile_lists)
    assert per_split == (geo.tiles_per_split,) * (geo.splits - 1) + (geo.last_split,)
    _check_common(geo, want, per_split, case[1], case[2])
    for key in ("form", "planes", "tiles", "ksteps", "nbuf"):
        if key in want:
            assert getattr(geo, key) == want[key], key
    if "per_split" in want:
        assert per_split == want["per_split"]
    # a knob that switches a form off must change the form of its row
    plain = {k: v for k, v in knobs.items() if k == "WGS"}
    if len(plain) < len(knobs):
        other = _geo16(case, plain)
        assert (other.form, other.planes) != (geo.form, geo.planes)


@pytest.mark.parametrize("case,knobs,jobs", wm.F16_GROUPED_CASES, ids=[wm.case_id(c, k) for c, k, _ in wm.F16_GROUPED_CASES])
def test_fp16_grouped_row_reaches_its_path(case, knobs, jobs):
    geo = _geo16(case, knobs, jobs)
    assert geo.splits == wm.lib_splits16(case, jobs, **wm.env16(knobs))
    wm.check_geometry_against_launch(geo, wm.launch_words(case, 1, jobs, **wm.env16(knobs)), 1)
    assert geo.tiles_per_split >= 3 and wm.stale_short_tile(geo)


def test_fp32_table_hits_every_targeted_condition():
    geos = [(_geo32(c, k), k) for c, k, _ in wm.F32_CASES]
    long_run = [(g.kernel, g.k, g.s) for g, _ in geos if wm.max_tiles_per_workgroup(g) >= 3]
    for ks in ((1, 1), (1, 2), (3, 1), (3, 2)):
        assert ("pipe",) + ks in long_run, ks
        assert any(g.kernel == "pipe" and (g.k, g.s) == ks and (wm.stale_short_tile(g) or ks == (1, 1)) for g, _ in geos), ks
    for ks in ((1, 1), (1, 2), (3, 1), (3, 2), (4, 2)):
        assert ("simple",) + ks in long_run, ks
    assert any(k and g.kernel == "simple" and wm.max_tiles_per_workgroup(g) >= 3 for g, k in geos)  # MP_WGRAD_SIMPLE
    assert any(len({len(t) for t in g.tile_lists}) > 1 for g, _ in geos)  # uneven split
    for name in ("grouped16", "grouped4", "plain"):
        assert any(g.reduce == name and g.reduce_rounds >= 1 and g.reduce_tail[1] > 0 for g, _ in geos), name


def test_fp16_table_hits_every_targeted_condition():
    geos = [_geo16(c, k) for c, k, _ in wm.F16_CASES]
    long_run = {(g.form, g.k, g.s, g.planes) for g in geos if g.tiles_per_split >= 3}
    kernels = {(f, k, s) for f, k, s, _ in long_run}
    for want in [("dma32", 1, 1), ("dma32", 1, 2), ("dma32", 3, 1), ("dma32", 3, 2), ("dma32", 4, 2), ("wide", 1, 1), ("wide", 1, 2),
                 ("wide", 3, 1), ("wide", 3, 2), ("narrow", 3, 1), ("narrow", 3, 2), ("reg", 1, 1), ("reg", 1, 2), ("reg", 3, 1),
                 ("reg", 3, 2), ("reg", 4, 2)]:
        assert want in kernels, want
    for form in ("dma32", "wide", "narrow"):  # stride 2 as parity planes and as one linear image
        assert (form, 3, 2, True) in long_run and (form, 3, 2, False) in long_run, form
    for form in ("dma32", "wide", "narrow", "reg"):
        assert any(g.form == form and wm.stale_short_tile(g) and g.tiles_per_split >= 3 for g in geos), form
    assert any(g.form == "reg" and g.nbuf == 1 and g.tiles_per_split >= 3 for g in geos)
    assert any(g.form == "reg" and g.nbuf == 2 and g.tiles_per_split >= 3 for g in geos)
    wide_ksteps = {g.ksteps for g in geos if g.form == "wide" and g.tiles_per_split >= 3}
    assert 1 in wide_ksteps, "single k-step only"
    assert any(k % 2 == 0 for k in wide_ksteps), "pairs only"
    assert any(k % 2 == 1 and k >= 3 for k in wide_ksteps), "pairs plus the single-step tail"
    assert any(g.last_split != g.tiles_per_split for g in geos)  # uneven split
    assert any(g.reduce == "grouped16" and g.splits % 64 and g.reduce_tail[1] > 0 for g in geos)


def test_restated_geometry_agrees_with_the_library_on_random_shapes():
    """Split counts of both restatements against the workspace queries, every form switch and the grouped query included; form,
    tile rows, k-steps, pitch, buffers, planes, tiles per split, LDS bytes and reduce kernel against the launch words."""
    forms = set()
    for case, simple, knobs, jobs in wm.random_draws(600):
        env32 = {"MP_WGRAD_SIMPLE": "1"} if simple else {}
        geo = wm.geometry32(*case, simple=simple)
        assert (geo.splits if geo else 0) == wm.lib_splits32(case, **env32), (case, simple)
        wm.check_geometry_against_launch(geo, wm.launch_words(case, 0, **env32), 0)
        geo = _geo16(case, knobs, jobs)
        assert (geo.splits if geo else 0) == wm.lib_splits16(case, jobs, **wm.env16(knobs)), (case, knobs, jobs)
        wm.check_geometry_against_launch(geo, wm.launch_words(case, 1, 0 if jobs == 1 else jobs, **wm.env16(knobs)), 1)
        if geo:
            forms.add((geo.form, geo.planes, geo.nbuf))
    assert {f for f, _, _ in forms} == {"dma32", "wide", "narrow", "reg"} and ("reg", False, 1) in forms


@pytest.mark.parametrize("case,half,bound", [((50, 32, 32, 3, 1, 16, 12), False, 5e-5), ((5, 72, 136, 3, 2, 40, 24), True, 1e-4),
                                             ((7, 72, 80, 1, 2, 44, 12), True, 1e-4)])
def test_one_dropped_tile_is_far_outside_the_bound(case, half, bound):
    """The rows with the MOST tiles (each tile the smallest share of the gradient): losing the last tile moves the float64
    reference by more than 100 times the bound the GPU test allows."""
    n, cin, cout, k, s, h, w = case
    geo = wm.geometry16(*case, wgs=8) if half else wm.geometry32(*case)
    x, dz, ref = wm.operands(case, half)
    rows = geo.rows[-1]
    dropped = dz.clone()
    dropped[n - 1, :, geo.ho - rows:] = 0
    moved = float((wm.reference_dw(x, dropped, k, s, wm.out_hw(k, s, h, w)[0]) - ref).abs().max() / ref.abs().max())
    assert moved > 100 * bound, moved


def test_reference_dw_is_the_definition():
    """reference_dw against the defining sum, written out, on a shape small enough for it."""
    import torch
    g = torch.Generator().manual_seed(3)
    for k, s, h, w in ((3, 2, 5, 6), (1, 2, 4, 3), (4, 2, 6, 4), (3, 1, 3, 4)):
        pad, ho, wo = wm.out_hw(k, s, h, w)
        x, dz = torch.randn(2, 3, h, w, generator=g).double(), torch.randn(2, 2, ho, wo, generator=g).double()
        want = torch.zeros(2, 3, k, k, dtype=torch.float64)
        for ky in range(k):
            for kx in range(k):
                for y in range(ho):
                    for xo in range(wo):
                        yi, xi = y * s + ky - pad, xo * s + kx - pad
                        if 0 <= yi < h and 0 <= xi < w:
                            want[:, :, ky, kx] += torch.einsum("no,ni->oi", dz[:, :, y, xo], x[:, :, yi, xi])
        got = wm.reference_dw(x, dz, k, s, pad)
        assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-12
