"""Floors under the generated (band case, variant) matrix of the column-band tests (tests/band_matrix.py).

tests/test_gpu_bands.py collects only the pairs the library reports as served for ALL bands of a case, so a kernel family that stopped
taking band descriptors (out_off_x > 0 inside a wider output, pad_left != pad_top) would shrink the matrix instead of failing it.
These host-only checks pin it from below, and pin which of the SPECIALISED forms take a band at all - a form that starts accepting
bands cannot do so without showing up here, and its pairs then enter the GPU matrix (fp16) or have to be added to it (fp32).
"""
from tests import band_matrix as bm
from tests import f16_matrix as fm

# matrix sizes the library answers at this commit (fp32 forced variants -1 ... 12; fp16 heuristic + one-tile + other families;
# fp16 persistent multi-tile under MP_F16_MT_GROUPS = 1 and 3)
FLOORS = {"fp32": 287, "fp16 one-tile": 390, "fp16 multi-tile": 329}


def test_matrix_sizes_have_a_floor():
    got = {"fp32": len(bm.f32_pairs()), "fp16 one-tile": len(bm.f16_tile_pairs()), "fp16 multi-tile": len(bm.f16_mt_pairs())}
    for name, floor in FLOORS.items():
        assert got[name] >= floor, f"{name}: the served band matrix shrank to {got[name]} pairs (floor {floor})"


def test_every_band_case_is_served_in_fp32_and_in_fp16():
    for kind, case in bm.all_cases():
        assert any(bm.f32_serves(kind, case, v) for v in bm.F32_FORCED if v >= 0), f"no forced fp32 variant takes every band of {kind} {case}"
        assert any(bm.f16_serves(kind, case, v) for v in fm.TILE_VARIANTS + fm.MT_VARIANTS + bm.F16_OTHER) or \
            any(bm.f16_serves(kind, case, v, MP_F16_MT_GROUPS=g) for g in bm.MT_GROUPS for v in fm.MT_VARIANTS), \
            f"no forced fp16 variant takes every band of {kind} {case}"
        # and the library's own heuristic, which is what MINDPOSE_AUTOTUNE=0 plans run
        assert bm.f32_serves(kind, case, -1) and bm.f16_serves(kind, case, -1), f"the heuristic refuses a band of {kind} {case}"


def test_every_tile_variant_serves_a_band_case():
    f32 = {p.values[2] for p in bm.f32_pairs()}
    assert set(bm.F32_TILE_VARIANTS) <= f32, f"fp32 tile variants that take no band case: {sorted(set(bm.F32_TILE_VARIANTS) - f32)}"
    tile = {p.values[2] for p in bm.f16_tile_pairs()}
    assert set(fm.TILE_VARIANTS) <= tile, f"fp16 one-tile variants that take no band case: {sorted(set(fm.TILE_VARIANTS) - tile)}"
    for g in bm.MT_GROUPS:
        mt = {p.values[3] for p in bm.f16_mt_pairs() if p.values[0] == str(g)}
        assert set(fm.MT_VARIANTS) <= mt, f"fp16 multi-tile variants that take no band case (groups {g}): {sorted(set(fm.MT_VARIANTS) - mt)}"


def test_the_specialised_forms_that_accept_a_band_are_exactly_these():
    """fp32: the streaming 1x1, small-problem and Winograd forms refuse every band descriptor of the tables; the blocked-GEMM form
    (10) takes single phase bands of the 64 -> 128 transposed conv (those whose conv_w == w) but never all bands of a case, so it
    has no pair in the matrix.  fp16: the weight-stationary family refuses; six weights-in-registers variants take the bands of the
    1x1 layers (no halo column, so pad_left never matters to them) - their pairs ARE in the matrix."""
    assert bm.other_forms_accepting_a_band() == {"f32": [10], "winograd": False, "f16": [25, 27, 31, 33, 34, 36]}
    assert not [p for p in bm.f32_pairs() if p.values[2] in bm.F32_OTHER_FORMS or p.values[2] == 9]
    in_matrix = {p.values[2] for p in bm.f16_tile_pairs()} & set(bm.F16_OTHER)
    assert in_matrix == {25, 27, 31, 33, 34, 36}, in_matrix
    for p in bm.f16_tile_pairs():
        kind, case, v = p.values
        if v in bm.F16_OTHER:
            assert kind == "conv" and case[3] == 1, f"a weights-in-registers variant took a band with a halo: {case} v{v}"


def test_the_tables_hold_the_alignment_case():
    """A band whose width is a multiple of 4 at a column offset inside an output whose width is not: rows of the band alternate
    between 16-byte and 8-byte alignment (even output width) or run through all four 4-byte alignments (odd output width) in fp32,
    with one and with two residual tensors."""
    hit = set()
    for case in bm.BAND_CASES:
        for _, _, d in bm.conv_case_bands(case):
            if d.conv_w % 4 == 0 and d.out_w % 4 != 0 and d.out_off_x > 0:
                hit.add((case[8], 4 if d.out_w % 2 else 8))  # (residuals, alignment in bytes of the odd rows)
    assert {(1, 8), (2, 8), (1, 4), (2, 4)} <= hit, hit


def test_the_gemm_form_is_reached_band_by_band():
    """Variant 10 serves no whole case (see above), so tests/test_gpu_bands.py runs it per band: the assignment must hold both."""
    assign = bm.gemm_band_variants()
    assert sorted(set(assign.values())) == [-1, 10], assign
