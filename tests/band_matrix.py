"""The (band case, kernel variant) matrix of the column-band tests, generated from the library's own answer.

A layer wider than every kernel's pixel tile runs as output-column bands (mindpose_amd/models/layers.py `conv_column_bands`,
`deconv_phase_column_bands`).  A band is an `mp_conv_desc` with `out_off_x > 0` inside a wider output, `pad_left !=
pad_top` and an input buffer of its own.  BAND_CASES / DECONV_BAND_CASES are whole layers with a band count; a (case, variant) pair
enters the matrix when the library answers "served" (`mp_conv_supported` / `mp_f16_conv_supported`, host-only) for ALL bands of the
case.  Nothing is skipped: a collected pair that fails to launch fails.  tests/test_band_matrix_cpu.py holds the floors,
tests/test_gpu_bands.py runs every pair against the unbanded layer.
"""
import ctypes
import functools

import pytest

from mindpose_amd import _lib
from mindpose_amd.models.layers import conv_column_bands, deconv_phase_column_bands
from tests import f16_matrix as fm

BAND_CASES = [
    # n, cin, cout, k, s, h, w, relu, n_res, nb  (pad = k // 2; h cut to 8 ... 16 rows: the width is what matters)
    (1, 32, 32, 3, 1, 12, 416, True, 1, 5),    # HigherHRNet head BasicBlock conv + residual, 832-pixel image: 84 x 4 + 80
    (1, 32, 32, 3, 1, 12, 416, True, 1, 3),    # ... in the three bands the fp32 plan takes: 139 / 139 / 138
    (1, 32, 32, 3, 1, 12, 256, True, 1, 3),    # ... 512-pixel image: 86 / 86 / 84
    (1, 32, 17, 1, 1, 12, 416, False, 0, 5),   # final_layers.1: 17 couts + bias
    (1, 3, 64, 3, 2, 16, 832, True, 0, 5),     # stem conv1 on the 832-pixel image (3 channels in one block)
    (1, 64, 64, 3, 2, 16, 416, True, 0, 3),    # stem conv2: 70 / 70 / 68 output columns
    (1, 64, 256, 1, 1, 8, 208, True, 1, 3),    # stage-1 expand conv + identity
    (1, 256, 64, 1, 1, 8, 208, True, 0, 3),    # stage-1 reduce conv
    (1, 256, 64, 3, 2, 8, 208, True, 0, 4),    # transition1.1 (3x3 stride 2)
    (1, 48, 48, 3, 1, 8, 208, True, 1, 3),     # W48 branch 0
    (1, 96, 96, 3, 1, 8, 208, True, 1, 3),     # W48 widths, 96 channels
    (1, 48, 96, 3, 2, 8, 208, True, 0, 4),     # W48 transition
    # synthetic: narrow layers forced into bands, served by many variants
    (2, 16, 16, 3, 1, 8, 40, True, 1, 3),      # 14 / 14 / 12
    (3, 16, 24, 3, 2, 9, 50, True, 0, 2),      # stride 2: 13 / 12 output columns
    (2, 8, 17, 3, 1, 8, 27, False, 0, 4),      # 7 / 7 / 7 / 6, 17 couts
    (2, 8, 17, 3, 1, 8, 27, False, 0, 5),      # 6 x 4 + 3: a last band three columns wide
    (2, 16, 16, 3, 1, 8, 26, True, 1, 6),      # 5 x 5 + 1: a last band ONE column wide
    (7, 16, 16, 3, 1, 4, 40, True, 2, 3),      # n not a multiple of the image group, two residuals
    (2, 5, 40, 3, 2, 9, 51, True, 0, 2),       # odd input width under stride 2, cin 5, cout 40
    (2, 5, 40, 1, 1, 9, 27, True, 0, 5),       # 1x1 with ragged channels, last band 3 wide
    (4, 32, 32, 3, 1, 16, 40, True, 1, 3),     # enough tiles for long runs of the persistent multi-tile kernel
    (3, 16, 24, 3, 2, 9, 50, False, 2, 5),     # stride 2 in five bands of 5, two residuals
    # the alignment case: band width a multiple of 4 inside an output whose width is not - every other row of a band starts at an
    # address that is only 8-byte aligned (the fp32 epilogue's 16-byte path, csrc/conv_mfma.h vec_ok)
    (1, 32, 32, 3, 1, 8, 250, True, 1, 3),     # 84 / 84 / 82
    (1, 32, 32, 3, 1, 8, 250, True, 2, 3),
    (2, 16, 16, 3, 1, 8, 30, True, 1, 4),      # small twin: 8 / 8 / 8 / 6
    (2, 16, 16, 3, 1, 8, 30, True, 2, 4),
    (2, 16, 16, 3, 1, 7, 26, True, 1, 7),      # 4 x 6 + 2, odd row count
    (2, 16, 17, 1, 1, 8, 30, False, 1, 4),     # 1x1 + residual
    # ... and an ODD output width (4 x 6 + 3 of 27 columns): band rows that are only 4-byte aligned.  No recipe width gives this
    # (they are multiples of 16); it is the worst alignment the descriptor allows
    (2, 16, 16, 3, 1, 7, 27, True, 1, 7),
    (2, 16, 16, 3, 1, 7, 27, True, 2, 7),
]

DECONV_BAND_CASES = [
    # n, cin, cout, h, w, relu, nb - Conv2dTranspose(k=4, s=2, p=1) as four 2x2 phase convs, each in nb input-column bands
    (1, 66, 32, 8, 208, True, 3),    # HigherHRNet deconv layer (32 + 17 + 17 channels: cin not a multiple of 8), 832-pixel image
    (1, 66, 32, 8, 128, True, 2),    # ... 512-pixel image
    (2, 64, 128, 8, 40, True, 3),    # blocked-GEMM widths (cin % 16 == 0, cout >= 96)
    (2, 16, 24, 6, 27, False, 4),    # ragged: 7 / 7 / 7 / 6
]

F32_TILE_VARIANTS = list(range(8))          # cout tile x pixel tile builds of the direct kernel (csrc/conv_mfma.h)
F32_OTHER_FORMS = {8: "streaming 1x1", 10: "blocked GEMM", 11: "small-problem", 12: "small-problem wide"}
F32_FORCED = [-1] + list(range(13))         # what mp_conv2d_fwd_variant takes (9 is the tuner's index of the Winograd form)
MT_GROUPS = (1, 3)                          # MP_F16_MT_GROUPS, as test_conv_f16_multi_tile_vs_oracle sets it
F16_OTHER = fm.WREG_VARIANTS + fm.WS_VARIANTS


@functools.lru_cache(maxsize=None)
def conv_case_bands(case):
    """[(start, width_in, ConvDesc)] of a BAND_CASES entry."""
    n, cin, cout, k, s, h, w, relu, _, nb = case
    return conv_column_bands(n, cin, h, w, cout, k, s, k // 2, relu, nb)


@functools.lru_cache(maxsize=None)
def deconv_case_bands(case):
    """{(py, px): [(start, width_in, ConvDesc)]} of a DECONV_BAND_CASES entry."""
    n, cin, cout, h, w, relu, nb = case
    return {(py, px): deconv_phase_column_bands(n, cin, h, w, cout, py, px, relu, nb) for py in (0, 1) for px in (0, 1)}


def case_descs(kind, case):
    if kind == "conv":
        return [d for _, _, d in conv_case_bands(case)]
    return [d for bands in deconv_case_bands(case).values() for _, _, d in bands]


def case_res(kind, case):
    return case[8] if kind == "conv" else 0


def all_cases():
    return [("conv", c) for c in BAND_CASES] + [("deconv", c) for c in DECONV_BAND_CASES]


def f32_supported(d, variant) -> bool:
    return _lib.load().mp_conv_supported(ctypes.byref(d), int(variant)) == 1


def f32_serves(kind, case, variant) -> bool:
    return all(f32_supported(d, variant) for d in case_descs(kind, case))


def f16_serves(kind, case, variant, **env) -> bool:
    return all(fm.supported(d, variant, case_res(kind, case), 0, **env) for d in case_descs(kind, case))


def _id(kind, ci, variant, extra=""):
    return f"{kind}{ci}-{extra}v{variant}" if variant >= 0 else f"{kind}{ci}-{extra}heuristic"


def _indexed():
    return [(kind, ci, case) for kind, cases in (("conv", BAND_CASES), ("deconv", DECONV_BAND_CASES)) for ci, case in enumerate(cases)]


def f32_pairs():
    """(kind, case, variant): fp32, every forced variant -1 ... 12 that serves all bands of the case."""
    return [pytest.param(kind, case, v, id=_id(kind, ci, v)) for kind, ci, case in _indexed() for v in F32_FORCED
            if f32_serves(kind, case, v)]


def f16_tile_pairs():
    """fp16: the heuristic, the one-tile family and every variant of another family (weights in registers, weight-stationary)
    that takes all bands of the case."""
    return [pytest.param(kind, case, v, id=_id(kind, ci, v)) for kind, ci, case in _indexed()
            for v in [-1] + fm.TILE_VARIANTS + F16_OTHER if f16_serves(kind, case, v)]


def f16_mt_pairs():
    """fp16 persistent multi-tile family under MP_F16_MT_GROUPS = 1 and 3: (groups, kind, case, variant)."""
    return [pytest.param(str(g), kind, case, v, id=_id(kind, ci, v, f"g{g}-")) for g in MT_GROUPS for kind, ci, case in _indexed()
            for v in fm.MT_VARIANTS if f16_serves(kind, case, v, MP_F16_MT_GROUPS=g)]


GEMM_BAND_CASE = DECONV_BAND_CASES[2]  # 64 -> 128: the widths the blocked-GEMM phase form is built for


def gemm_band_variants(case=GEMM_BAND_CASE):
    """{(py, px, band index): 10 or -1}: the blocked-GEMM form (fp32 variant 10) takes single phase bands - those whose conv_w equals
    their input width - never all bands of a case, so it has no pair in the matrix; the plan's tuner can still pick it for such a
    band.  This is the per-band assignment that reaches it: variant 10 where the library answers yes, the heuristic elsewhere."""
    return {(py, px, bi): (10 if f32_supported(d, 10) else -1)
            for (py, px), bands in deconv_case_bands(case).items() for bi, (_, _, d) in enumerate(bands)}


def other_forms_accepting_a_band():
    """The specialised forms that accept at least one single band DESCRIPTOR of the tables today: {"f32": [variant ids],
    "winograd": bool, "f16": [variant ids]}."""
    lib = _lib.load()
    descs = [(d, case_res(kind, case)) for kind, case in all_cases() for d in case_descs(kind, case)]
    return {
        "f32": sorted(v for v in F32_OTHER_FORMS if any(f32_supported(d, v) for d, _ in descs)),
        "winograd": any(lib.mp_conv_winograd_supported(ctypes.byref(d)) == 0 for d, _ in descs),
        "f16": sorted(v for v in F16_OTHER if any(fm.supported(d, v, r, 0) for d, r in descs)),
    }
