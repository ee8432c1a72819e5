"""The (case, tile variant) matrix of the fp32 direct convolution (csrc/conv_mfma.h), generated from the library's own answer.

A case is a layer in one of seven KINDS; the kind decides the launches (`launches`: descriptor, weight packing, where the result
accumulates) and the fp64 reference tests/test_gpu_conv_variants.py compares with:

    conv          k 1 / 3 stride 1 / 2 and the 7x7 stride-2 stem, "same" padding, 0 ... 2 residuals, ReLU          packing 0
    up            1x1 + nearest up-sampling by out_mul = out_rep = 2 / 4 / 8 + two residuals + ReLU (HRModule fuse)  packing 0
    deconv        Conv2dTranspose(4, 2, 1) as four 2x2 phase convs, pad (1 - py, 1 - px), out_mul 2, offset (py, px) packing 1
    dgrad_s1      data gradient of a stride-1 conv: pad k - 1 - p, roles swapped                                      packing 2
    dgrad_k3s2    data gradient of a 3x3 stride-2 conv: four 2x2 pad-0 phases, out_mul 2, offset (py, px)            packing 3
    dgrad_k1s2    data gradient of a 1x1 stride-2 conv: 1x1 with out_mul 2 into a zero-filled tensor                  packing 2
    deconv_dgrad  data gradient of the transposed conv: four 2x2 phases, pad (py, px), summed through res1            packing 4

The descriptors are the ones mindpose_amd/models/layers.py and train_ops.py build (`_conv_dgrad`, `_deconv_forward`,
`_deconv_backward`).  A (case, variant) pair enters the matrix when `mp_conv_supported` (host-only) answers "served" for EVERY launch
of the case, for the heuristic (-1) and the forced variants 0 ... 12.  Nothing is skipped: a collected pair whose launch fails, fails.
`geometry` reads a served launch's tile geometry back from the library (`mp_plan_add_conv_variant` on fake pointers +
`mp_plan_entry_info`) and derives the chunk count, the staging width and the epilogue branch from it; tests/test_f32_matrix_cpu.py
holds the floors: every tile variant 0 ... 7 meets every class of geometry in at least one pair.
"""
import ctypes
import functools

import pytest

from mindpose_amd import _lib

TILE_VARIANTS = list(range(8))        # cout tile x pixel tile builds of the direct kernel (csrc/conv_mfma.h ConvVariant)
FORCED = [-1] + list(range(13))       # what mp_conv2d_fwd_variant takes: 8 streaming 1x1, 10 blocked GEMM, 11 / 12 small-problem
PHASES = [(0, 0), (0, 1), (1, 0), (1, 1)]

CONV_CASES = [
    # n, cin, cout, k, s, h, w, relu, n_res
    (2, 24, 24, 3, 1, 19, 20, True, 1),    # ragged last row tile (19 rows in tiles of 9 or 4), 2 ... 6 chunks
    (7, 16, 16, 3, 1, 4, 4, True, 2),      # image groups of 12 / 6: 7 images leave a ragged last group
    (5, 256, 80, 3, 1, 8, 6, True, 1),     # 8x6 map: the whole-image 16-byte epilogue, 16 ... 64 chunks, cout 80 = 64 + 16 = 48 + 32
    (3, 20, 40, 3, 1, 11, 13, False, 2),   # odd width: scalar staging + the scalar epilogue, five chunks
    (2, 36, 72, 3, 2, 21, 28, True, 0),    # stride 2, Wo = 14: vector staging with the scalar epilogue
    (3, 10, 24, 3, 2, 15, 11, True, 1),    # cin % 4 != 0 in three chunks
    (2, 136, 17, 1, 1, 10, 12, False, 0),  # 1x1 head widths: 17 couts, up to 17 chunks, ragged row tile on the 96-pixel variants
    (2, 64, 96, 1, 2, 17, 16, True, 2),    # 1x1 stride 2 (ResNet down-sample), odd height
    (3, 8, 40, 1, 2, 10, 6, False, 0),     # ... on a 5x3 output: image groups under stride 2
    (2, 3, 64, 7, 2, 40, 32, True, 0),     # 7x7 stem, 20 x 16 output: ragged row tile on the 192-pixel variants that build it
    (2, 16, 16, 3, 1, 10, 14, True, 1),    # 140 pixels: whole-image 16-byte epilogue on the 192-pixel variants, scalar on the 96s
    (3, 4, 17, 3, 1, 6, 8, False, 1),      # ONE chunk of one cin quad
    (2, 8, 16, 1, 1, 8, 8, True, 0),       # two chunks at most, cout a single 16-wide sub-tile
    (3, 6, 24, 3, 1, 9, 8, True, 2),       # cin 6 -> 8: a half-empty second quad, row tiles of a 9-row map
    (2, 12, 40, 3, 2, 16, 16, False, 1),   # 3x3 stride 2, 12 input channels: an odd chunk count where CK = 4
]

UP_CASES = [
    # n, cin, cout, h, w, factor - the 1x1 conv of an HRModule fuse row, up-sampled into the sum of the row
    (2, 64, 32, 8, 12, 2),
    (2, 128, 32, 6, 8, 4),
    (3, 256, 32, 2, 4, 8),
    (2, 96, 48, 5, 6, 2),      # Wo = 6: the scalar path with the up-sample mapping
    (2, 20, 17, 9, 16, 2),     # ragged row tile + 17 couts through the up-sample epilogue
]

DECONV_CASES = [
    # n, cin, cout, h, w, relu
    (3, 20, 24, 5, 8, True),
    (3, 20, 24, 5, 7, False),  # Wo = 7: the scalar path with the phase mapping
    (1, 66, 32, 16, 24, True), # the HigherHRNet deconv widths (32 + 17 + 17 channels in)
]

DGRAD_S1_CASES = [
    # n, cin, cout, k, h, w, n_res - of the FORWARD conv (pad k // 2): the launch reads dz [n, cout, h, w] and writes dx [n, cin, h, w]
    (2, 24, 40, 3, 13, 12, 1),
    (3, 17, 32, 1, 6, 10, 0),
    (2, 16, 6, 3, 9, 8, 1),    # 6 forward couts = 6 kernel input channels
]

DGRAD_K3S2_CASES = [
    # n, cin, cout, h, w - of the forward 3x3 stride-2 pad-1 conv (even h, w): dz [n, cout, h / 2, w / 2] -> dx [n, cin, h, w]
    (2, 24, 36, 10, 16),
    (3, 16, 10, 14, 10),       # Wo = 5: scalar epilogue; 10 kernel input channels
    (2, 32, 64, 42, 24),       # 21 x 12 phases: ragged last row tile under the pad-0 2x2 window (reads row 21 = the halo)
]

DGRAD_K1S2_CASES = [
    # n, cin, cout, h, w - of the forward 1x1 stride-2 conv
    (2, 40, 64, 12, 16),
    (3, 24, 10, 10, 6),
]

DECONV_DGRAD_CASES = [
    # n, cin, cout, h, w - of the forward transposed conv: dy [n, cout, 2h, 2w] -> dx [n, cin, h, w]
    (2, 34, 32, 6, 8),
    (3, 24, 10, 5, 7),
]

KINDS = [("conv", CONV_CASES), ("up", UP_CASES), ("deconv", DECONV_CASES), ("dgrad_s1", DGRAD_S1_CASES),
         ("dgrad_k3s2", DGRAD_K3S2_CASES), ("dgrad_k1s2", DGRAD_K1S2_CASES), ("deconv_dgrad", DECONV_DGRAD_CASES)]
TRAIN_FLAGS = _lib.MP_CONV_SHARES_CUS  # what train_ops.py sets on every descriptor of a training step


def _desc(n, cin, h, w, cout, k, s, pad_t, pad_l, conv_h, conv_w, out_h, out_w, out_mul=1, out_rep=1, off_y=0, off_x=0, relu=0, flags=0):
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=s, pad_top=pad_t, pad_left=pad_l, conv_h=conv_h,
                         conv_w=conv_w, out_h=out_h, out_w=out_w, out_mul=out_mul, out_rep=out_rep, out_off_y=off_y, out_off_x=off_x,
                         relu=int(relu), flags=flags)


class Launch:
    """One kernel launch of a case.  ``accumulate``: res1 is the case's own output so far (the phases of deconv_dgrad)."""

    def __init__(self, desc, transposed, py=0, px=0, accumulate=False):
        self.desc, self.transposed, self.py, self.px, self.accumulate = desc, transposed, py, px, accumulate


@functools.lru_cache(maxsize=None)
def launches(kind, case):
    if kind == "conv":
        n, cin, cout, k, s, h, w, relu, _ = case
        p = k // 2
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        return [Launch(_desc(n, cin, h, w, cout, k, s, p, p, ho, wo, ho, wo, relu=relu), 0)]
    if kind == "up":
        n, cin, cout, h, w, f = case
        return [Launch(_desc(n, cin, h, w, cout, 1, 1, 0, 0, h, w, h * f, w * f, out_mul=f, out_rep=f, relu=1), 0)]
    if kind == "deconv":
        n, cin, cout, h, w, relu = case
        return [Launch(_desc(n, cin, h, w, cout, 2, 1, 1 - py, 1 - px, h, w, 2 * h, 2 * w, out_mul=2, off_y=py, off_x=px, relu=relu), 1, py, px)
                for py, px in PHASES]
    if kind == "dgrad_s1":
        n, cin, cout, k, h, w, _ = case
        p = k // 2
        return [Launch(_desc(n, cout, h, w, cin, k, 1, k - 1 - p, k - 1 - p, h, w, h, w, flags=TRAIN_FLAGS), 2)]
    if kind == "dgrad_k3s2":
        n, cin, cout, h, w = case
        ho, wo = h // 2, w // 2
        return [Launch(_desc(n, cout, ho, wo, cin, 2, 1, 0, 0, ho, wo, h, w, out_mul=2, off_y=py, off_x=px, flags=TRAIN_FLAGS), 3, py, px)
                for py, px in PHASES]
    if kind == "dgrad_k1s2":
        n, cin, cout, h, w = case
        ho, wo = h // 2, w // 2
        return [Launch(_desc(n, cout, ho, wo, cin, 1, 1, 0, 0, ho, wo, h, w, out_mul=2, flags=TRAIN_FLAGS), 2)]
    if kind == "deconv_dgrad":
        n, cin, cout, h, w = case
        return [Launch(_desc(n, cout, h, w, cin, 2, 1, py, px, h, w, h, w, flags=TRAIN_FLAGS), 4, py, px, accumulate=(py, px) != (0, 0))
                for py, px in PHASES]
    raise ValueError(kind)


def n_res(kind, case):
    """Residual tensors of the case's epilogue that are operands (the running sum of deconv_dgrad is not one)."""
    return {"conv": lambda: case[8], "up": lambda: 2, "dgrad_s1": lambda: case[6]}.get(kind, lambda: 0)()


def supported(d, variant) -> bool:
    return _lib.load().mp_conv_supported(ctypes.byref(d), int(variant)) == 1


def serves(kind, case, variant) -> bool:
    return all(supported(la.desc, variant) for la in launches(kind, case))


def all_cases():
    return [(kind, ci, case) for kind, cases in KINDS for ci, case in enumerate(cases)]


def pair_id(kind, ci, variant):
    return f"{kind}{ci}-v{variant}" if variant >= 0 else f"{kind}{ci}-heuristic"


def pairs(variants=FORCED):
    """(kind, case, variant) pytest params: every forced variant that serves all launches of the case."""
    return [pytest.param(kind, case, v, id=pair_id(kind, ci, v)) for kind, ci, case in all_cases() for v in variants if serves(kind, case, v)]


# ---- a served launch's geometry, read back from the library ---------------------------------------------------------------------

def _round_up(v, m):
    return (v + m - 1) // m * m


def _plane_pad(raw):
    """Smallest value >= raw that is 16 mod 32 (the LDS cin-plane stride, csrc/conv_api.hip plane_pad)."""
    v = raw + (16 - raw) % 32
    assert v >= raw and v % 32 == 16 and v - 32 < raw
    return v


def epilogue_branch(d, R):
    """Which branch of the epilogue of csrc/conv_mfma.h a launch ends in, from the descriptor and the rows per tile R.
    Restates `vec_ok` (conv_mfma.h, "const bool vec_ok =" at the top of the epilogue) and the if-chain below it."""
    whole_image = (R == d.conv_h and (d.conv_h * d.conv_w) % 4 == 0 and d.out_mul == 1 and d.out_rep == 1 and d.out_w == d.conv_w and
                   d.out_h == d.conv_h and d.out_off_x == 0 and d.out_off_y == 0)
    vec_ok = d.conv_w % 4 == 0 or whole_image
    mapping = "plain" if d.out_mul == 1 and d.out_rep == 1 else f"up{d.out_rep}" if d.out_rep == d.out_mul and d.out_rep in (2, 4, 8) else "phase"
    if not vec_ok:
        return "scalar-" + ("up" if mapping.startswith("up") else mapping)
    if mapping == "plain":
        return "plain16" if d.conv_w % 4 == 0 else "whole-image16"
    return mapping


def geometry(d, variant):
    """The tile geometry the library configures for descriptor ``d`` under ``variant`` (-1: whatever the heuristic picks), or None
    when the pair is not served by the direct kernel.  R, G, CK, the tiles and the LDS bytes come from `mp_plan_entry_info`; the
    rest is derived here and cross-checked against the reported block count and LDS size (`consistent`)."""
    lib = _lib.load()
    plan = lib.mp_plan_create()
    assert plan
    try:
        fake = [0x7F0000000000 + 256 * i for i in range(1, 8)]
        if lib.mp_plan_add_conv_variant(plan, ctypes.byref(d), int(variant), *fake) != 0:
            return None
        info = (ctypes.c_int64 * 12)()
        assert lib.mp_plan_entry_info(plan, 0, info) == 0
        kind, ks, stride, picked, blocks, lds, ct, pt, ck, g, r, light = list(info)
    finally:
        lib.mp_plan_destroy(plan)
    if kind != 0 or not 0 <= picked < 8:
        return None  # another form (streaming 1x1, GEMM, small-problem): its own info layout
    cin_pad4, t = _round_up(d.cin, 4), ks * ks
    n_chunks = cin_pad4 // ck
    rin, wp = (r - 1) * stride + ks, (d.conv_w - 1) * stride + ks
    if wp < d.pad_left + d.w and d.pad_left + d.w - wp <= 2:
        wp = d.pad_left + d.w  # whole input rows are staged
    ncols = min(d.w, wp - d.pad_left)
    vec = d.w % 4 == 0 and ncols % 4 == 0  # 16-byte staging units
    tiles_y = 1 if (g > 1 or r >= d.conv_h) else -(-d.conv_h // r)
    tiles_n, n_ct = -(-d.n // g), -(-_round_up(d.cout, 16) // ct)
    nbuf = 2 if n_chunks > 1 else 1
    return dict(variant=picked, ct=ct, pt=pt, light=bool(light), CK=ck, G=g, R=r, n_chunks=n_chunks, vec_staging=vec, tiles_y=tiles_y,
                tiles_n=tiles_n, n_ct=n_ct, blocks=blocks, lds=lds, epilogue=epilogue_branch(d, r),
                consistent=(blocks == n_ct * tiles_y * tiles_n and cin_pad4 % ck == 0 and
                            lds == nbuf * (ck * _plane_pad(g * rin * wp) + ck * t * ct) * 4))
