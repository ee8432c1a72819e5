"""The (shape, tile variant) matrix of the fp16 convolution tests, generated from the library's own answer.

`mp_f16_conv_supported` (include/mindpose_hip.h) runs the entry point's checks and the kernel family's dispatch without the launch -
host-only, so the matrix can be built at collection time and on a machine without a GPU.  A pair the library does not serve is never
collected (no skip), every collected pair must return MP_OK (a HIP error or a pair that stopped being served is a FAILURE), and
tests/test_f16_matrix_cpu.py holds the floors: every forced variant serves at least one of its family's cases and the pairs the
tuner picked for the three bench plans (tests/golden/bench_plan_picks.json) are still served.

The second half of the file is the EDGE matrix: case tables in launch kinds - as mindpose_amd/models/layers.py and
train_ops.py build the descriptors -, `launch_words` (the launch record of `mp_f16_conv_launch_words` as a dict) and `classes`, which
reads from that record the classes of tile geometry a launch is in.  tests/test_f16_matrix_cpu.py holds the floor - every forced
variant meets every class of its family in a collected pair, or the (variant, class) is a row of its exemption table -,
tests/test_gpu_f16_variants.py runs every pair.
"""
import contextlib
import ctypes
import functools
import itertools
import os

import pytest

from mindpose_amd import _lib

# tile-variant families (csrc/conv_f16.h): one-tile 0-9 + 20, 21, 24; persistent multi-tile 10-19 + 22, 23; weights in registers
# 25-36 + 45-47; weight-stationary 37-44
TILE_VARIANTS = list(range(10)) + [20, 21, 24]
MT_VARIANTS = list(range(10, 20)) + [22, 23]
WREG_VARIANTS = list(range(25, 37)) + [45, 46, 47]
WREG_S2_VARIANTS = list(range(25, 37))
WS_VARIANTS = list(range(37, 45))

CONV_CASES = [
    # n, cin, cout, k, s, h, w, relu, n_res
    (2, 32, 32, 3, 1, 64, 48, True, 1),     # W32 branch 0
    (3, 64, 64, 3, 1, 32, 24, True, 1),     # branch 1 (two chunks with the 64-cout tile)
    (3, 128, 128, 3, 1, 16, 12, True, 0),
    (5, 256, 256, 3, 1, 8, 6, True, 2),     # multi-image tiles, many chunks
    (2, 3, 64, 3, 2, 64, 48, True, 0),      # stem conv1: 3 channels in one block, zero planes
    (2, 64, 64, 3, 2, 32, 24, True, 0),     # stem conv2 (stride 2)
    (2, 48, 48, 3, 1, 24, 16, True, 1),     # W48 widths: cin padded to 64, cout tile 48
    (2, 96, 192, 3, 2, 16, 12, False, 2),   # fuse-layer down-sampling conv with both residuals
    (2, 64, 256, 1, 1, 16, 12, True, 1),    # bottleneck 1x1
    (2, 256, 64, 1, 1, 16, 12, True, 0),
    (3, 32, 17, 1, 1, 64, 48, False, 0),    # head: 17 couts + bias
    (1, 40, 24, 3, 1, 9, 7, False, 0),      # ragged everything
]

WREG_CASES = [
    # n, cin, cout, k, s, h, w, relu, n_res  - stride-1 "same" convs with >= 64 input channels (conv_f16_wreg.hip)
    (3, 64, 64, 3, 1, 32, 24, True, 1),     # branch 1: row bands of 4, 8 bands per image
    (3, 128, 128, 3, 1, 16, 12, True, 1),   # branch 2: half-image bands (P6) / quarter bands (P3)
    (5, 256, 256, 3, 1, 8, 6, True, 1),     # branch 3: two images per tile, odd batch -> a half-empty last tile
    (2, 192, 192, 3, 1, 16, 12, True, 0),   # W48 branch 2: three cout tiles per wave
    (3, 96, 192, 3, 1, 12, 9, False, 1),    # ragged: 10-row bands of a 12-row map, 6 padding lanes per tile
    (2, 72, 64, 3, 1, 10, 7, True, 0),      # input channels padded 72 -> 96: three zero planes from the range check
    (2, 256, 64, 1, 1, 16, 12, True, 0),    # 1x1 (no halo column), 8 k-steps
    (2, 64, 256, 1, 1, 16, 12, True, 1),    # 1x1, four cout tiles per wave
    (130, 128, 128, 3, 1, 16, 12, True, 1), # more workgroups than CUs
    (3, 32, 32, 3, 1, 64, 48, True, 1),     # branch 0: pixel-split waves (W4), one k-step (no refill), 8-row bands
    (2, 48, 48, 3, 1, 24, 16, True, 1),     # W48 widths: three cout tiles, cin padded 48 -> 64
    (2, 96, 96, 3, 1, 24, 18, True, 0),     # W48 branch 1: W2 with three cout tiles per wave
    (3, 192, 192, 3, 1, 24, 18, True, 1),   # W48 branch 2 at config 5's map: P7C3 = 6-row bands, four per image
    (3, 384, 384, 3, 1, 12, 9, True, 1),    # W48 branch 3 at config 5's map: P4C3 = 7-row bands (7 + 5 rows), two cout slices
    (2, 256, 256, 3, 1, 10, 8, False, 1),   # P5C4: 256 couts per workgroup, 80-px bands
]

WS_CASES = [
    # n, cin, cout, k, s, h, w, relu, n_res - 3x3 stride-1 layers of the 32 ... 128-channel branches (W32 and W48 widths), ragged
    # bands (h not a multiple of the rows per tile), padded channel counts, long tile runs (MP_F16_WS_GROUPS)
    (5, 32, 32, 3, 1, 64, 48, True, 1),
    (3, 48, 48, 3, 1, 96, 72, True, 1),
    (3, 48, 48, 3, 1, 23, 72, True, 0),
    (6, 64, 64, 3, 1, 32, 24, True, 1),
    (5, 64, 64, 3, 1, 21, 17, False, 1),
    (6, 96, 96, 3, 1, 48, 36, True, 1),
    (4, 96, 96, 3, 1, 11, 36, True, 0),
    (9, 128, 128, 3, 1, 16, 12, True, 1),
    (3, 40, 48, 3, 1, 30, 33, True, 1),
    (3, 72, 96, 3, 1, 19, 20, False, 1),
    (2, 128, 64, 3, 1, 16, 12, True, 0),
    (4, 128, 128, 3, 1, 24, 16, True, 0),   # 128 couts x 96 px (variant 44): two-row bands
]

WREG_S2_CASES = [
    # n, cin, cout, h, w, n_res - 3x3 stride-2 pad-1 convs of the transition / exchange-unit layers (conv_f16_wreg.hip, S = 2)
    (3, 32, 64, 64, 48, 2),     # fuse down-sampling conv with running sum + identity
    (3, 64, 128, 32, 24, 1),
    (5, 128, 256, 16, 12, 0),   # two images per tile, odd batch
    (2, 32, 32, 64, 48, 0),
    (2, 64, 64, 30, 22, 2),     # ragged: odd output extents after the stride
    (2, 96, 192, 24, 18, 1),    # W48 widths
    (2, 256, 128, 17, 13, 0),   # odd input extents: the last tap column reads the shared zero slot (round 4's 256 -> 64 form of this
                                # case was served by NO variant of the family and had been skipping since it was written)
    (2, 48, 96, 48, 36, 1),     # W48 transition 48 -> 96: the three-cout-tile two-wave shape (variant 32)
    (2, 32, 96, 32, 24, 0),     # ... and the four-wave one (variant 35)
]

PHASES4_CASES = [(2, 32, 64, 32, 24), (3, 64, 128, 16, 12), (2, 48, 96, 24, 16), (5, 32, 32, 64, 48)]  # n, cin, cout, h, w
PHASES4_VARIANTS = [0, 4, 10, 13, 17]


def conv_desc(n, cin, cout, k, s, h, w, relu=0, flags=0):
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=s, pad_top=pad, pad_left=pad, conv_h=ho, conv_w=wo,
                         out_h=ho, out_w=wo, out_mul=1, out_rep=1, out_off_y=0, out_off_x=0, relu=int(relu), flags=flags)


def phases4_desc(n, cin, cout, h, w):
    """The merged four-phase launch of a 3x3 stride-2 data gradient: input = the [n, cout, h/2, w/2] gradient, output [n, cin, h, w]."""
    ho, wo = h // 2, w // 2
    return _lib.ConvDesc(n=n, cin=cout, h=ho, w=wo, cout=cin, kh=2, kw=2, stride=1, pad_top=0, pad_left=0, conv_h=ho, conv_w=wo,
                         out_h=h, out_w=w, out_mul=2, out_rep=1, out_off_y=0, out_off_x=0, relu=0, flags=_lib.MP_CONV_PHASES4)


@contextlib.contextmanager
def knobs(**env):
    """MP_* experiment knobs for the duration of a query (tests set the same ones with monkeypatch for the launch)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def supported(desc, variant, n_res=0, stats=0, **env) -> bool:
    with knobs(**env):
        return bool(_lib.load().mp_f16_conv_supported(ctypes.byref(desc), int(variant), int(n_res), int(stats)))


def served_pairs(cases, variants, desc_of, n_res_of=lambda c: 0, stats=0, **env):
    """[(case, variant)] the library serves, as pytest params with readable ids."""
    out = []
    for ci, case in enumerate(cases):
        d = desc_of(case)
        for v in variants:
            if supported(d, v, n_res_of(case), stats, **env):
                out.append(pytest.param(case, v, id=f"case{ci}-v{v}"))
    return out


def conv_case_desc(case):
    n, cin, cout, k, s, h, w, relu, _ = case
    return conv_desc(n, cin, cout, k, s, h, w, relu)


def conv_case_res(case):
    return case[8]


def s2_case_desc(case):
    n, cin, cout, h, w, _ = case
    return conv_desc(n, cin, cout, 3, 2, h, w, 1)


def s2_case_res(case):
    return case[5]


def phases4_case_desc(case):
    return phases4_desc(*case)


# ---- the edge matrix ------------------------------------------------------------------------------------------------

PHASES = [(0, 0), (0, 1), (1, 0), (1, 1)]
TRAIN_FLAGS = _lib.MP_CONV_SHARES_CUS  # what train_ops.py sets on every descriptor of a training step

# mp_f16_conv_launch_words: the two return codes, then - after an accepted build - these fields (csrc/conv_f16.hip, same order)
WORD_NAMES = ("rc dry_rc ks stride variant lds_bytes N C8in H W Cout Cout_pad16 C8out Ho Wo pad_t pad_l R G Rin Wp img_plane plane PK PKs "
              "n_chunks n_ct tiles_y tiles_n ncols upc in_buf w_buf nbuf relu out_h out_w out_mul off_y off_x magic_upc magic_ncols magic_rin "
              "magic_rwo magic_wo RWo total_blocks phases w_phase_bytes tiles_total tiles_per_wg n_groups ni_used nw_used magic_rows step_rows "
              "step_cols st_mode st_nparts st_relu pre_relu has_x has_wp has_scale has_shift has_res1 has_res2 has_out has_st_part has_st_z "
              "has_st_y has_pre_scale has_pre_shift has_pre_out st_part_offset").split()


def launch_words(desc, variant, n_res=0, stats=0, **env):
    """The launch record of (desc, variant, residual count, statistics mode) under the knobs `env` as {field: value}, or None when the
    entry point would refuse the launch (either return code non-zero)."""
    cap = len(WORD_NAMES) + 8
    buf = (ctypes.c_int64 * cap)()
    with knobs(**env):
        n = _lib.load().mp_f16_conv_launch_words(ctypes.byref(desc), int(variant), int(n_res), int(stats), buf, cap)
    assert n >= 2, f"mp_f16_conv_launch_words returned {n}"
    if buf[0] != 0 or buf[1] != 0:
        return None
    assert n == len(WORD_NAMES), (n, len(WORD_NAMES))
    return dict(zip(WORD_NAMES, buf[:n]))


def classes(words, family, n_res):
    """The classes of tile geometry the launch `words` (launch_words) is in; family = "tile" / "mt" / "wreg" / "wreg_s2" / "ws"
    decides which fields mean what (the table at the top of csrc/conv_f16.h).  What each class guards: DESIGN 4.4a."""
    w = words
    out = set()
    # pixel tile: R rows of one image, or - when that is the whole image - G images (f16_geom_fit)
    if w["G"] > 1:
        out.add("group:ragged" if w["N"] % w["G"] else "group:even")
    elif w["R"] >= w["Ho"]:
        out.add("image:whole")
    else:
        out.add("rows:ragged" if w["Ho"] % w["R"] else "rows:even")
    out.add(f"res:{n_res}")
    if w["PKs"] < w["PK"]:
        out.add("k:zero-planes")       # fewer staged planes than the k-steps read: the rest of LDS stays zero
    if w["Cout"] % 8:
        out.add("cout:%8")             # padding channels inside the last 8-channel block: stored as zeros
    if w["Cout"] % 16 == 8:
        out.add("cout:%16==8")         # whole 8-channel blocks, but the last 16-cout MFMA tile has no second one: co_off = kInv there
    if family in ("tile", "mt"):
        t = w["ks"] * w["ks"]
        ct = w["w_buf"] // (w["PK"] * t)
        out.add("cout:partial-tile" if w["Cout_pad16"] % ct else "cout:whole-tiles")
        out.add("cols:partial" if w["ncols"] < w["W"] else "cols:all")
        out.add("staging:several-slots" if w["ni_used"] > 1 else "staging:one-slot")
        out.add({1: "out:plain", 2: "out:phase"}[w["out_mul"]] if w["phases"] == 1 else "out:phases4")
    if family == "tile":
        nc = w["n_chunks"]
        out.add("chunks:1" if nc == 1 else "chunks:2" if nc == 2 else "chunks:odd" if nc % 2 else "chunks:even")
        if nc > 1 and nc * w["PK"] > w["C8in"]:
            out.add("chunks:c8in-tail")  # the last chunk runs past C8in: the `off = kOob` line of stage_load
        out.add("step:cols" if w["step_cols"] else "step:rows-only")
    if family == "mt":
        out.add(f"nbuf:{w['nbuf']}")
    if family in ("mt", "ws"):
        tpw, total, ty = w["tiles_per_wg"], w["tiles_total"], w["tiles_y"]
        out.add("run:ragged-last" if total % tpw else "run:even")
        if total > ty and (tpw > ty or ty % tpw):
            out.add("run:crosses-image")
        out.add("groups:several" if w["n_groups"] > 1 else "groups:one")
    if family in ("wreg", "wreg_s2"):
        out.add("dma:fast" if w["upc"] > 0 else "dma:slow")
    return out


# the classes every forced variant of a family has to meet (tests/test_f16_matrix_cpu.py; exemptions are rows of its table)
ROW_CLASSES = ["rows:ragged", "rows:even", "image:whole", "group:ragged", "group:even"]
FAMILY_CLASSES = {
    "tile": ROW_CLASSES + ["res:0", "res:1", "res:2", "k:zero-planes", "chunks:1", "chunks:2", "chunks:odd", "chunks:even", "chunks:c8in-tail",
                           "cout:%8", "cout:%16==8", "cout:partial-tile", "cols:partial", "staging:several-slots", "step:cols", "step:rows-only",
                           "out:plain", "out:phase", "out:phases4"],
    "mt": ROW_CLASSES + ["res:0", "res:1", "res:2", "k:zero-planes", "cout:%8", "cout:%16==8", "cout:partial-tile", "cols:partial",
                         "staging:several-slots", "nbuf:1", "nbuf:2", "out:plain", "out:phase", "out:phases4", "run:ragged-last", "run:even",
                         "run:crosses-image", "groups:several", "groups:one"],
    "wreg": ROW_CLASSES + ["res:0", "res:1", "k:zero-planes", "cout:%8", "cout:%16==8", "dma:fast", "dma:slow"],
    "wreg_s2": ROW_CLASSES + ["res:0", "res:1", "res:2", "k:zero-planes", "cout:%8", "cout:%16==8"],
    "ws": ["rows:ragged", "rows:even", "image:whole", "res:0", "res:1", "k:zero-planes", "cout:%8", "cout:%16==8", "run:ragged-last", "run:even", "run:crosses-image", "groups:several"],
}


def _desc(n, cin, h, w, cout, k, s, pad_t, pad_l, conv_h, conv_w, out_h, out_w, out_mul=1, off_y=0, off_x=0, relu=0, flags=0):
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=s, pad_top=pad_t, pad_left=pad_l, conv_h=conv_h,
                         conv_w=conv_w, out_h=out_h, out_w=out_w, out_mul=out_mul, out_rep=1, out_off_y=off_y, out_off_x=off_x,
                         relu=int(relu), flags=flags)


class Launch:
    """One kernel launch of a case: its descriptor, the weight packing (mp_f16_pack_weight mode + phase), whether `res1` is the case's
    own output so far (`accumulate`: the phases of deconv_dgrad, out == res1) and whether it is the merged MP_CONV_PHASES4 launch."""

    def __init__(self, desc, mode, py=0, px=0, accumulate=False, merged=False):
        self.desc, self.mode, self.py, self.px, self.accumulate, self.merged = desc, mode, py, px, accumulate, merged


# kind -> what a case tuple holds; every kind is built as layers.py / train_ops.py (`_conv_dgrad`, `_dgrad16_stride2`,
# `_deconv_forward`, `_deconv_backward`) build it
#   conv               n, cin, cout, k, s, h, w, relu, n_res, crop   "same" padding; crop > 0: only the first conv_w - crop output columns
#                                                                    (the first band of a column-banded layer: ncols < W)      packing 0
#   deconv             n, cin, cout, h, w, relu      Conv2dTranspose(4, 2, 1): four 2x2 phases, pad 1 - p, offset p          packing 1
#   dgrad_s1           n, cin, cout, k, h, w, n_res  of the FORWARD stride-1 conv: reads dz [n, cout, h, w], writes dx         packing 2
#   dgrad_k3s2         n, cin, cout, h, w            of the forward 3x3 stride-2 pad-1 conv (h, w of ITS input, odd allowed):
#                                                    four 2x2 pad-0 phases, out_mul 2, offset p                                 packing 3
#   dgrad_k3s2_merged  n, cin, cout, h, w            the same as ONE MP_CONV_PHASES4 launch (even h, w only: validate)         packing 3
#   dgrad_k1s2         n, cin, cout, h, w            of the forward 1x1 stride-2 conv: out_mul 2 into a zeroed gradient        packing 2
#   deconv_dgrad       n, cin, cout, h, w            of the transposed conv: four 2x2 phases, pad p, summed through res1 = out packing 4
@functools.lru_cache(maxsize=None)
def launches(kind, case):
    if kind == "conv":
        n, cin, cout, k, s, h, w, relu, _, crop = case
        p = k // 2
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1 - crop
        return [Launch(_desc(n, cin, h, w, cout, k, s, p, p, ho, wo, ho, wo, relu=relu), 0)]
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
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return [Launch(_desc(n, cout, ho, wo, cin, 2, 1, 0, 0, (h - py + 1) // 2, (w - px + 1) // 2, h, w, out_mul=2, off_y=py, off_x=px,
                             flags=TRAIN_FLAGS), 3, py, px) for py, px in PHASES]
    if kind == "dgrad_k3s2_merged":
        n, cin, cout, h, w = case
        assert h % 2 == 0 and w % 2 == 0
        return [Launch(_desc(n, cout, h // 2, w // 2, cin, 2, 1, 0, 0, h // 2, w // 2, h, w, out_mul=2,
                             flags=TRAIN_FLAGS | _lib.MP_CONV_PHASES4), 3, merged=True)]
    if kind == "dgrad_k1s2":
        n, cin, cout, h, w = case
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return [Launch(_desc(n, cout, ho, wo, cin, 1, 1, 0, 0, ho, wo, h, w, out_mul=2, flags=TRAIN_FLAGS), 2)]
    if kind == "deconv_dgrad":
        n, cin, cout, h, w = case
        return [Launch(_desc(n, cout, h, w, cin, 2, 1, py, px, h, w, h, w, flags=TRAIN_FLAGS), 4, py, px, accumulate=(py, px) != (0, 0))
                for py, px in PHASES]
    raise ValueError(kind)


def n_res(kind, case):
    """Residual tensors of the case's epilogue that are operands (the running sum of deconv_dgrad is not one)."""
    return {"conv": lambda: case[8], "dgrad_s1": lambda: case[6]}.get(kind, lambda: 0)()


def launch_res(kind, case, la):
    """Residual pointers the launch is given: the case's operands, or the running sum."""
    return 1 if la.accumulate else n_res(kind, case)


def pair_words(kind, case, variant, **env):
    """[launch words] of every launch of the case under the forced variant, or None when the library refuses one of them."""
    out = []
    for la in launches(kind, case):
        w = launch_words(la.desc, variant, launch_res(kind, case, la), 0, **env)
        if w is None:
            return None
        out.append(w)
    return out


def pair_classes(kind, case, variant, family, **env):
    """The classes the pair's launches are in (their union: every launch is checked on its own on the GPU), or None: not served."""
    ws = pair_words(kind, case, variant, **env)
    if ws is None:
        return None
    out = set()
    for la, w in zip(launches(kind, case), ws):
        out |= classes(w, family, launch_res(kind, case, la))
    return out


# The search grid behind the exemption table of tests/test_f16_matrix_cpu.py: a (variant, class) may be exempt only when NO case of
# its family's grid reaches the class on the variant.  Small maps of every raggedness against the 64 ... 384-pixel tiles, batch sizes
# that leave short image groups, channel counts on both sides of every 8 / 16 / 32 boundary up to the widest layers (264 = 8 chunks
# of 32 + 8), 0 ... 2 residuals; the edge tables below were drawn from the same grid.
GRID_MAPS = [(4, 4), (8, 6), (9, 7), (13, 24), (21, 13), (16, 12), (32, 24), (5, 40), (13, 8), (7, 48)]
GRID_N = (2, 3, 5, 6)


def search_grid(family):
    """(kind, case) of the family's grid, in a fixed order"""
    if family in ("tile", "mt"):
        cins, couts = (8, 24, 40, 64, 72, 128, 136, 256, 264), (17, 24, 40, 64, 72)
        for n, cin, cout, (k, s), (h, w), res, crop in itertools.product(GRID_N, cins, couts, ((1, 1), (3, 1), (3, 2), (1, 2)), GRID_MAPS,
                                                                         (0, 1, 2), (0, 4)):
            if crop == 0 or w // s > 6:
                yield "conv", (n, cin, cout, k, s, h, w, bool(res % 2), res, crop)
        for n, cin, cout, (h, w) in itertools.product(GRID_N, (8, 40, 72, 264), (17, 24, 64), GRID_MAPS):
            yield "deconv", (n, cin, cout, h, w, True)
            yield "dgrad_k3s2", (n, cin, cout, h, w)
            if h % 2 == 0 and w % 2 == 0:
                yield "dgrad_k3s2_merged", (n, cin, cout, h, w)
            yield "dgrad_k1s2", (n, cin, cout, h, w)
            yield "deconv_dgrad", (n, cin, cout, h, w)
            for k, res in ((1, 0), (3, 0), (3, 1)):
                yield "dgrad_s1", (n, cin, cout, k, h, w, res)
    elif family in ("wreg", "wreg_s2"):
        s = 2 if family == "wreg_s2" else 1
        maps = GRID_MAPS + [(24, 18), (12, 9), (10, 8), (30, 22), (17, 13), (64, 48), (42, 36), (46, 36)]
        for n, cin, cout, k, (h, w), res in itertools.product(GRID_N, (24, 32, 40, 48, 64, 72, 128, 264), (32, 60, 64, 88, 96, 120, 124, 128, 184, 188, 192, 248, 252, 256), (1, 3), maps,
                                                              (0, 1, 2)):
            if k == 3 or s == 1:
                yield "conv", (n, cin, cout, k, s, h, w, bool(res % 2), res, 0)
            if s == 1 and res < 2:
                yield "dgrad_s1", (n, cout, cin, k, h, w, res)
    elif family == "ws":
        maps = GRID_MAPS + [(24, 18), (23, 72), (11, 36), (30, 33), (19, 20), (21, 17), (32, 20), (26, 24), (16, 12), (12, 9), (8, 12), (20, 16), (16, 18)]
        for n, cin, cout, (h, w), res in itertools.product(GRID_N + (9,), (24, 32, 40, 48, 64, 72, 96, 104, 120, 128), (24, 28, 32, 40, 44, 48, 56, 60, 64, 88, 92, 96, 120, 124, 128), maps, (0, 1)):
            yield "conv", (n, cin, cout, 3, 1, h, w, bool(res), res, 0)
            yield "dgrad_s1", (n, cout, cin, 3, h, w, res)
    else:
        raise ValueError(family)


FAMILY_VARIANTS = {"tile": TILE_VARIANTS, "mt": MT_VARIANTS, "wreg": WREG_VARIANTS, "wreg_s2": WREG_S2_VARIANTS, "ws": WS_VARIANTS}
# the knob sets a family's pairs are collected under (as the existing tests set them; the slow-DMA knob forces the weights-in-registers
# kernel's other staging form on shapes that would take the fast one)
FAMILY_KNOBS = {"tile": [{}], "mt": [dict(MP_F16_MT_GROUPS=1), dict(MP_F16_MT_GROUPS=3)], "wreg": [{}, dict(MP_F16_WREG_SLOW_DMA=1)],
                "wreg_s2": [{}], "ws": [dict(MP_F16_WS_GROUPS=2), dict(MP_F16_WS_GROUPS=5)]}
LDS_KINDS = ["conv", "deconv", "dgrad_s1", "dgrad_k3s2", "dgrad_k3s2_merged", "dgrad_k1s2", "deconv_dgrad"]
FAMILY_KINDS = {"tile": LDS_KINDS, "mt": LDS_KINDS, "wreg": ["conv", "dgrad_s1"], "wreg_s2": ["conv"], "ws": ["conv", "dgrad_s1"]}

# The edge tables: the first cases of each are chosen by hand (the odd extents of every stride-2 kind, one case per launch kind), the
# rest by a greedy cover of the (variant, class) holes over `search_grid` - see the floor in tests/test_f16_matrix_cpu.py for what
# they reach.  One table for the two LDS-operand families (one-tile, multi-tile), as CONV_CASES above.
EDGE_LDS_CASES = [
    ("conv", (3, 264, 24, 1, 1, 8, 6, False, 2, 0)),      # 48-px map: image groups (short last group on the 96-px tiles), 3 / 9 chunks + C8in tail
    ("conv", (5, 8, 64, 1, 1, 9, 7, True, 2, 0)),         # 63-px map, N = 5: a short last group on every tile size; one zero-padded chunk
    ("conv", (3, 8, 72, 1, 1, 5, 40, False, 0, 0)),       # 5 x 40: ragged row bands of 4 / 2 rows; 72 couts = a partial 64- / 48-cout tile
    ("conv", (3, 40, 24, 3, 2, 21, 13, True, 1, 0)),      # 3x3 stride 2 on odd extents (11 x 7 out)
    ("conv", (2, 24, 40, 1, 2, 9, 7, False, 0, 0)),       # 1x1 stride 2 on odd extents (5 x 4 out)
    ("deconv", (3, 40, 24, 9, 7, True)),
    ("dgrad_k3s2", (3, 24, 40, 21, 13)),                  # odd extents: the four phases have 11 / 10 rows and 7 / 6 columns
    ("dgrad_k3s2_merged", (3, 24, 40, 16, 12)),
    ("dgrad_k1s2", (3, 24, 40, 21, 13)),
    ("deconv_dgrad", (3, 24, 40, 9, 7)),
    ("dgrad_s1", (2, 24, 40, 3, 13, 24, 1)),
    ("conv", (5, 256, 17, 1, 1, 16, 12, False, 0, 4)),    # cropped output (8 of 12 columns: ncols < W), 17 couts, 2 / 4 / 8 chunks
    ("dgrad_k3s2_merged", (3, 8, 17, 32, 24)),
    ("deconv", (2, 8, 17, 32, 24, True)),
    ("dgrad_k3s2", (6, 8, 17, 5, 40)),
    ("deconv_dgrad", (2, 8, 17, 13, 8)),
    ("dgrad_s1", (2, 8, 64, 1, 13, 24, 0)),
    # three wide maps with large K: the one-input-buffer fallback (nbuf == 1) of the one-workgroup-per-CU multi-tile builds - 15 / 17 /
    # 19, 16 / 18 and 23 in turn -, and 4 / 8 chunks (an even count >= 4) on the one-tile builds
    ("conv", (2, 128, 17, 3, 1, 7, 48, False, 0, 0)),
    ("conv", (3, 40, 17, 1, 2, 7, 48, False, 0, 4)),      # 1x1 stride 2, cropped: two chunks with a C8in tail, rows-only staging steps
    ("conv", (2, 72, 17, 3, 1, 5, 40, False, 0, 0)),
    ("conv", (2, 256, 17, 3, 1, 13, 24, False, 0, 0)),
]
EDGE_WREG_CASES = [
    ("conv", (2, 72, 192, 3, 1, 13, 24, False, 0, 0)),
    ("dgrad_s1", (2, 256, 72, 3, 16, 12, 1)),
    ("dgrad_s1", (6, 192, 64, 3, 8, 6, 1)),
    ("conv", (6, 64, 256, 3, 1, 10, 8, False, 0, 0)),
    ("conv", (2, 64, 192, 3, 1, 32, 24, False, 0, 0)),
    ("conv", (3, 64, 192, 3, 1, 8, 6, False, 0, 0)),
    ("conv", (5, 64, 256, 3, 1, 4, 4, False, 0, 0)),
    ("conv", (5, 64, 192, 3, 1, 10, 8, False, 0, 0)),
    ("conv", (2, 64, 256, 3, 1, 24, 18, False, 0, 0)),
    ("conv", (3, 64, 256, 1, 1, 8, 6, False, 0, 0)),
    ("conv", (6, 64, 256, 3, 1, 4, 4, False, 0, 0)),
    ("conv", (3, 64, 192, 3, 1, 4, 4, False, 0, 0)),
    ("conv", (5, 64, 192, 3, 1, 4, 4, False, 0, 0)),
    ("conv", (2, 24, 96, 1, 1, 16, 12, False, 0, 0)),
    ("conv", (2, 24, 96, 1, 1, 24, 18, False, 0, 0)),
    # couts off the 16 boundary (the 16-byte paired stores of the epilogue against a last block with padding channels / without a
    # partner block): 184 = 192 - 8 and 188 on the builds whose workgroup takes 32 / 64 / 96 / 192 couts, 248 and 252 on the 128 / 256 ones
    ("conv", (2, 64, 184, 3, 1, 13, 24, False, 0, 0)),
    ("conv", (2, 64, 188, 3, 1, 13, 24, False, 0, 0)),
    ("conv", (2, 64, 248, 3, 1, 13, 24, False, 0, 0)),
    ("conv", (2, 64, 252, 3, 1, 13, 24, False, 0, 0)),
]
EDGE_WREG_S2_CASES = [
    ("conv", (2, 128, 128, 3, 2, 17, 13, True, 1, 0)),    # odd input extents
    ("conv", (2, 72, 192, 3, 2, 13, 24, False, 0, 0)),
    ("conv", (2, 72, 256, 3, 2, 30, 22, False, 2, 0)),
    ("conv", (2, 24, 192, 3, 2, 64, 48, True, 1, 0)),     # 32 x 24 out: row bands on the 192- and 384-pixel tiles of the pixel-split builds
    ("conv", (5, 64, 192, 3, 2, 16, 12, True, 1, 0)),
    ("conv", (2, 24, 192, 3, 2, 42, 36, False, 2, 0)),
    ("conv", (2, 64, 256, 3, 2, 16, 12, False, 0, 0)),
    ("conv", (2, 64, 192, 3, 2, 32, 24, False, 2, 0)),
    ("conv", (2, 64, 256, 3, 2, 32, 24, True, 1, 0)),
    ("conv", (2, 24, 96, 3, 2, 32, 24, False, 0, 0)),
    ("conv", (5, 64, 256, 3, 2, 9, 7, False, 0, 0)),
    ("conv", (2, 24, 96, 3, 2, 46, 36, False, 0, 0)),     # 23 x 18 out: the ragged band of the 384-pixel four-wave builds (21 + 2 rows)
    ("conv", (3, 24, 96, 3, 2, 32, 24, False, 0, 0)),
    ("conv", (6, 64, 192, 3, 2, 8, 6, False, 0, 0)),
    ("conv", (2, 64, 256, 3, 2, 9, 7, False, 0, 0)),
    ("conv", (2, 64, 120, 3, 2, 13, 24, False, 0, 0)),
    ("conv", (2, 64, 192, 3, 2, 9, 7, False, 0, 0)),
    ("conv", (2, 64, 192, 3, 2, 24, 18, False, 0, 0)),
    # couts off the 16 boundary (120 above is the other one), the 24-channel ones for the four-wave builds 34 / 35
    ("conv", (2, 64, 188, 3, 2, 13, 24, False, 0, 0)),
    ("conv", (2, 24, 88, 3, 2, 32, 24, False, 0, 0)),
    ("conv", (2, 64, 252, 3, 2, 13, 24, False, 0, 0)),
    ("conv", (2, 24, 188, 3, 2, 32, 24, False, 0, 0)),
    ("conv", (2, 64, 184, 3, 2, 13, 24, False, 0, 0)),
    ("conv", (2, 64, 248, 3, 2, 9, 7, False, 0, 0)),
]
EDGE_WS_CASES = [
    ("conv", (2, 40, 64, 3, 1, 23, 72, False, 0, 0)),
    ("conv", (6, 72, 96, 3, 1, 32, 24, False, 0, 0)),
    ("conv", (2, 104, 128, 3, 1, 23, 72, False, 0, 0)),
    ("dgrad_s1", (5, 96, 40, 3, 32, 24, 1)),
    ("conv", (2, 24, 32, 3, 1, 23, 72, False, 0, 0)),
    ("dgrad_s1", (2, 96, 72, 3, 32, 20, 1)),
    ("dgrad_s1", (2, 128, 104, 3, 13, 24, 0)),
    ("dgrad_s1", (2, 32, 24, 3, 32, 24, 1)),
    ("conv", (2, 40, 48, 3, 1, 32, 20, False, 0, 0)),
    ("dgrad_s1", (2, 64, 40, 3, 32, 24, 1)),
    ("conv", (2, 104, 64, 3, 1, 13, 24, True, 1, 0)),
    # couts off the 16 boundary, per build by its cin range and cout slice (24 / 28 for 37, 40 / 44 for 38, 56 / 60 for 39 / 40, 88 / 92
    # for 41 / 42, 120 / 124 for 43 / 44), and maps one tile holds whole (16 x 12 = 192 px, 8 x 12 = 96 px, 13 x 24 = 312 px)
    ("conv", (3, 40, 56, 3, 1, 16, 12, False, 0, 0)),
    ("conv", (3, 104, 120, 3, 1, 8, 12, False, 0, 0)),
    ("conv", (3, 40, 92, 3, 1, 13, 24, False, 0, 0)),
    ("conv", (3, 72, 88, 3, 1, 13, 24, False, 0, 0)),
    ("conv", (3, 24, 24, 3, 1, 16, 12, False, 0, 0)),
    ("conv", (3, 72, 44, 3, 1, 16, 12, False, 0, 0)),
    ("conv", (2, 104, 124, 3, 1, 13, 24, False, 0, 0)),
    ("conv", (2, 24, 28, 3, 1, 13, 24, False, 0, 0)),
    ("conv", (2, 40, 40, 3, 1, 32, 24, False, 0, 0)),
    ("conv", (2, 40, 60, 3, 1, 13, 24, False, 0, 0)),
    ("conv", (2, 72, 28, 3, 1, 32, 24, False, 0, 0)),
]
# n, cin, cout, k, s, h, w - the cases tests/test_gpu_f16_variants.py runs the two statistics tests of tests/test_gpu_bn_fuse.py on (that
# file and its CASES stay as they are): the statistics builds (STATS = 1 / 2 are separate
# instantiations) on the geometry their `valid` mask guards.  With statistics mode 1 the launch words still show, on some forced variant
# of each LDS family: a short last image group (5 images of 63 / 104 px, 3 of 48 px), a ragged last row band (11 x 40), a multi-chunk C8in
# tail (264 channels) - the floor is test_statistics_cases_keep_their_classes in tests/test_f16_matrix_cpu.py
STATS_EDGE_CASES = [(5, 8, 64, 1, 1, 9, 7), (3, 8, 72, 1, 1, 11, 40), (3, 264, 24, 1, 1, 8, 6), (5, 8, 40, 3, 1, 13, 8),
                    (29, 8, 64, 1, 1, 8, 6)]  # 29 images: the multi-tile kernels need >= 2 tiles per workgroup under that test's 7 groups
FAMILY_CASES = {"tile": EDGE_LDS_CASES, "mt": EDGE_LDS_CASES, "wreg": EDGE_WREG_CASES, "wreg_s2": EDGE_WREG_S2_CASES, "ws": EDGE_WS_CASES}


def _knob_id(env):
    return "".join(f"{k.rsplit('_', 1)[-1].lower()}{v}-" for k, v in env.items())


@functools.lru_cache(maxsize=None)
def edge_pairs(family):
    """[(kind, case, variant, env as a sorted tuple of items, classes)] of a family: every (case, forced variant, knob set) of its
    table whose launches the library all serves"""
    out = []
    for kind, case in FAMILY_CASES[family]:
        for env in FAMILY_KNOBS[family]:
            for v in FAMILY_VARIANTS[family]:
                cl = pair_classes(kind, case, v, family, **env)
                if cl is not None:
                    out.append((kind, case, v, tuple(sorted(env.items())), frozenset(cl)))
    return out


def edge_params():
    """pytest params (family, kind, case, variant, env) of the whole edge matrix, with readable ids"""
    out = []
    for family in FAMILY_CASES:
        index = {kc: i for i, kc in enumerate(FAMILY_CASES[family])}
        for kind, case, v, env, _ in edge_pairs(family):
            out.append(pytest.param(family, kind, case, v, env, id=f"{family}-{_knob_id(dict(env))}{kind}{index[(kind, case)]}-v{v}"))
    return out
