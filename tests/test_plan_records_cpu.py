"""Pins what a launch plan shows of itself, host-only: the return code of every `mp_plan_add_*` call, `mp_plan_size` after it and the
twelve `mp_plan_entry_info` values of every recorded entry, for a fixed list of calls that walks every add function, every kernel
family an entry can hold and every bad input the add functions check (tests/golden/plan_entry_info.json).

The add functions only configure and store their pointer arguments (the first device call of a kernel family sits in its launch
function), so the pointers here are fake, distinct, 256-byte-aligned addresses and the plan is never run - no GPU needed.  A change
of the plan's host code that claims to leave behaviour alone must leave the fixture untouched.

    python tests/test_plan_records_cpu.py --record      rewrites the fixture from the built library (only when a change MEANS to
                                                        move a launch geometry or an info value), and the call list's text form
                                                        (tests/golden/plan_calls.txt, replayed by tools/plan_records_host_check.sh
                                                        under the host sanitizers)
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models import tuner  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "plan_entry_info.json")
CALLS_TEXT = os.path.join(HERE, "golden", "plan_calls.txt")  # the call list as text, for tools/plan_records_host_check.cpp

V_COUNT = tuner.F32_VARIANTS - 1  # direct tile variants 0 .. V_COUNT - 1; V_COUNT itself = the streaming 1x1 kernel
POINTWISE, GEMM, SMALL, SMALL_WIDE = V_COUNT, tuner.F32_GEMM, tuner.F32_SMALL, tuner.F32_SMALL_WIDE
NULL_PLAN = "null-plan"  # in place of a call's arguments: the same call on a null plan


def desc(n, cin, cout, k, s, h, w, relu=1, flags=0):
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=s, pad_top=pad, pad_left=pad, conv_h=ho, conv_w=wo,
                         out_h=ho, out_w=wo, out_mul=1, out_rep=1, out_off_y=0, out_off_x=0, relu=relu, flags=flags)


def deconv_desc(n, cin, cout, h, w):
    """Phase (0, 0) of Conv2dTranspose(k=4, s=2, p=1): a 2x2 conv on every second pixel of the 2h x 2w output."""
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=2, kw=2, stride=1, pad_top=1, pad_left=1, conv_h=h, conv_w=w,
                         out_h=2 * h, out_w=2 * w, out_mul=2, out_rep=1, out_off_y=0, out_off_x=0, relu=1, flags=0)


def calls():
    """[(label, function name, arguments after the plan)] - a fixed list: the fake addresses count up from one base."""
    nxt = [0x7F0000000000]

    def A(k=None):  # one fresh address, or a list of k
        got = []
        for _ in range(k or 1):
            nxt[0] += 256
            got.append(nxt[0])
        return got[0] if k is None else got

    out = []

    def add(label, fn, *args):
        out.append((label, fn, list(args)))

    def bad(fn, good, null_at, zero=None):
        """The bad inputs every add function checks: a null plan, a null required pointer, a zero dimension."""
        out.append((f"{fn} null plan", fn, [NULL_PLAN] + list(good)))
        for i in null_at:
            out.append((f"{fn} null argument {i}", fn, [None if j == i else a for j, a in enumerate(good)]))
        if zero is not None:
            i, v = zero
            out.append((f"{fn} zero dimension", fn, [v if j == i else a for j, a in enumerate(good)]))

    def conv(label, d, res=0, fn="mp_plan_add_conv", variant=None):
        ptrs = A(4) + [A() if res >= 1 else None, A() if res >= 2 else None, A()]
        add(label, fn, ctypes.byref(d), *(([variant] if variant is not None else []) + ptrs))

    # ---- fp32 direct conv, the library's choice: every arm of the cout order, k = 1 / 2 / 3 / 7, both strides
    conv("conv k1 64->256 16x12", desc(2, 64, 256, 1, 1, 16, 12), res=1)
    conv("conv k1 s2 64->128 16x12", desc(2, 64, 128, 1, 2, 16, 12))
    conv("conv k2 32->48 16x12", desc(2, 32, 48, 2, 1, 16, 12))
    conv("conv k3 32->17 64x48", desc(3, 32, 17, 3, 1, 64, 48, relu=0))
    conv("conv k3 40->40 9x7 ragged", desc(1, 40, 40, 3, 1, 9, 7), res=2)
    conv("conv k3 s2 64->80 32x24", desc(2, 64, 80, 3, 2, 32, 24))
    conv("conv k3 s2 96->192 16x12", desc(2, 96, 192, 3, 2, 16, 12), res=2)
    conv("conv k7 s2 3->64 64x48", desc(2, 3, 64, 7, 2, 64, 48))
    conv("conv k3 32->32 64x48 row tiles", desc(2, 32, 32, 3, 1, 64, 48), res=1)
    add("set lane 1", "mp_plan_set_lane", 1)
    conv("conv k3 256->256 8x6 image groups", desc(8, 256, 256, 3, 1, 8, 6), res=1)
    conv("conv k3 48->96 24x18", desc(2, 48, 96, 3, 1, 24, 18))
    add("barrier", "mp_plan_add_barrier")
    good = [ctypes.byref(desc(2, 32, 32, 3, 1, 64, 48))] + A(4) + [None, None, A()]
    bad("mp_plan_add_conv", good, [0, 1, 2, 3, 4, 7], zero=(0, ctypes.byref(desc(0, 32, 32, 3, 1, 64, 48))))
    add("conv k5 unsupported", "mp_plan_add_conv", ctypes.byref(desc(2, 32, 32, 5, 1, 64, 48)), *(A(4) + [None, None, A()]))
    add("conv k7 s1 unsupported", "mp_plan_add_conv", ctypes.byref(desc(2, 3, 64, 7, 1, 64, 48)), *(A(4) + [None, None, A()]))

    # ---- fp32 conv, forced variants
    for v in range(V_COUNT + 6):
        conv(f"variant {v} k3 32->32 64x48", desc(2, 32, 32, 3, 1, 64, 48), res=1, fn="mp_plan_add_conv_variant", variant=v)
    for v in range(V_COUNT):
        conv(f"variant {v} k7 3->64 64x48", desc(2, 3, 64, 7, 2, 64, 48), fn="mp_plan_add_conv_variant", variant=v)
    add("set lane 2", "mp_plan_set_lane", 2)
    conv("variant -1 k1 64->256", desc(2, 64, 256, 1, 1, 16, 12), fn="mp_plan_add_conv_variant", variant=-1)
    for label, d in (("64->256", desc(2, 64, 256, 1, 1, 16, 12)), ("64->64", desc(4, 64, 64, 1, 1, 16, 12)),
                     ("256->64", desc(2, 256, 64, 1, 1, 16, 12)), ("128->128", desc(130, 128, 128, 1, 1, 16, 12)),
                     ("32->32 unsupported", desc(2, 32, 32, 1, 1, 16, 12)), ("64->256 9x7 unsupported", desc(2, 64, 256, 1, 1, 9, 7))):
        conv(f"pointwise {label}", d, res=1, fn="mp_plan_add_conv_variant", variant=POINTWISE)
    conv("pointwise two residuals", desc(2, 64, 256, 1, 1, 16, 12), res=2, fn="mp_plan_add_conv_variant", variant=POINTWISE)
    for label, d in (("k1 64->256 16x12", desc(2, 64, 256, 1, 1, 16, 12)), ("k1 64->256 16x12 N=128", desc(128, 64, 256, 1, 1, 16, 12)),
                     ("k1 s2 64->128 16x12", desc(2, 64, 128, 1, 2, 16, 12)), ("k3 s2 64->64 32x24", desc(8, 64, 64, 3, 2, 32, 24)),
                     ("k1 64->64 unsupported", desc(2, 64, 64, 1, 1, 16, 12)), ("k3 s1 unsupported", desc(2, 64, 128, 3, 1, 16, 12))):
        conv(f"gemm {label}", d, res=2, fn="mp_plan_add_conv_variant", variant=GEMM)
    for v in (SMALL, SMALL_WIDE):
        for label, d in (("k3 256->256 8x6", desc(2, 256, 256, 3, 1, 8, 6)), ("k3 s2 64->128 16x12", desc(1, 64, 128, 3, 2, 16, 12)),
                         ("k1 256->17 8x6", desc(1, 256, 17, 1, 1, 8, 6)), ("k3 32->32 4x4", desc(1, 32, 32, 3, 1, 4, 4)),
                         ("k2 unsupported", desc(1, 32, 32, 2, 1, 8, 6)), ("k3 32->32 64x48 N=64", desc(64, 32, 32, 3, 1, 64, 48))):
            conv(f"small {v} {label}", d, res=2, fn="mp_plan_add_conv_variant", variant=v)
    good = [ctypes.byref(desc(2, 32, 32, 3, 1, 64, 48)), 1] + A(4) + [None, None, A()]
    bad("mp_plan_add_conv_variant", good, [0, 2, 8], zero=(0, ctypes.byref(desc(2, 32, 0, 3, 1, 64, 48))))

    # ---- transposed conv head as one GEMM launch
    for n in (2, 64):
        add(f"deconv 256->256 16x12 N={n}", "mp_plan_add_deconv4x4s2_gemm", ctypes.byref(deconv_desc(n, 256, 256, 16, 12)), *A(5))
    add("deconv not the phase-0 launch", "mp_plan_add_deconv4x4s2_gemm", ctypes.byref(desc(2, 256, 256, 2, 1, 16, 12)), *A(5))
    add("deconv 256->64 unsupported", "mp_plan_add_deconv4x4s2_gemm", ctypes.byref(deconv_desc(2, 256, 64, 16, 12)), *A(5))
    good = [ctypes.byref(deconv_desc(2, 256, 256, 16, 12))] + A(5)
    bad("mp_plan_add_deconv4x4s2_gemm", good, [0, 1, 2, 5], zero=(0, ctypes.byref(deconv_desc(2, 0, 256, 16, 12))))

    # ---- fp16 conv: library choice, tile, light tile, 16-cout and 384-pixel tiles, multi-tile, weights in registers, weight-stationary
    add("set lane 3", "mp_plan_set_lane", 3)
    for v in (-1, 1, 3, 6, 11, 16, 20, 24, 25, 31, 37, 40, 45, 48):
        conv(f"f16 variant {v} 64->64 32x24", desc(6, 64, 64, 3, 1, 32, 24), res=1, fn="mp_plan_add_conv_f16", variant=v)
    for v in (-1, 2, 7, 26, 32):
        conv(f"f16 variant {v} s2 48->96 48x36", desc(2, 48, 96, 3, 2, 48, 36), res=2, fn="mp_plan_add_conv_f16", variant=v)
    for v in (-1, 0, 5, 27):
        conv(f"f16 variant {v} k1 256->64 16x12", desc(2, 256, 64, 1, 1, 16, 12), fn="mp_plan_add_conv_f16", variant=v)
    conv("f16 variant -1 k1 32->17 64x48", desc(3, 32, 17, 1, 1, 64, 48, relu=0), fn="mp_plan_add_conv_f16", variant=-1)
    for v in range(49):  # every id on a launch with tile runs long enough for the persistent kernels (they refuse one tile per workgroup)
        conv(f"f16 variant {v} 64->64 32x24 N=1024", desc(1024, 64, 64, 3, 1, 32, 24), res=1, fn="mp_plan_add_conv_f16", variant=v)
    good = [ctypes.byref(desc(6, 64, 64, 3, 1, 32, 24)), 1] + A(4) + [None, None, A()]
    bad("mp_plan_add_conv_f16", good, [0, 2, 3, 8], zero=(0, ctypes.byref(desc(6, 64, 64, 3, 1, 0, 24))))
    add("set lane 0", "mp_plan_set_lane", 0)
    add("barrier", "mp_plan_add_barrier")

    # ---- fp32 Winograd: cout tiles 64 / 32 / 32 on the image-grouped 8x6 layer (two teams need workgroups and the CUs to themselves)
    for label, d in (("256->256 8x6 N=128", desc(128, 256, 256, 3, 1, 8, 6)), ("256->256 8x6 N=64", desc(64, 256, 256, 3, 1, 8, 6)),
                     ("256->256 8x6 N=128 shares CUs", desc(128, 256, 256, 3, 1, 8, 6, flags=_lib.MP_CONV_SHARES_CUS)),
                     ("32->32 64x48 N=2", desc(2, 32, 32, 3, 1, 64, 48)), ("64->64 32x24 N=128", desc(128, 64, 64, 3, 1, 32, 24)),
                     ("128->128 16x12 N=32", desc(32, 128, 128, 3, 1, 16, 12)), ("s2 unsupported", desc(2, 32, 32, 3, 2, 64, 48)),
                     ("9x7 unsupported", desc(2, 32, 32, 3, 1, 9, 7))):
        conv(f"winograd {label}", d, res=2, fn="mp_plan_add_conv_winograd")
    good = [ctypes.byref(desc(2, 32, 32, 3, 1, 64, 48))] + A(4) + [None, None, A()]
    bad("mp_plan_add_conv_winograd", good, [0, 1, 2, 3, 4, 7], zero=(0, ctypes.byref(desc(2, 32, 32, 3, 1, 64, 0))))
    # the shape is configured BEFORE the operands are looked at: an unsupported shape with a null operand is "unsupported"
    add("winograd unsupported shape and null x", "mp_plan_add_conv_winograd", ctypes.byref(desc(2, 32, 32, 1, 1, 64, 48)), None, *(A(3) + [None, None, A()]))

    # ---- fused fp16 BasicBlock: 32 channels on a large map (second structure; a forced 6-row band: first structure, <6,5> build) and
    # a small map (first structure, <5,3> build), 64 and 128 channels
    for label, (n, c, h, w, rows) in (("c32 64x48", (2, 32, 64, 48, 0)), ("c32 64x48 6 rows", (2, 32, 64, 48, 6)), ("c32 64x48 8 rows", (2, 32, 64, 48, 8)),
                                      ("c32 64x48 2 rows", (2, 32, 64, 48, 2)), ("c32 8x6", (2, 32, 8, 6, 0)), ("c32 16x12 N=700", (700, 32, 16, 12, 0)),
                                      ("c28 64x48", (1, 28, 64, 48, 0)), ("c64 32x24", (2, 64, 32, 24, 0)), ("c64 32x24 2 rows", (2, 64, 32, 24, 2)),
                                      ("c128 16x12", (2, 128, 16, 12, 0)), ("c48 unsupported", (2, 48, 24, 18, 0)),
                                      ("c32 7 rows unsupported", (2, 32, 64, 48, 7)), ("c32 negative rows", (2, 32, 64, 48, -1))):
        add(f"block {label}", "mp_plan_add_basicblock_f16", *(A(8) + [n, c, h, w, rows]))
    inplace = A(7)
    add("block in place unsupported", "mp_plan_add_basicblock_f16", *(inplace + [inplace[0], 2, 32, 64, 48, 0]))
    good = A(8) + [2, 32, 64, 48, 0]
    bad("mp_plan_add_basicblock_f16", good, list(range(8)), zero=(8, 0))

    # ---- the 1x1 chains of stage 1
    def chain16(n=2, cm=64, ce=256, cr=64, h=16, w=12):
        return A(5) + [1] + A(3) + [1] + A(2) + [n, cm, ce, cr, h, w]

    add("set lane 1", "mp_plan_set_lane", 1)
    add("chain f16", "mp_plan_add_expand_reduce_f16", *chain16())
    add("chain f16 64x48 N=128", "mp_plan_add_expand_reduce_f16", *chain16(n=128, h=64, w=48))
    add("chain f16 width unsupported", "mp_plan_add_expand_reduce_f16", *chain16(ce=128))
    add("chain f16 9x7 unsupported", "mp_plan_add_expand_reduce_f16", *chain16(h=9, w=7))
    bad("mp_plan_add_expand_reduce_f16", chain16(), [0, 1, 2, 6, 10, 11], zero=(12, 0))

    def chain16_ds(n=2, cm=64, ce=256, cr=64, h=16, w=12):
        return A(8) + [0] + A(3) + [1] + A(2) + [n, cm, ce, cr, h, w]

    add("chain f16 down-sample", "mp_plan_add_ds_expand_reduce_f16", *chain16_ds())
    add("chain f16 down-sample width unsupported", "mp_plan_add_ds_expand_reduce_f16", *chain16_ds(cm=32))
    bad("mp_plan_add_ds_expand_reduce_f16", chain16_ds(), [0, 1, 2, 5, 13, 14], zero=(19, 0))
    # x0 is looked at first: with it null even an unsupported width answers "null"
    add("chain f16 down-sample null x0 and unsupported width", "mp_plan_add_ds_expand_reduce_f16", *[None if i == 1 else a for i, a in enumerate(chain16_ds(cm=32))])

    def chain16_dual(n=2, cm=64, ce=256, cr=64, h=16, w=12):
        return A(4) + [0] + A(3) + [1] + A(2) + [n, cm, ce, cr, h, w]

    add("chain f16 dual", "mp_plan_add_dual_pw_f16", *chain16_dual())
    add("chain f16 dual 64x48", "mp_plan_add_dual_pw_f16", *chain16_dual(n=4, h=64, w=48))
    bad("mp_plan_add_dual_pw_f16", chain16_dual(), [0, 1, 5, 9, 10], zero=(16, 0))

    def chain32(form, n=2, cm=64, ce=256, cr=64, h=16, w=12):
        mid, res, x0, wd, sd, bd, w3, s3, b3, w1, s1, b1, y, z = A(14)
        if form == "down-sample":
            res = None
        else:
            x0 = wd = sd = bd = None
        if form == "expand only":
            w1 = s1 = b1 = z = None
        return [mid, res, x0, wd, sd, bd, w3, s3, b3, w1, s1, b1, y, z, n, cm, ce, cr, h, w]

    for form in ("down-sample", "chain", "expand only"):  # info[11] = 4, 2, 8
        add(f"chain f32 {form}", "mp_plan_add_expand_reduce", *chain32(form))
        add(f"chain f32 {form} 64x48 N=128", "mp_plan_add_expand_reduce", *chain32(form, n=128, h=64, w=48))
    add("chain f32 both residual sources", "mp_plan_add_expand_reduce", *[a if a is not None else A() for a in chain32("down-sample")])
    add("chain f32 width unsupported", "mp_plan_add_expand_reduce", *chain32("chain", cr=32))
    add("chain f32 9x7 unsupported", "mp_plan_add_expand_reduce", *chain32("chain", h=9, w=7))
    bad("mp_plan_add_expand_reduce", chain32("chain"), [0, 1, 6, 7, 10, 12, 13], zero=(18, 0))
    add("barrier", "mp_plan_add_barrier")
    add("set lane 0", "mp_plan_set_lane", 0)

    # ---- first conv of the network from the fp32 image
    for fn in ("mp_plan_add_stem_conv", "mp_plan_add_stem_conv_f16"):
        for n, h, w in ((128, 256, 192), (1, 512, 512), (2, 64, 96)):
            add(f"{fn} {h}x{w} N={n}", fn, *(A(4) + [1, A(), n, h, w]))
        add(f"{fn} odd rows unsupported", fn, *(A(4) + [0, A(), 2, 63, 96]))
        add(f"{fn} 40 columns unsupported", fn, *(A(4) + [0, A(), 2, 64, 40]))
        bad(fn, A(4) + [1, A(), 2, 64, 96], [0, 1, 2, 3, 5], zero=(7, 0))

    # ---- element-wise kinds
    add("maxpool", "mp_plan_add_maxpool", *(A(2) + [2, 64, 64, 48]))
    bad("mp_plan_add_maxpool", A(2) + [2, 64, 64, 48], [0, 1], zero=(4, 0))
    for fn in ("mp_plan_add_fuse_sum", "mp_plan_add_fuse_sum_f16"):
        for terms in (1, 2, 3):
            t = A(terms) + [None] * (3 - terms)
            add(f"{fn} {terms} terms", fn, A(), t[0], 2, t[1], 4 if terms >= 2 else 0, t[2], 8 if terms >= 3 else 0, A(), 2, 32, 64, 48, terms & 1)
        good = A(2) + [2, None, 0, None, 0, A(), 2, 32, 64, 48, 1]
        bad(fn, good, [0, 1, 7], zero=(9, 0))
    for to_c8 in (1, 0):
        add(f"layout to_c8={to_c8}", "mp_plan_add_layout_f16", to_c8, *(A(2) + [2, 17, 64, 48]))
    bad("mp_plan_add_layout_f16", [1] + A(2) + [2, 17, 64, 48], [1, 2], zero=(6, 0))
    add("set lane 2", "mp_plan_set_lane", 2)
    for c8 in (0, 1):
        a, b, o = A(3)
        add(f"concat c8={c8}", "mp_plan_add_concat", a, 32, b, 17, o, 2, 128, 128, c8)
        add(f"concat 34 + 32 c8={c8}", "mp_plan_add_concat", a, 34, b, 32, o, 1, 16, 12, c8)  # c8: the first tensor must end on a block
        add(f"col slice c8={c8}", "mp_plan_add_col_slice", a, o, 2 * 32 * 128, 208, 96, 112, c8)
        add(f"col slice whole width c8={c8}", "mp_plan_add_col_slice", a, o, 64, 48, 0, 48, c8)
        add(f"col slice past the row c8={c8}", "mp_plan_add_col_slice", a, o, 64, 48, 40, 9, c8)
        add(f"col slice negative start c8={c8}", "mp_plan_add_col_slice", a, o, 64, 48, -1, 8, c8)
    a, b, o = A(3)
    bad("mp_plan_add_concat", [a, 32, b, 17, o, 2, 128, 128, 1], [0, 2, 4], zero=(3, 0))
    bad("mp_plan_add_col_slice", [a, o, 64, 48, 8, 16, 0], [0, 1], zero=(5, 0))

    # ---- lanes
    add("set lane 3", "mp_plan_set_lane", 3)
    add("set lane 4 (out of range)", "mp_plan_set_lane", 4)
    add("set lane -1 (out of range)", "mp_plan_set_lane", -1)
    add("maxpool on lane 3", "mp_plan_add_maxpool", *(A(2) + [1, 3, 8, 8]))
    add("barrier", "mp_plan_add_barrier")
    add("set lane null plan", "mp_plan_set_lane", NULL_PLAN, 1)
    add("barrier null plan", "mp_plan_add_barrier", NULL_PLAN)
    return out


def calls_text():
    """One call per line for the stand-alone replay: function name, then `noplan` (null plan), `null`, `d:<the descriptor's 20 fields>`
    or an integer (a dimension, a flag or a fake address)."""
    def tok(a):
        if a is None:
            return "null"
        if a == NULL_PLAN:
            return "noplan"
        if isinstance(a, int):
            return str(a)
        return "d:" + ",".join(str(getattr(a._obj, f)) for f, _ in _lib.ConvDesc._fields_)  # (ctypes.byref keeps its object)
    return "".join(" ".join([fn] + [tok(a) for a in args]) + "\n" for _, fn, args in calls())


def record():
    """Walk the call list on a fresh plan; what comes back is everything a plan shows of itself without running."""
    lib = _lib.load()
    plan = lib.mp_plan_create()
    assert plan
    try:
        rows = []
        for label, fn, args in calls():
            if args and args[0] == NULL_PLAN:
                rc = getattr(lib, fn)(None, *args[1:])
            else:
                rc = getattr(lib, fn)(plan, *args)
            rows.append([label, rc, lib.mp_plan_size(plan)])
        info = (ctypes.c_int64 * 12)()
        entries = []
        for i in range(lib.mp_plan_size(plan)):
            for j in range(12):
                info[j] = -7  # every value is written
            assert lib.mp_plan_entry_info(plan, i, info) == 0
            entries.append(list(info))
        size = lib.mp_plan_size(plan)
        errors = {"index -1": lib.mp_plan_entry_info(plan, -1, info), "index = size": lib.mp_plan_entry_info(plan, size, info),
                  "null plan": lib.mp_plan_entry_info(None, 0, info), "null info": lib.mp_plan_entry_info(plan, 0, None),
                  "size of a null plan": lib.mp_plan_size(None)}
    finally:
        lib.mp_plan_destroy(plan)
    return {"calls": rows, "entries": entries, "entry_info_errors": errors}


def dumps(rec):
    """One call / one entry per line: a drift shows as the lines that moved."""
    lines = ["{", ' "calls": ['] + [f"  {json.dumps(r)}{',' if i + 1 < len(rec['calls']) else ''}" for i, r in enumerate(rec["calls"])]
    lines += [" ],", ' "entries": ['] + [f"  {json.dumps(e)}{',' if i + 1 < len(rec['entries']) else ''}" for i, e in enumerate(rec["entries"])]
    lines += [" ],", f' "entry_info_errors": {json.dumps(rec["entry_info_errors"], sort_keys=True)}', "}"]
    return "\n".join(lines) + "\n"


def _without_knobs(monkeypatch):
    for k in list(os.environ):  # tests/conftest.py turns the knob switch on: no MP_* knob of the environment may move a geometry
        if k.startswith("MP_"):
            monkeypatch.delenv(k)


def test_plan_calls_and_entry_infos_match_the_fixture(monkeypatch):
    _without_knobs(monkeypatch)
    got = record()
    with open(FIXTURE) as fh:
        want = json.load(fh)
    assert [r[0] for r in got["calls"]] == [r[0] for r in want["calls"]], "the call list changed: record the fixture again"
    moved = [(g, w) for g, w in zip(got["calls"], want["calls"]) if g != w]
    assert not moved, f"return code / plan size moved (got, want): {moved[:8]}"
    assert len(got["entries"]) == len(want["entries"])
    moved = [(i, g, w) for i, (g, w) in enumerate(zip(got["entries"], want["entries"])) if g != w]
    assert not moved, f"entry info moved (index, got, want): {moved[:8]}"
    assert got["entry_info_errors"] == want["entry_info_errors"]
    assert dumps(got) == open(FIXTURE).read()


def test_the_text_form_of_the_call_list_is_current():
    assert calls_text() == open(CALLS_TEXT).read(), "the call list changed: record the fixtures again"


def test_the_call_list_reaches_every_kind_and_form(monkeypatch):
    """The fixture is only as good as what it walks: every historical kind id, every fp32 conv alternative (direct tile variants,
    streaming 1x1, GEMM in its plain / gathered / four-phase forms, both small-problem forms), every fused-block form the builders
    produce, the three fp16 chain forms and the three fp32 chain forms, the Winograd cout tiles 64 / 32 / 32 of the 8x6 layer."""
    _without_knobs(monkeypatch)
    rec = record()
    by_kind = {}
    for e in rec["entries"]:
        by_kind.setdefault(e[0], []).append(e)
    assert sorted(by_kind) == list(range(16))
    assert {e[3] for e in by_kind[0]} >= set(range(V_COUNT)) | {POINTWISE, GEMM, SMALL, SMALL_WIDE}
    gemm = [e for e in by_kind[0] if e[3] == GEMM]
    assert {(e[1], e[2], e[9], e[11]) for e in gemm} >= {(1, 1, 1, 0), (1, 2, 1, 1), (3, 2, 1, 1), (2, 1, 4, 1)}
    direct = [e for e in by_kind[0] if e[3] < V_COUNT]
    assert {e[1] for e in direct} == {1, 2, 3, 7} and {e[2] for e in direct} == {1, 2} and {e[11] for e in direct} == {0, 1}
    assert any(e[9] > 1 for e in direct) and any(e[9] == 1 and e[10] == 2 for e in direct)  # image groups; row tiles of a 64-row map
    assert {e[3] for e in by_kind[8]} == {0, 1, 2, 4, 5}  # (form 3, the four-wave second structure, is not built any more)
    assert {e[3] for e in by_kind[10]} == {0, 1, 2} and {(e[3], e[11]) for e in by_kind[13]} == {(1, 4), (0, 2), (2, 8)}
    wino = {c[0]: i for i, c in enumerate(c for c in rec["calls"] if c[0].startswith("winograd ") and c[1] == 0)}
    tiles = [by_kind[9][wino[f"winograd 256->256 8x6 {k}"]][6] for k in ("N=128", "N=64", "N=128 shares CUs")]
    assert tiles == [64, 32, 32], tiles
    f16 = {e[3] for e in by_kind[3]}
    assert f16 & set(range(5)) and f16 & set(range(5, 10)) and f16 & set(range(10, 20)) and f16 & (set(range(25, 37)) | {45, 46, 47}) and f16 & set(range(37, 45))
    rcs = {c[1] for c in rec["calls"]}
    assert rcs == {0, -1, -2, -3}, rcs  # ok, null, shape, unsupported


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    for k in [k for k in os.environ if k.startswith("MP_")]:
        del os.environ[k]
    os.environ.setdefault("MINDPOSE_EXPERIMENT_KNOBS", "1")  # as under pytest (no knob is set: none is honoured either way)
    with open(FIXTURE, "w") as fh:
        fh.write(dumps(record()))
    with open(CALLS_TEXT, "w") as fh:
        fh.write(calls_text())
    print(f"wrote {FIXTURE} and {CALLS_TEXT}")
