"""The weight-gradient kernels' multi-tile cases: case tables, a restatement of the host-side geometry, the float64 reference.

Both weight-gradient kernels (csrc/conv_wgrad.hip, csrc/wgrad_f16.hip) are persistent over the pixel axis: a workgroup walks several
pixel tiles and stages tile t + 1 into the other LDS buffer while the matrix cores work on tile t.  Small test shapes give every
workgroup ONE tile; the tables here are shapes (and MP_* knobs) that give a workgroup three tiles or more on every kernel
instantiation, form and reduce kernel.  `geometry32` / `geometry16` restate `wgrad_geometry` and `geometry` / `geometry_dma` in
Python so that each row can say which path it reaches; tests/test_wgrad_matrix_cpu.py asserts those properties and checks the
restatement against the library's workspace queries and against the launch it builds (`launch_words`, host-only),
tests/test_gpu_wgrad_tiles.py runs the rows.
"""
import ctypes
import functools
import random
from types import SimpleNamespace

from mindpose_amd import _lib
from tests import f16_matrix as fm

# ---- tables -------------------------------------------------------------------------------------------------------------------
# (n, cin, cout, k, s, h, w), knobs, the properties the row is there for (checked by test_wgrad_matrix_cpu.py against geometry32)
F32_CASES = [
    ((5, 390, 500, 3, 1, 20, 12), {}, dict(kernel="pipe", R=9, rows=(9, 9, 2), n_tiles=15, splits=4, per_wg=(4, 4, 4, 3), stale=True,
                                           ragged_channels=True)),
    ((11, 512, 512, 1, 1, 8, 8), {}, dict(kernel="pipe", n_tiles=11, splits=4, per_wg=(3, 3, 3, 2))),
    ((5, 512, 512, 1, 2, 40, 16), {}, dict(kernel="pipe", R=7, rows=(7, 7, 6), n_tiles=15, splits=4, stale=True)),
    ((5, 390, 500, 3, 2, 32, 16), {}, dict(kernel="pipe", R=6, rows=(6, 6, 4), n_tiles=15, splits=4, stale=True, ragged_channels=True)),
    ((11, 512, 500, 3, 1, 8, 6), {}, dict(kernel="simple", n_tiles=11, splits=4)),
    ((9, 512, 512, 3, 2, 16, 12), {}, dict(kernel="simple", n_tiles=9, splits=4)),
    ((9, 512, 512, 1, 2, 16, 12), {}, dict(kernel="simple", n_tiles=9, splits=4)),
    ((11, 512, 512, 1, 1, 8, 6), {}, dict(kernel="simple", n_tiles=11, splits=4)),
    ((25, 256, 512, 4, 2, 8, 6), {}, dict(kernel="simple", n_tiles=25, splits=8, per_wg=(4, 3, 3, 3, 3, 3, 3, 3))),
    ((5, 512, 512, 3, 1, 40, 12), {"MP_WGRAD_SIMPLE": "1"}, dict(kernel="simple", R=16, rows=(16, 16, 8), n_tiles=15, splits=4,
                                                                  forced=True)),
    ((50, 32, 32, 3, 1, 16, 12), {}, dict(reduce="grouped16", splits=100, rounds=1, tail=(2, 3))),
    ((9, 64, 64, 3, 1, 20, 12), {}, dict(reduce="grouped4", splits=27, rounds=1, tail=(2, 3))),
    ((13, 288, 288, 3, 1, 8, 8), {}, dict(reduce="plain", splits=12, rounds=1, tail=(4, 4))),
]

# knobs: the MP_WGRAD16_* suffix -> value
_S2STEM = (5, 3, 64, 3, 2, 40, 24)
F16_CASES = [
    ((5, 40, 24, 3, 1, 40, 12), dict(WGS=4), dict(form="dma32", planes=False, R=16, rows=(16, 16, 8), tiles=15, per_split=(8, 7),
                                                  stale=True, ragged_channels=True)),
    ((5, 72, 80, 3, 1, 20, 12), dict(WGS=8), dict(form="wide", planes=False, R=9, tiles=15, per_split=(8, 7), ksteps=4, stale=True)),
    ((5, 72, 80, 3, 1, 22, 20), dict(WGS=8), dict(form="wide", planes=False, tiles=30, per_split=(15, 15), ksteps=3)),
    ((5, 72, 80, 3, 1, 20, 12), dict(WGS=8, WIDE=0), dict(form="dma32", planes=False, tiles=10, per_split=(10,))),
    ((5, 72, 80, 3, 1, 40, 12), dict(WGS=8, DMA=0), dict(form="reg", nbuf=2, tiles=15, per_split=(15,), stale=True)),
    (_S2STEM, dict(WGS=3), dict(form="narrow", planes=True, tiles=15, per_split=(5, 5, 5), stale=True)),
    (_S2STEM, dict(WGS=3, NARROW=0), dict(form="dma32", planes=True, tiles=15, per_split=(15,))),
    (_S2STEM, dict(WGS=3, PLANES=0), dict(form="narrow", planes=False, tiles=20, per_split=(7, 7, 6))),
    (_S2STEM, dict(WGS=3, DMA=0), dict(form="reg", nbuf=2, tiles=25, per_split=(25,))),
    ((5, 32, 64, 3, 2, 40, 24), dict(WGS=4), dict(form="dma32", planes=True, per_split=(8, 7))),
    ((5, 32, 64, 3, 2, 40, 24), dict(WGS=4, PLANES=0), dict(form="dma32", planes=False, per_split=(10, 10))),
    ((5, 72, 136, 3, 2, 40, 24), dict(WGS=12), dict(form="wide", planes=True, tiles=50, per_split=(25, 25), ksteps=1)),
    ((5, 72, 136, 3, 2, 40, 24), dict(WGS=12, PLANES=0), dict(form="wide", planes=False, ksteps=2)),
    ((7, 72, 250, 1, 1, 28, 12), dict(WGS=8), dict(form="wide", planes=False, tiles=21, per_split=(21,), stale=True)),
    ((7, 32, 17, 1, 1, 40, 12), dict(WGS=2), dict(form="dma32", planes=False, tiles=21, per_split=(11, 10), ragged_channels=True)),
    ((7, 72, 80, 1, 2, 44, 12), dict(WGS=8), dict(form="wide", planes=True, tiles=35, per_split=(18, 17), stale=True)),
    ((7, 32, 48, 1, 2, 44, 12), dict(WGS=2), dict(form="dma32", planes=True, tiles=14, per_split=(14,))),
    ((7, 48, 32, 4, 2, 36, 6), dict(WGS=2), dict(form="dma32", tiles=14, per_split=(14,))),
    ((7, 48, 32, 4, 2, 36, 6), dict(WGS=2, DMA=0), dict(form="reg", nbuf=2, tiles=14, per_split=(14,))),
    ((3, 16, 24, 3, 2, 12, 200), dict(WGS=2, DMA=0), dict(form="reg", nbuf=1, R=1, tiles=18, per_split=(9, 9))),
    ((100, 32, 32, 3, 1, 16, 12), dict(), dict(reduce="grouped16", splits=100, rounds=1, tail=(2, 3))),
    # the instantiations the rows above leave out: narrow k3s1, register-staged <1,1> and <1,2>
    ((5, 12, 40, 3, 1, 40, 12), dict(WGS=3), dict(form="narrow", planes=False, tiles=15, per_split=(5, 5, 5), stale=True,
                                                  ragged_channels=True)),
    ((7, 32, 17, 1, 1, 40, 12), dict(WGS=2, DMA=0), dict(form="reg", nbuf=2, tiles=21, per_split=(11, 10), ragged_channels=True)),
    ((7, 32, 48, 1, 2, 44, 12), dict(WGS=2, DMA=0), dict(form="reg", nbuf=2, tiles=14, per_split=(14,))),
]

# mp_f16_conv_wgrad_grouped, three layers per launch
F16_GROUPED_CASES = [
    ((5, 72, 80, 3, 1, 20, 12), dict(WGS=16), 3),
    (_S2STEM, dict(WGS=4), 3),
]


def case_id(case, knobs):
    n, cin, cout, k, s, h, w = case
    tail = "".join(f"-{key}{val}" for key, val in knobs.items()).replace("MP_WGRAD_", "")
    return f"n{n}_{cin}to{cout}_k{k}s{s}_{h}x{w}{tail}"


def env16(knobs):
    """{"WGS": 4} -> {"MP_WGRAD16_WGS": "4"}"""
    return {f"MP_WGRAD16_{key}": str(val) for key, val in knobs.items()}


def geo16_kwargs(knobs):
    names = {"WGS": "wgs", "DMA": "dma", "WIDE": "wide", "PLANES": "planes", "NARROW": "narrow"}
    return {names[key]: (int(val) if key == "WGS" else bool(int(val))) for key, val in knobs.items()}


def out_hw(k, s, h, w):
    pad = 1 if k == 4 else k // 2
    return pad, (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1


def desc(case):
    n, cin, cout, k, s, h, w = case
    pad, ho, wo = out_hw(k, s, h, w)
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=s, pad_top=pad, pad_left=pad, conv_h=ho, conv_w=wo,
                         out_h=ho, out_w=wo, out_mul=1, out_rep=1, out_off_y=0, out_off_x=0, relu=0, flags=0)


# ---- geometry restatement -------------------------------------------------------------------------------------------------------
def _reduce(count, splits):
    """(kernel, unrolled rounds, (fewest, most) slabs a thread takes in the tail loop) of the slab reduce - the thresholds of
    `wgrad_reduce_choice` (csrc/wgrad_common.h), restated: the independent check of the one place they live."""
    if count <= 18432 and splits >= 64:
        name, g = "grouped16", 16
    elif count <= 73728 and splits >= 16:
        name, g = "grouped4", 4
    else:
        return "plain", splits // 8, (splits % 8, splits % 8)
    rounds, tails = 0, []
    for lane in range(g):
        k, r = lane, 0
        while k + 3 * g < splits:
            k, r = k + 4 * g, r + 1
        tails.append(len(range(k, splits, g)))
        rounds = max(rounds, r)
    return name, rounds, (min(tails), max(tails))


def _rows(tile, tiles_y, R, ho):
    return min(R, ho - (tile % tiles_y) * R)


def _stale(lists, tiles_y, R, ho, nbuf):
    for tiles in lists:
        held_full = [False] * nbuf
        for i, t in enumerate(tiles):
            b = i % nbuf
            if _rows(t, tiles_y, R, ho) < R:
                if held_full[b]:
                    return True
            else:
                held_full[b] = True
    return False


def stale_short_tile(geo):
    """True when some workgroup stages a short tile (Ho % R rows) into an LDS buffer that earlier in the same workgroup held a full
    tile: the rows behind the short tile must read as zeros, not as what the buffer held."""
    return _stale(geo.tile_lists, geo.tiles_y, geo.R, geo.ho, geo.nbuf)


def geometry32(n, cin, cout, k, s, h, w, simple=False):
    """`wgrad_geometry` of csrc/conv_wgrad.hip."""
    pad, ho, wo = out_hw(k, s, h, w)
    r0 = min(max(192 // wo, 1), ho)
    vec = w % 4 == 0 and wo % 4 == 0 and k != 4 and not simple
    R = r0
    if vec:
        budget = 78
        while True:
            rin, wp = (R - 1) * s + k, max((wo - 1) * s + k, pad + w)
            xplane, zpitch = (rin * wp + 31) // 32 * 32 + 2, (R * wo + 31) // 32 * 32 + 2
            lds = 2 * 32 * (xplane + zpitch) * 4
            if (32 * (R * wo // 4) <= 6 * 256 and 32 * rin * (w // 4) <= 9 * 256 and lds <= budget * 1024 and zpitch < 65536
                    and 32 * xplane < 65536):
                break
            if R == 1:
                if budget == 78:
                    budget, R = 150, r0
                    continue
                vec = False
                break
            R -= 1
    if not vec:
        R = r0
        while True:
            rin, wp = (R - 1) * s + k, (wo - 1) * s + k
            lds = 32 * ((rin * wp | 1) + ((((R * wo + 3) & ~3) + 1) | 1)) * 4
            if lds <= 150 * 1024 or R == 1:
                break
            R = (R + 1) // 2
        if lds > 150 * 1024:
            return None
    tiles_y = (ho + R - 1) // R
    n_tiles = n * tiles_y
    out_tiles = ((cout + 31) // 32) * ((cin + 31) // 32)
    splits = min(max(1024 // out_tiles, 1), n_tiles, 256)
    count = cout * cin * k * k
    red, rounds, tail = _reduce(count, splits)
    return SimpleNamespace(kernel="pipe" if vec else "simple", k=k, s=s, R=R, ho=ho, wo=wo, tiles_y=tiles_y, n_tiles=n_tiles, splits=splits,
                           tile_lists=[list(range(b, n_tiles, splits)) for b in range(splits)], nbuf=2 if vec else 1,
                           rows=tuple(_rows(t, tiles_y, R, ho) for t in range(tiles_y)), count=count, reduce=red, reduce_rounds=rounds,
                           reduce_tail=tail, lds_bytes=lds)


_DMA_PIECES, _DMA_PIECES_WIDE = 28, 12
_NZ, _NX = 4, 10


def _geometry_dma(cin, cout, k, s, w, ho, wo, pad, wide, planes, narrow):
    """`geometry_dma` of csrc/wgrad_f16.hip: None, or (form index, R, K, P, planes on, lds bytes)."""
    wide = wide and k <= 3 and cin > 32 and cout > 32
    planes = planes and s == 2
    narrow = narrow and k == 3 and cin <= 16 and cout > 16
    P = max(w + 2 * pad, wo)
    px = P
    if planes:
        P = max((w + 2 * pad + 1) // 2, wo)
        px = 2 * P
    for form in ([1, 0] if wide else [2, 0] if narrow else [0]):
        tbx, tbz = {1: 8, 2: 2, 0: 4}[form], 8 if form else 4
        np_ = _DMA_PIECES_WIDE if form == 1 else _DMA_PIECES
        for budget in (78 * 1024, 150 * 1024):
            for R in range(min(ho, 16), 0, -1):
                rin = (R - 1) * s + k
                K = (R * P + 31) // 32 * 32
                xneed = max(s * (K - 1) + (k - 1) * px + (k - 1) + 1, rin * px)
                if planes:
                    xneed = 2 * max(s * (K - 1) + ((k - 1) >> 1) * px + (k - 1) + 1, ((rin + 1) >> 1) * px)
                xslots, zslots = (xneed + 11) // 16 * 16 + 4, K + 4 + (16 - K % 16 if K % 16 else 0)
                pieces = (tbx * xslots + 63) // 64 + (tbz * zslots + 63) // 64
                lds = 2 * pieces * 64 * 16
                if pieces > 4 * np_ or lds > budget:
                    continue
                return form, R, K, P, planes, lds
    return None


def geometry16(n, cin, cout, k, s, h, w, wgs=512, dma=True, wide=True, planes=True, narrow=True, n_jobs=1):
    """`geometry` + `geometry_dma` of csrc/wgrad_f16.hip (the keyword arguments are the MP_WGRAD16_* knobs)."""
    pad, ho, wo = out_hw(k, s, h, w)
    found = _geometry_dma(cin, cout, k, s, w, ho, wo, pad, wide, planes, narrow) if dma else None
    if found:
        idx, R, K, P, planes_on, lds = found
        form, nbuf = ("dma32", "wide", "narrow")[idx], 2
    else:
        idx, planes_on, form, P = 0, False, "reg", max(w + 2 * pad, wo)
        for nbuf, budget in ((2, 78 * 1024), (2, 150 * 1024), (1, 150 * 1024)):
            for R in range(min(ho, 16), 0, -1):
                rin = (R - 1) * s + k
                K = (R * P + 31) // 32 * 32
                xrows = max(s * (K - 1) + (k - 1) * P + (k - 1) + 1, rin * P)
                lds = nbuf * (K + xrows) * 40 * 2
                if R * wo * 4 <= _NZ * 256 and rin * w * 4 <= _NX * 256 and lds <= budget:
                    found = True
                    break
            if found:
                break
        if not found:
            return None
    tiles_y = (ho + R - 1) // R
    tiles = n * tiles_y
    tw_o, tw_i = 64 if idx else 32, {1: 64, 2: 16, 0: 32}[idx]
    ct = ((cout + tw_o - 1) // tw_o) * ((cin + tw_i - 1) // tw_i)
    target = wgs if wgs >= 1 else 512
    splits = (target if idx == 1 else target + target // 2) // (ct * n_jobs) if n_jobs > 1 else target // ct
    splits = min(max(splits, 1), tiles)
    tps = (tiles + splits - 1) // splits
    splits = (tiles + tps - 1) // tps
    count = cout * cin * k * k
    red, rounds, tail = _reduce(count, splits)
    return SimpleNamespace(form=form, planes=planes_on, k=k, s=s, R=R, ho=ho, wo=wo, P=P, K=K, ksteps=K // 32, nbuf=nbuf, tiles_y=tiles_y,
                           tiles=tiles, splits=splits, tiles_per_split=tps, last_split=tiles - (splits - 1) * tps,
                           tile_lists=[list(range(b * tps, min((b + 1) * tps, tiles))) for b in range(splits)],
                           rows=tuple(_rows(t, tiles_y, R, ho) for t in range(tiles_y)), count=count, reduce=red, reduce_rounds=rounds,
                           reduce_tail=tail, lds_bytes=lds, n_jobs=n_jobs)


def max_tiles_per_workgroup(geo):
    return max(len(t) for t in geo.tile_lists)


# ---- the library's own answer (host-only) -------------------------------------------------------------------------------------
def lib_splits32(case, **env):
    with fm.knobs(**env):
        nb = _lib.load().mp_conv_wgrad_workspace_bytes(ctypes.byref(desc(case)))
    return nb // (case[1] * case[2] * case[3] * case[3] * 4)


def lib_splits16(case, n_jobs=1, **env):
    lib, d = _lib.load(), desc(case)
    with fm.knobs(**env):
        nb = (lib.mp_f16_conv_wgrad_workspace_bytes(ctypes.byref(d)) if n_jobs == 1
              else lib.mp_f16_conv_wgrad_grouped_workspace_bytes(ctypes.byref(d), n_jobs))
    return nb // (n_jobs * case[1] * case[2] * case[3] * case[3] * 4)


# mp_conv_wgrad_launch_words (include/mindpose_hip.h, host-only): the return code, then - after an accepted geometry - the
# non-pointer fields of the kernel parameter block in declaration order, grid, block, LDS bytes, kernel id and slab reduce
_LAUNCH = ["grid_x", "grid_y", "grid_z", "block", "lds_bytes", "half", "form", "ks", "stride", "reduce_g", "reduce_blocks", "reduce_jobs"]
WORDS32 = ["rc"] + ("N Cin H W Cout Ho Wo pad R Rin Wp xplane zpitch tiles_y n_tiles splits ci_tiles vec zq xw4").split() + _LAUNCH
WORDS16 = ["rc"] + ("N Cin C8in H W Cout C8out Ho Wo pad R P Px Rin K xrows tiles_y tiles splits tiles_per_split ci_tiles nbuf magic_wo magic_w "
                    "xslots zslots pieces x_pieces z_base wide co_tiles plane_slots magic_px magic_xs magic_zs magic_p n_jobs").split() + _LAUNCH
FORMS16 = ("dma32", "wide", "narrow", "reg")


def launch_words(case, half, n_jobs=0, **env):
    """The launch of a case as the entry point builds it: [rc] after a refusal, else the words of WORDS32 / WORDS16.  n_jobs: 0 = the
    single-layer entry, 1 .. 8 = mp_f16_conv_wgrad_grouped."""
    cap = 64
    buf = (ctypes.c_int64 * cap)()
    with fm.knobs(**env):
        n = _lib.load().mp_conv_wgrad_launch_words(ctypes.byref(desc(case)), int(half), int(n_jobs), buf, cap)
    assert n == 1 or n == len(WORDS16 if half else WORDS32), f"mp_conv_wgrad_launch_words returned {n}"
    return list(buf[:n])


def check_geometry_against_launch(geo, words, half):
    """The restated geometry (geometry32 / geometry16, None = refused) against the launch the library builds."""
    if geo is None:
        assert words[0] != 0 and len(words) == 1, words
        return
    w = SimpleNamespace(**dict(zip(WORDS16 if half else WORDS32, words)))
    assert w.rc == 0 and w.half == half and (w.ks, w.stride) == (geo.k, geo.s)
    reduce_g = {"plain": 0, "grouped4": 4, "grouped16": 16}[geo.reduce]
    if half:
        got = (FORMS16[w.form], w.R, w.K, w.P, w.nbuf, w.plane_slots > 0, w.tiles_per_split, w.tiles, w.splits, w.lds_bytes, w.reduce_g)
        want = (geo.form, geo.R, geo.K, geo.P, geo.nbuf, geo.planes, geo.tiles_per_split, geo.tiles, geo.splits, geo.lds_bytes, reduce_g)
        assert (w.grid_y, w.grid_z, w.reduce_jobs) == (geo.splits, geo.n_jobs, geo.n_jobs)
    else:
        got = (("simple", "pipe")[w.form], w.R, w.tiles_y, w.n_tiles, w.splits, w.lds_bytes, w.reduce_g)
        want = (geo.kernel, geo.R, geo.tiles_y, geo.n_tiles, geo.splits, geo.lds_bytes, reduce_g)
        assert (w.grid_y, w.grid_z, w.reduce_jobs) == (geo.splits, 1, 1)
    assert got == want, (got, want)


def random_draws(count=600, seed=20240607):
    """`count` seeded random (case, fp32 forced simple, MP_WGRAD16_* knobs, jobs) draws over every kernel size, stride and form switch"""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        k, s = rng.choice([(1, 1), (1, 2), (3, 1), (3, 2), (4, 2)])
        case = (rng.randint(1, 40), rng.choice([3, 16, 17, 32, 40, 48, 64, 72, 128, 256, 390, 512]),
                rng.choice([16, 17, 24, 32, 64, 80, 136, 250, 256, 500, 512]), k, s, rng.randint(2, 70), rng.randint(2, 220))
        if k == 4 and (case[5] % 2 or case[6] % 2):
            continue
        simple = rng.random() < 0.3
        knobs = {"WGS": rng.choice([1, 2, 3, 4, 8, 12, 16, 64])} if rng.random() < 0.7 else {}
        knobs.update({key: 0 for key in ("DMA", "WIDE", "PLANES", "NARROW") if rng.random() < 0.25})
        out.append((case, simple, knobs, rng.choice([1, 1, 2, 3, 8])))
    return out


# ---- reference ------------------------------------------------------------------------------------------------------------------
def reference_dw(x, dz, k, s, pad):
    """The weight gradient in float64 on the CPU (autograd of F.conv2d on float64 operands)."""
    import torch
    import torch.nn.functional as F
    wt = torch.zeros(dz.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.detach().cpu().double(), wt, None, stride=s, padding=pad).backward(dz.detach().cpu().double())
    return wt.grad


@functools.lru_cache(maxsize=None)
def operands(case, half, job=0):
    """(x, dz, float64 reference) of a case, computed once per session and left unchanged; half: operands rounded to fp16 first and
    then widened, so that every product is exact in the kernel and in the reference."""
    import torch
    n, cin, cout, k, s, h, w = case
    pad, ho, wo = out_hw(k, s, h, w)
    g = torch.Generator().manual_seed(sum(case) + 1000 * job)
    x, dz = torch.randn(n, cin, h, w, generator=g), torch.randn(n, cout, ho, wo, generator=g)
    if half:
        x, dz = x.half().float(), dz.half().float()
    return x, dz, reference_dw(x, dz, k, s, pad)
