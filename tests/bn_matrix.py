"""The training BatchNorm kernels' forms: case tables, a restatement of the host-side geometry, the float64 reference.

csrc/train_ops.hip runs the fp16 BatchNorm of the amp-O2 step in three forms - one launch with a grid barrier (`bn16_coop_kernel`),
two launches (`bn16_reduce_kernel`, then `bn16_apply_kernel` / `bn16_bwd_apply_kernel`) and apply-only passes on a conv epilogue's
partial slots (`bn16_apply_pre_*`, `bn16_bwd_apply_pre_*`, `bn16_fold_kernel`, `bn16_finalize_kernel`) - and the fp32 BatchNorm as
`bn_reduce_kernel` + `bn_apply_kernel` / `bn_bwd_apply_kernel`.  Which form a call takes, and how it cuts the tensor, is decided on
the host from the shape alone.  This module restates those decisions in Python (no GPU, no library), enumerates the exact
(image, pixel) set every partial slot sums, and holds the float64 reference; tests/test_bn_matrix_cpu.py asserts that every row
below reaches what it is listed for, tests/test_gpu_bn_forms.py runs the rows through the C ABI.
"""
import torch

# ---- constants of csrc/train_ops.hip --------------------------------------------------------------------------------------------
BN_SPLIT = 32            # kBnSplit: image stride of the fp32 reduction
MAX_SPLIT = 256          # kBn16MaxSplit
COOP_MAX_GRID = 128      # kCoopMaxGrid
COOP_MAX_ELEMS = 1 << 19  # MP_BN16_COOP_MAX default (16-byte elements); read once per process, so rows choose by shape
MAX_FOLD_PARTS = 512     # kMaxFoldParts
FOLD_SPLIT = 8           # kFoldSplit
BATCH = 4                # kBatch of the apply-only kernels: 4 x 256 elements per batch
EPS = 1e-5
MOMENTUM = 0.9           # the entries' convention: moving = momentum * moving + (1 - momentum) * batch
U32 = 2.0 ** -24         # unit roundoff of fp32


def c8_of(c):
    return (c + 7) // 8


def ceil_div(a, b):
    return (a + b - 1) // b


# ---- host geometry, one function per function of the library ---------------------------------------------------------------------
def coop_plan(n, c8, hw):
    """bn16_coop_plan: nsplit of the one-launch form, or None when the call takes the two-launch form."""
    if n * c8 * hw > COOP_MAX_ELEMS or c8 > COOP_MAX_GRID:
        return None
    nsplit = min(COOP_MAX_GRID // c8, 32)
    while nsplit > 1 and ceil_div(n * hw, nsplit) < 256:
        nsplit -= 1
    return nsplit


def split(n, c8, hw):
    """bn16_split: image groups x pixel chunks of bn16_reduce_kernel."""
    want = min(max(512 // c8, 32), MAX_SPLIT)
    gi = min(n, want)
    gp = max(want // gi, 1)
    while gp > 1 and ceil_div(hw, gp) < 256:
        gp -= 1
    return gi, gp


def apply_chunks(n, c8, hw):
    """bn16_apply_chunks: chunks of the flat (image, pixel) range per channel block in the two-launch form's second launch."""
    chunks = ceil_div(768, c8)
    while chunks > 1 and (n * hw) // chunks < 1024:
        chunks -= 1
    return chunks


def pre_chunks(n, c8, hw, blocks=1024, floor=1024):
    """bn16_pre_chunks with its two knobs (MP_BN_PRE_BLOCKS, MP_BN_PRE_MIN)."""
    chunks = ceil_div(blocks, c8)
    while chunks > 1 and (n * hw) // chunks < floor:
        chunks -= 1
    return chunks


def prefold(n_parts, above=MAX_FOLD_PARTS):
    """bn16_prefold: (fold launch runs, slots the consumer folds)."""
    return (True, FOLD_SPLIT) if n_parts > above else (False, n_parts)


def fold_ranges(n_parts):
    """slot range [s0, s1) of each of the kFoldSplit blocks of bn16_fold_kernel (possibly empty)."""
    per = ceil_div(n_parts, FOLD_SPLIT)
    return [(f * per, max(f * per, min(f * per + per, n_parts))) for f in range(FOLD_SPLIT)]


def form(n, c, hw):
    return "two" if coop_plan(n, c8_of(c), hw) is None else "coop"


def nsplit16(n, c, hw):
    ns = coop_plan(n, c8_of(c), hw)
    if ns is None:
        gi, gp = split(n, c8_of(c), hw)
        ns = gi * gp
    return ns


def chunk_ranges(per_blk, chunks):
    """[e0, e1) of every chunk of a flat range cut as the apply kernels cut it (len = ceil; trailing chunks may be empty)."""
    ln = ceil_div(per_blk, chunks)
    return [(k * ln, max(k * ln, min(k * ln + ln, per_blk))) for k in range(chunks)]


def batches(e0, e1):
    """element count of each 4 x 256 batch the apply-only kernels walk over [e0, e1)."""
    return [min(256 * BATCH, e1 - b) for b in range(e0, e1, 256 * BATCH)]


def apply_exact(n, hw):
    """the `exact` condition of every kernel that divides the flat index by hw (all but bn16_reduce_kernel)."""
    return n * hw * hw < 2 ** 32


def mulhi_div(e, d):
    """what the kernels compute under `exact`: __umulhi(e, 2^32 / d + 1) - in Python integers."""
    return (e * (2 ** 32 // d + 1)) >> 32


# ---- slices: the (image, pixel) set partial slot sp sums, as flat indices img * hw + pixel ----------------------------------------
def coop_slice(n, hw, nsplit, sp):
    ln = ceil_div(n * hw, nsplit)
    return torch.arange(min(sp * ln, n * hw), min((sp + 1) * ln, n * hw))


def two_slice(n, hw, gi, gp, sp):
    ig, pc = sp % gi, sp // gi
    chunk = ceil_div(hw, gp)
    pix = torch.arange(min(pc * chunk, hw), min((pc + 1) * chunk, hw))
    img = torch.arange(ig, n, gi)
    return (img[:, None] * hw + pix[None, :]).reshape(-1)


def f32_slice(n, hw, sp):
    img = torch.tensor(list(range(sp, n, BN_SPLIT)), dtype=torch.long)
    return (img[:, None] * hw + torch.arange(hw)[None, :]).reshape(-1)


def slices16(n, c, hw):
    """every slot's slice of a reducing fp16 call, in slot order."""
    c8 = c8_of(c)
    ns = coop_plan(n, c8, hw)
    if ns is not None:
        return [coop_slice(n, hw, ns, sp) for sp in range(ns)]
    gi, gp = split(n, c8, hw)
    return [two_slice(n, hw, gi, gp, sp) for sp in range(gi * gp)]


def slices32(n, hw):
    return [f32_slice(n, hw, sp) for sp in range(BN_SPLIT)]


# ---- tables ---------------------------------------------------------------------------------------------------------------------
# reducing fp16 entries: (n, c, hw), the properties the row is there for (asserted by test_bn_matrix_cpu.py)
REDUCING_ROWS = [
    ((28, 12, 12288), dict(form="two", gi=28, gp=9, chunk=1366, last=1360, exact=True, c8=2, near_bound=True)),
    ((29, 12, 12288), dict(form="two", gi=29, gp=8, exact=False, c8=2)),
    ((40, 136, 800), dict(form="two", gi=32, gp=1, c8=17, apply_len=1033, two_images=8)),
    ((6, 32, 49152), dict(form="two", gi=6, gp=21, chunk=2341, last=2332, apply_len=1536, exact=False, c8=4)),
    ((2, 1025, 48), dict(form="two", c8=129, pad=7, under_threshold=True)),
    ((3, 1032, 1), dict(form="two", c8=129, hw1=True)),
    ((7, 12, 24576), dict(form="coop", nsplit=32, exact=True, c8=2)),
    ((8, 12, 24576), dict(form="coop", nsplit=32, exact=False, c8=2)),
    ((7, 40, 919), dict(form="coop", nsplit=25, slice_len=258, straddles=True)),
    ((6, 1024, 96), dict(form="coop", nsplit=1, c8=128)),
    ((6, 1009, 48), dict(form="coop", nsplit=1, c8=127, pad=7)),
    ((3, 9, 1), dict(form="coop", hw1=True, c8=2, pad=7)),
    ((5, 12, 63), dict(form="coop", c8=2, pad=4, odd_hw=True)),
]
ILL_ROWS = [(28, 12, 12288), (7, 40, 919)]  # also run with z = 24 + 0.25 randn (variance 1e-4 of the second moment)
MODES = [(0, 0), (1, 0), (0, 1), (1, 1)]   # (relu, residual)

# apply-only entries: (n, c, hw), n_parts, knobs, properties
_SMALL = (6, 17, 48)
APPLY_ROWS = [((_SMALL, k, {}, dict(fold=k > MAX_FOLD_PARTS))) for k in (1, 63, 64, 65, 511, 512, 513, 4097)] + [
    ((29, 12, 12288), 37, {}, dict(exact=False, c8=2, batches=[1024])),
    ((6, 32, 49152), 6, {}, dict(chunk_len=1152, batches=[1024, 128])),
    ((4, 20, 660), 5, {"MP_BN_PRE_BLOCKS": "3", "MP_BN_PRE_MIN": "1"}, dict(chunks=1, chunk_len=2640, batches=[1024, 1024, 592])),
    ((2, 9, 5), 3, {"MP_BN_PRE_BLOCKS": "16", "MP_BN_PRE_MIN": "1"}, dict(chunks=8, chunk_len=2, empty=3)),
    (_SMALL, 37, {"MP_BN_PREFOLD_ABOVE": "4"}, dict(fold=True)),
]
# one grouped call: four jobs drawn from different rows, the first above the fold limit
GROUPED_JOBS = [(_SMALL, 513), ((4, 20, 660), 5), ((2, 9, 5), 3), ((7, 40, 919), 65)]

# fp32 entries (raw ABI): (n, c, hw), properties
F32_ROWS = [
    ((33, 5, 3072), dict(float4=True, trips=3, two_images=1)),
    ((3, 7, 323), dict(float4=False, trips=2)),
    ((2, 6, 4), dict(float4=True, trips=1, idle_threads=True)),
]
F32_ILL_ROW = (33, 5, 3072)


def row_id(shape, *extra):
    n, c, hw = shape
    return f"n{n}_c{c}_hw{hw}" + "".join(f"-{e}" for e in extra)


def pre_knobs(knobs):
    return int(knobs.get("MP_BN_PRE_BLOCKS", 1024)), int(knobs.get("MP_BN_PRE_MIN", 1024))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def make_inputs(shape, ill=False, half=True):
    """seeded CPU inputs as float64 [n, c, hw] tensors holding fp16-representable (half) or fp32-representable values"""
    n, c, hw = shape
    g = torch.Generator().manual_seed(1000 * n + 10 * c + hw + (7 if ill else 0))
    rnd = (lambda t: t.half().double()) if half else (lambda t: t.float().double())
    z = torch.randn(n, c, hw, generator=g)
    z = rnd(24.0 + 0.25 * z if ill else 1.5 * z + 0.3)
    res = rnd(torch.randn(n, c, hw, generator=g))
    dy = rnd(torch.randn(n, c, hw, generator=g))
    gamma = (torch.rand(c, generator=g) + 0.5).float().double()
    beta = (torch.randn(c, generator=g) * 0.1).float().double()
    mm = (torch.randn(c, generator=g) * 0.2).float().double()
    mv = (torch.rand(c, generator=g) + 0.5).float().double()
    return dict(z=z, res=res, dy=dy, gamma=gamma, beta=beta, mm=mm, mv=mv)


def pack_c8(x, pad_value=float("nan")):
    """float64 [n, c, hw] -> fp16 [n, c8, hw, 8]; the padding-channel lanes hold pad_value (NaN: garbage no kernel may let through)"""
    n, c, hw = x.shape
    c8 = c8_of(c)
    full = torch.full((n, c8 * 8, hw), pad_value, dtype=torch.float64)
    full[:, :c] = x
    return full.reshape(n, c8, 8, hw).permute(0, 1, 3, 2).contiguous().half()


def unpack_c8(t, c):
    """fp16 [n, c8, hw, 8] -> (float64 [n, c, hw], the padding lanes as int16 bit patterns)"""
    n, c8, hw, _ = t.shape
    full = t.permute(0, 1, 3, 2).reshape(n, c8 * 8, hw)
    return full[:, :c].double(), full[:, c:].contiguous().view(torch.int16)


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def per_channel(x):
    """[n, c, hw] -> [c, n * hw] with the flat index the slices use"""
    return x.permute(1, 0, 2).reshape(x.shape[1], -1)


def slot_sums(term, slices):
    """float64 [c, slots]: sum of term ([n, c, hw]) over each slice"""
    flat = per_channel(term)
    return torch.stack([flat.index_select(1, idx).sum(dim=1) for idx in slices], dim=1)


def chain_terms(slices):
    """k of the slot bound: the longest fp32 chain a thread of the slot's workgroup adds, ceil(slice count / 256)"""
    return torch.tensor([ceil_div(max(int(idx.numel()), 1), 256) for idx in slices], dtype=torch.float64)


def slot_bounds(term, slices):
    """|slot - exact| <= (k + 6) * 2^-24 * sum |terms|: a chain of k fp32 additions ((k - 1) u), the term's own fp32 roundings
    (x-hat and the product: 3 u) and slack for the conversion; the fp64 combination behind it adds nothing at this scale"""
    return (chain_terms(slices) + 6.0)[None, :] * U32 * slot_sums(term.abs(), slices)


def forward_ref(z, gamma, beta, res, relu, mm, mv, stats=None):
    """float64 BatchNorm forward in training mode; `stats` = (mean, invstd) to evaluate y at instead of the reference's own"""
    n, c, hw = z.shape
    count = n * hw
    eps, mom = float(torch.tensor(EPS, dtype=torch.float32)), float(torch.tensor(MOMENTUM, dtype=torch.float32))
    mean = z.mean(dim=(0, 2))
    var = ((z - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    invstd = 1.0 / torch.sqrt(var + eps)
    unbiased = var * count / (count - 1) if count > 1 else var
    m, i = (mean, invstd) if stats is None else stats
    sc = gamma * i
    y = z * sc[None, :, None] + (beta - m * sc)[None, :, None]
    if res is not None:
        y = y + res
    if relu:
        y = y.clamp_min(0.0)
    return dict(mean=mean, var=var, invstd=invstd, mm=mom * mm + (1.0 - mom) * mean, mv=mom * mv + (1.0 - mom) * unbiased, y=y,
                eps=eps, mom=mom)


def backward_ref(dy, z, y_given, gamma, mean, invstd, relu):
    """float64 BatchNorm backward at the statistics the entry is given; the mask is y_given > 0"""
    n, c, hw = z.shape
    g = dy * (y_given > 0) if relu else dy
    xh = (z - mean[None, :, None]) * invstd[None, :, None]
    dbeta, dgamma = g.sum(dim=(0, 2)), (g * xh).sum(dim=(0, 2))
    m = n * hw
    dz = (gamma * invstd)[None, :, None] * (g - dbeta[None, :, None] / m - xh * dgamma[None, :, None] / m)
    return dict(g=g, xh=xh, dbeta=dbeta, dgamma=dgamma, dz=dz)


def stat_bounds(z, sum_bound, sumsq_bound, ref):
    """bounds on the saved statistics from bounds on sum z and sum z^2 (per channel):
    mean: sum bound / count + 2^-24 |mean| (the fp32 store); var = E z^2 - mean^2: sumsq bound / count + 2 |mean| dmean;
    invstd, relative: 1/2 dvar / (var + eps) + 2^-23 (fp64 rsqrt, the fp32 store)"""
    count = z.shape[0] * z.shape[2]
    dmean = sum_bound / count + U32 * ref["mean"].abs()
    dvar = sumsq_bound / count + 2.0 * ref["mean"].abs() * dmean
    dinv_rel = 0.5 * dvar / (ref["var"] + ref["eps"]) + 2.0 * U32
    return dmean, dvar, dinv_rel


def moving_bound(ref, old, new, dstat):
    """momentum * old + (1 - momentum) * stat in fp32: the statistic's own error scaled, three fp32 roundings on the two products"""
    return (1.0 - ref["mom"]) * dstat + 3.0 * U32 * ((ref["mom"] * old).abs() + (new - ref["mom"] * old).abs())


def tol16(ref):
    """the project's fp16 rule (tests/test_gpu_train_f16.py::_close16): 2^-9 |ref| + 2e-4 max |ref|"""
    return ref.abs() * 2.0 ** -9 + 2e-4 * ref.abs().max()


def spread_partials(a, b, c, n_parts, seed):
    """exact per-channel sums a, b (float64 [c]) spread over n_parts fp32 slots with uneven positive weights, in the conv
    epilogue's layout [c8][n_parts][8][2]"""
    c8 = c8_of(c)
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(n_parts, generator=g).double() + 0.1
    w = w / w.sum()
    full = torch.zeros(c8 * 8, 2, dtype=torch.float64)
    full[:c, 0], full[:c, 1] = a, b
    return (full.reshape(c8, 1, 8, 2) * w.reshape(1, n_parts, 1, 1)).float().contiguous()


def partial_totals(p, c):
    """what the slots hold: float64 per-channel totals of fp32 [c8][n_parts][8][2], and the totals of the slots' magnitudes"""
    c8 = p.shape[0]
    tot = p.double().sum(dim=1).reshape(c8 * 8, 2)[:c]
    mag = p.double().abs().sum(dim=1).reshape(c8 * 8, 2)[:c]
    return tot, mag
