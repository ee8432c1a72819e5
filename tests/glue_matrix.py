"""The case lists and CPU references of the kernels a training step runs BETWEEN its convolutions and BatchNorms: the exchange-unit
sums and their backward, the fan-out gradient sum, max-pool forward / backward, the stem weight gradient, the sub-pixel phase gather
and the optimizer tail (AdamW, scaled AdamW, the four other optimizers, the overflow check).  Importable without a GPU;
tests/test_glue_matrix_cpu.py holds the floors of the lists and checks the references against each other,
tests/test_gpu_train_glue.py runs every case on the device.

Every launch below caps its grid and strides over the rest.  ENTRIES states, per entry point, that cap in units of one thread's
loop trip, with the source line it restates, and how many trips (`units`) and elements a case holds; every list has a case that
exceeds its cap by less than 2 %, so the second grid pass runs with a ragged end.
"""
import numpy as np
import torch

U16, U24 = 2.0 ** -11, 2.0 ** -24  # unit round-offs of fp16 and fp32


def ceil_div(a, b):
    return -(-a // b)


def c8_of(c):
    return ceil_div(c, 8)


def is_pow2(v):
    return v >= 1 and v & (v - 1) == 0


# ---- cases --------------------------------------------------------------------------------------------------------------------------

# (n, c, h, w, scales, relu) - fp32 NCHW; scales are powers of two that divide h and w (mp_fuse_upsample_sum refuses the rest)
FUSE32_CASES = [
    (1, 3, 4, 8, (2,), 1),               # vector path (w % 4 == 0), 96 elements: one partly filled block
    (2, 6, 8, 24, (2, 4, 8), 1),         # three terms
    (2, 5, 4, 12, (1,), 0),              # scale 1, no ReLU
    (1, 7, 8, 16, (1, 1), 1),            # a repeated scale 1
    (2, 3, 4, 4, (2, 4), 0),             # w == 4: one quad per row
    (3, 5, 24, 20, (4, 2), 1),           # 1800 quads: several blocks, descending scales
    (2, 3, 4, 6, (1, 2), 1),             # scalar path (w % 4 != 0): w = 6
    (1, 5, 6, 10, (2,), 0),              # w = 10
    (2, 2, 4, 10, (1, 2), 0),            # w = 10 with scale 1
    (3, 2, 2, 14, (1, 2, 2), 1),         # w = 14, three terms
    (3, 1, 3, 7, (1,), 0),               # 63 elements: odd extents, scale 1 only
    (1, 1, 5, 3, (1, 1, 1), 1),          # 15 elements
    (2, 7, 10, 18, (2, 1), 1),           # 2520 elements: several blocks of the scalar kernel
    (1, 131073, 8, 8, (2, 4), 1),        # vector path over the cap: 2,097,168 quads (8.4 M floats)
    (1, 174763, 2, 6, (1, 2), 0),        # scalar path over the cap: 2,097,156 elements
]

# (n, c, h, w, scales, relu) - channel-blocked fp16; the entry takes the fast kernel when `f16_fuse_fast`, else the generic one
FUSE16_CASES = [
    (1, 8, 1, 1, (1,), 1),               # one unit; h = w = 1: the d == 1 branch of the reciprocal division, twice
    (2, 17, 1, 12, (1, 1), 0),           # h = 1
    (2, 8, 12, 1, (1,), 1),              # w = 1
    (3, 17, 21, 13, (1,), 1),            # odd map at scale 1
    (2, 48, 6, 10, (2,), 0),             # 3 x 5 low-resolution map
    (2, 17, 12, 20, (2, 4), 1),
    (1, 8, 24, 40, (2, 4, 8), 1),        # 3 x 5 at scale 8
    (1, 48, 14, 18, (1, 2), 0),          # 7 x 9 at scale 2
    (2, 8, 12, 18, (3,), 1),             # generic kernel: a scale that is no power of two
    (1, 17, 12, 18, (2, 3), 0),
    (2, 48, 12, 18, (2, 3, 6), 1),
    (1, 8 * 131073 - 3, 4, 4, (2, 4), 1),    # fast kernel over the cap: 2,097,168 units, three padding lanes in the last block
    (1, 8 * 233017 - 5, 3, 3, (3,), 0),      # generic kernel over the cap: 2,097,153 units
]

# (half, operands, 16-byte units)
SUM_CAP = 4096 * 256
SUM_CASES = [(half, k, units) for half in (0, 1) for k in (2, 3, 4) for units in (1, 255, 256, 257)] + \
            [(0, 4, SUM_CAP + 7), (1, 3, SUM_CAP + 7), (1, 2, SUM_CAP + 7)]

POOL_MAPS = [(1, 1), (2, 3), (3, 2), (5, 5), (7, 12), (13, 9), (18, 14)]
POOL_KINDS = ("randn", "ties")
# (n, c, h, w)
POOL_FWD_CASES = [(2, 3, h, w) for h, w in POOL_MAPS] + [(1, 116509, 5, 5)]   # 116509 * 9 = 1,048,581 outputs
POOL_BWD_CASES = [(2, 3, h, w) for h, w in POOL_MAPS] + [(1, 167773, 5, 5)]   # 167773 * 25 = 4,194,325 inputs

# (k, cin, cout, n, h, w)
STEM_CASES = [(k, cin, cout, n, h, w) for k in (3, 7) for cin in (1, 2, 3, 4) for cout in (5, 64)
              for n, h, w in ((1, 7, 9), (1, 8, 8), (3, 30, 22))]

PHASES = [(0, 0), (0, 1), (1, 0), (1, 1)]
# (half, n, c, h, w, py, px): h x w is the OUTPUT (one phase of a 2h x 2w map)
GATHER_CASES = [(half, 2, c, h, w, py, px) for half in (0, 1) for c in (3, 8, 17) for h, w in ((1, 1), (5, 7), (12, 10)) for py, px in PHASES] + \
               [(0, 1, 119838, 5, 7, 1, 0), (1, 1, 8 * 119838 - 1, 5, 7, 0, 1)]   # 119838 * 35 = 4,194,330 outputs

OPT_CAP = 256 * 16 * 256
OPT_COUNTS = [1, 3, 255, 256, 257, OPT_CAP + 5]
# name -> (kind, hyper[5]) of mp_optimizer_step; lr, grad_scale and weight decay are OPT_LR, OPT_GRAD_SCALE, OPT_WD
OPT_VARIANTS = {
    "adam-step3": (1, (0.9, 0.999, 1e-8, 0.9 ** 3, 0.999 ** 3)),
    "sgd-first-step": (2, (0.9, 0.1, 0.0, 1.0, 0.0)),
    "sgd-dampening": (2, (0.9, 0.1, 0.0, 0.0, 0.0)),
    "sgd-nesterov": (2, (0.9, 0.0, 1.0, 0.0, 0.0)),
    "sgd-plain": (2, (0.0, 0.0, 0.0, 0.0, 0.0)),      # momentum == 0: state1 == NULL
    "momentum": (3, (0.9, 0.0, 0.0, 0.0, 0.0)),
    "momentum-nesterov": (3, (0.8, 1.0, 0.0, 0.0, 0.0)),
    "adagrad": (4, (0.0, 0.0, 0.0, 0.0, 0.0)),
}
OPT_LR, OPT_GRAD_SCALE, OPT_WD = 0.05, 0.125, 0.01
ADAMW_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6, wd=0.05)

FINITE_CAP = 256 * 8 * 256 * 4
FINITE_COUNTS = [1, 2, 3, 4, 5, 1027, FINITE_CAP + 7]


def fuse32_units(case):
    n, c, h, w = case[:4]
    return n * c * h * (w // 4) if w % 4 == 0 else n * c * h * w


def f16_fuse_fast(case):
    """the documented condition of mp_f16_fuse_upsample_sum's fast form: every scale a power of two and total * max(h, w) < 2^32"""
    n, c, h, w, scales, _ = case
    return all(is_pow2(s) for s in scales) and n * c8_of(c) * h * w * max(h, w) < 2 ** 32


def fuse16_bwd_cases():
    """mp_f16_fuse_upsample_sum_bwd takes power-of-two scales only: the forward cases that have them"""
    return [c for c in FUSE16_CASES if all(is_pow2(s) for s in c[4])]


class Entry:
    """cap: loop trips one grid pass covers; source: (file of csrc/, the line that sets the block limit - a block is 256 threads);
    units(case): trips of the case; elements(case): its scalar elements; vec: elements per trip where the kernel has a vector width."""

    def __init__(self, cap, source, cases, units, elements=None, vec=1):
        self.cap, self.source, self.cases, self.units, self.elements, self.vec = cap, source, cases, units, elements or units, vec


_planes16 = lambda case: case[0] * c8_of(case[1])  # noqa: E731
ENTRIES = {
    "mp_fuse_upsample_sum": Entry(256 * 32 * 256, ("eltwise_f32.hip", "if (blocks > 256 * 32) blocks = 256 * 32;"), FUSE32_CASES, fuse32_units,
                                  lambda c: c[0] * c[1] * c[2] * c[3], vec=4),
    # one launch per output; the widest is dbase, one thread per element
    "mp_fuse_upsample_sum_bwd": Entry(256 * 32 * 256, ("train_ops.hip", "if (blocks > 256 * 32) blocks = 256 * 32;"), FUSE32_CASES,
                                      lambda c: c[0] * c[1] * c[2] * c[3]),
    "mp_f16_fuse_upsample_sum": Entry(8192 * 256, ("conv_f16.hip", "blocks > 8192 ? 8192"), FUSE16_CASES, lambda c: _planes16(c) * c[2] * c[3]),
    "mp_f16_fuse_upsample_sum_bwd": Entry(8192 * 256, ("train_ops.hip", "if (blocks > 8192) blocks = 8192;"), fuse16_bwd_cases(),
                                          lambda c: _planes16(c) * c[2] * c[3]),
    "mp_sum_tensors": Entry(SUM_CAP, ("train_ops.hip", "if (blocks > 4096) blocks = 4096;"), SUM_CASES, lambda c: c[2]),
    "mp_maxpool3x3s2_same": Entry(256 * 16 * 256, ("eltwise_f32.hip", "if (blocks > 256 * 16) blocks = 256 * 16;"), POOL_FWD_CASES,
                                  lambda c: c[0] * c[1] * ceil_div(c[2], 2) * ceil_div(c[3], 2)),
    "mp_maxpool3x3s2_same_bwd": Entry(16384 * 256, ("sb_train_ops.hip", "if (blocks > 16384) blocks = 16384;"), POOL_BWD_CASES,
                                      lambda c: c[0] * c[1] * c[2] * c[3]),
    "mp_gather_phase": Entry(16384 * 256, ("sb_train_ops.hip", "if (blocks > 16384) blocks = 16384;"), [c for c in GATHER_CASES if not c[0]],
                             lambda c: c[1] * c[2] * c[3] * c[4]),
    "mp_f16_gather_phase": Entry(16384 * 256, ("sb_train_ops.hip", "if (blocks > 16384) blocks = 16384;"), [c for c in GATHER_CASES if c[0]],
                                 lambda c: c[1] * c8_of(c[2]) * c[3] * c[4]),
    "mp_adamw_step": Entry(OPT_CAP, ("step_end.hip", "if (blocks > 256 * 16) blocks = 256 * 16;"), OPT_COUNTS, lambda c: c),
    "mp_adamw_step_scaled": Entry(OPT_CAP, ("step_end.hip", "if (blocks > 256 * 16) blocks = 256 * 16;"), OPT_COUNTS, lambda c: c),
    "mp_optimizer_step": Entry(OPT_CAP, ("step_end.hip", "if (blocks > 256 * 16) blocks = 256 * 16;"), OPT_COUNTS, lambda c: c),
    "mp_grad_finite_check": Entry(FINITE_CAP // 4, ("step_end.hip", "if (blocks > 256 * 8) blocks = 256 * 8;"), FINITE_COUNTS,
                                  lambda c: c // 4, lambda c: c, vec=4),
}


# ---- data -----------------------------------------------------------------------------------------------------------------------------

def seed_of(*key):
    """a generator seed from a case (stable across processes, unlike hash())"""
    flat = []

    def walk(v):
        if isinstance(v, (tuple, list)):
            for u in v:
                walk(u)
        else:
            flat.append(v)

    walk(key)
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(flat)) % (2 ** 31)


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def randn_h(g, *shape):
    """standard normal values that fp16 holds exactly, as fp32"""
    return torch.randn(*shape, generator=g).half().float()


def pattern_bits(numel, dtype):
    """`numel` finite values of every magnitude and both signs (zeros, denormals and -0 among them), cheap to make: the 32-bit words
    of a multiplicative hash with the lowest exponent bit of every element cleared (an exponent field of all ones - inf, NaN, the
    guard sentinel - never appears)."""
    per_word = 1 if dtype == torch.float32 else 2
    words = torch.arange(ceil_div(numel, per_word), dtype=torch.int32).mul_(-1640531527)
    words.bitwise_and_(~0x00800000 if dtype == torch.float32 else ~0x04000400)
    return words.view(dtype)[:numel]


def to_c8(x):
    """[n, c, h, w] -> channel-blocked fp16 [n, ceil(c / 8), h, w, 8] (channel 8 blk + j in lane j, padding lanes +0)"""
    n, c, h, w = x.shape
    c8 = c8_of(c)
    full = torch.zeros(n, c8 * 8, h, w, dtype=torch.float16)
    full[:, :c] = x.half()
    return full.view(n, c8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()


def from_c8(t, c):
    n, c8, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, c8 * 8, h, w)[:, :c].contiguous()


def plant_zeros(t, g):
    """`t` with exact +0 and -0 planted at a tenth of its positions each (what a ReLU output under a mask holds)"""
    flat = t.clone().reshape(-1)
    r = torch.rand(flat.numel(), generator=g)
    flat[r < 0.1] = 0.0
    flat[(r >= 0.1) & (r < 0.2)] = -0.0
    return flat.view(t.shape)


# ---- references -----------------------------------------------------------------------------------------------------------------------

def up(t, s):
    """nearest up-sampling by s of the last two axes"""
    return t if s == 1 else t.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)


def fuse_sum_ref(base, terms, scales, relu):
    """act(base + sum_k up_{s_k}(t_k)) in float64"""
    v = base.double()
    for t, s in zip(terms, scales):
        v = v + up(t.double(), s)
    return v.clamp_min(0) if relu else v


def fuse_sum_restated(base, terms, scales, relu, half=False):
    """the kernels' arithmetic: fp32 sums in the term order ((base + up(t1)) + up(t2)) + up(t3), the ReLU, and (half) ONE rounding to
    fp16.  torch CPU evaluates each step in IEEE fp32, so the kernels must give these bits."""
    v = base.float()
    for t, s in zip(terms, scales):
        v = v + up(t.float(), s)
    if relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    return v.half() if half else v


def block_sums(g, s):
    """s x s block sums over the last two axes"""
    if s == 1:
        return g
    *lead, h, w = g.shape
    return g.reshape(*lead, h // s, s, w // s, s).sum(dim=(-3, -1))


def fuse_sum_bwd_ref(dy, out, scales, relu):
    """float64: g = dy * (out > 0) under the ReLU, else dy; returns ([dbase, dt_1 ...], [sum |g| over the same blocks])"""
    g = dy.double()
    if relu:
        g = g * (out > 0)
    ss = (1,) + tuple(scales)
    return [block_sums(g, s) for s in ss], [block_sums(g.abs(), s) for s in ss]


def pool_geometry(h, w):
    oh, ow = ceil_div(h, 2), ceil_div(w, 2)
    ph, pw = max((oh - 1) * 2 + 3 - h, 0), max((ow - 1) * 2 + 3 - w, 0)
    return oh, ow, ph // 2, pw // 2


def _windows(h, w):
    """per output (oy, ox): the valid input positions of its 3 x 3 window in row-major scan order"""
    oh, ow, pt, pl = pool_geometry(h, w)
    for oy in range(oh):
        for ox in range(ow):
            yield oy, ox, [(y, x) for y in range(oy * 2 - pt, oy * 2 - pt + 3) if 0 <= y < h
                           for x in range(ox * 2 - pl, ox * 2 - pl + 3) if 0 <= x < w]


def maxpool_ref(x):
    """nn.MaxPool2d(3, 2, pad_mode="same") as plain loops over the windows (the planes are the vector axis); finite inputs"""
    n, c, h, w = x.shape
    oh, ow, _, _ = pool_geometry(h, w)
    out = torch.empty(n, c, oh, ow, dtype=x.dtype)
    for oy, ox, taps in _windows(h, w):
        m = x[:, :, taps[0][0], taps[0][1]].clone()
        for y, xx in taps[1:]:
            m = torch.maximum(m, x[:, :, y, xx])
        out[:, :, oy, ox] = m
    return out


def maxpool_bwd_ref(x, dy):
    """every window's gradient goes to its FIRST maximum in row-major scan order of its valid elements; an input element adds the
    windows that pick it in window order (oy, then ox, ascending), in dy's precision"""
    n, c, h, w = x.shape
    dx = torch.zeros(n * c, h * w, dtype=dy.dtype)
    xf, gf = x.reshape(n * c, h, w), dy.reshape(n * c, *dy.shape[2:])
    for oy, ox, taps in _windows(h, w):
        m = xf[:, taps[0][0], taps[0][1]].clone()
        at = torch.full((n * c,), taps[0][0] * w + taps[0][1], dtype=torch.int64)
        for y, xx in taps[1:]:
            v = xf[:, y, xx]
            better = v > m  # strictly: a tie keeps the earlier element
            m = torch.where(better, v, m)
            at = torch.where(better, torch.full_like(at, y * w + xx), at)
        dx.scatter_add_(1, at.view(-1, 1), gf[:, oy, ox].reshape(-1, 1))  # one index per row: no two adds meet in one call
    return dx.view(n, c, h, w)


def stem_wgrad_ref(x, dz, k):
    """float64 weight gradient of the k x k stride-2 padding-k/2 conv, and sum |dz * x| per weight"""
    import torch.nn.functional as F
    cout, cin = dz.shape[1], x.shape[1]

    def wgrad(xx, gg):
        wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx, wt, None, stride=2, padding=k // 2).backward(gg)
        return wt.grad

    return wgrad(x.double(), dz.double()), wgrad(x.double().abs(), dz.double().abs())


def gather_phase_ref(x, py, px, c8=False):
    """phase (py, px) of the last two spatial axes; c8: x is channel-blocked, [n, c8, 2h, 2w, 8]"""
    return (x[:, :, py::2, px::2, :] if c8 else x[..., py::2, px::2]).contiguous()


def _f32(v):
    return float(np.float32(v))


def _one_minus(v):
    """1 - v as the kernels form it: in fp32, on the fp32 value of the hyper-parameter"""
    return float(np.float32(1.0) - np.float32(v))


def optimizer_ref(kind, p, g, s1, s2, lr, grad_scale, wd, hyper):
    """The update rules of csrc/optim_update.h, which step_update_kernel of csrc/step_end.hip runs (kind 0: AdamWeightDecay, hyper =
    (b1, b2, eps); the gradient is g * grad_scale, decoupled decay; kinds 1 ... 4: the gradient is g * grad_scale + wd * p), in float64 on
    hyper-parameters first rounded to fp32.  Returns (p, s1, s2); states a rule does not have come back unchanged."""
    p, g = p.double(), g.double()
    s1 = None if s1 is None else s1.double()
    s2 = None if s2 is None else s2.double()
    lr, gs, wd = _f32(lr), _f32(grad_scale), _f32(wd)
    h = [_f32(v) for v in hyper]
    if kind == 0:
        gi = g * gs
        m = h[0] * s1 + _one_minus(h[0]) * gi
        v = h[1] * s2 + _one_minus(h[1]) * gi * gi
        return p - lr * (m / (v.sqrt() + h[2]) + wd * p), m, v
    gi = g * gs + wd * p
    if kind == 1:
        m = h[0] * s1 + _one_minus(h[0]) * gi
        v = h[1] * s2 + _one_minus(h[1]) * gi * gi
        lr_t = lr * _one_minus(h[4]) ** 0.5 / _one_minus(h[3])
        return p - lr_t * m / (v.sqrt() + h[2]), m, v
    if kind == 2:
        d = gi
        if h[0] != 0:
            s1 = gi.clone() if h[3] != 0 else h[0] * s1 + _one_minus(h[1]) * gi
            d = gi + h[0] * s1 if h[2] != 0 else s1
        return p - lr * d, s1, s2
    if kind == 3:
        s1 = h[0] * s1 + gi
        return p - lr * (gi + h[0] * s1 if h[1] != 0 else s1), s1, s2
    s1 = s1 + gi * gi
    return p - lr * gi / s1.sqrt(), s1, s2
