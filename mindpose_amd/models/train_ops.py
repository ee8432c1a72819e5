"""Training-mode building blocks: torch.autograd Functions whose forward AND backward are HIP kernels behind the
C ABI (conv forward / data-gradient on the direct MFMA conv, weight-gradient MFMA kernel, BatchNorm2d with batch
statistics, exchange-unit sum).  torch.autograd only records the graph and owns the tensors.

Reference semantics: the cells of mindpose/models/backbones/hrnet.py run by mindspore.Model.train
(tools/train.py:176-233); amp aside, everything here computes in fp32.
"""
import contextlib
import ctypes
import os
from typing import Optional

import numpy as np
import torch

from .. import _lib
from .layers import BN_EPS, conv_desc
from .tuner import F16_VARIANTS, F32_WINOGRAD, autotune_on, tune_conv_variant, winograd_enabled

BN_MOMENTUM = 0.9  # mindspore.nn.BatchNorm2d(momentum=0.9): moving = 0.9*moving + 0.1*batch [MS-knowledge]

_const_cache = {}


def _ones_zeros(c: int, device):
    key = (c, str(device))
    if key not in _const_cache:
        _const_cache[key] = (torch.ones(c, device=device), torch.zeros(c, device=device))
    return _const_cache[key]


def _desc(n, cin, h, w, cout, k, stride, pad_t, pad_l, conv_h, conv_w, out_h, out_w, out_mul=1, out_rep=1, off_y=0,
          off_x=0, flags=0):
    return conv_desc(n, cin, h, w, cout, k, stride, pad_t, pad_l, conv_h, conv_w, out_h, out_w, out_mul, out_rep, off_y, off_x,
                     flags=_lib.MP_CONV_SHARES_CUS | flags)


def _conv_launch(lib, d, x, packed, scale, shift, out, what, packed_u=None, res1=None):
    """One forward-kernel launch (forward conv or a data-gradient conv) with the autotuned tile variant; ``packed_u``: the
    Winograd form of the same weights (3x3 stride 1), which then competes in the tuner; ``res1``: added in the epilogue."""
    v = tune_conv_variant(lib, d, x, packed, scale, shift, res1, None, out, packed_u=packed_u)
    if v == F32_WINOGRAD and packed_u is not None:
        _lib.check(lib.mp_conv2d_winograd_fwd(ctypes.byref(d), _lib.ptr(x), _lib.ptr(packed_u), _lib.ptr(scale), _lib.ptr(shift),
                                              _lib.ptr(res1), None, _lib.ptr(out), _lib.stream()), what)
        return
    _lib.check(lib.mp_conv2d_fwd_variant(ctypes.byref(d), v, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(shift),
                                         _lib.ptr(res1), None, _lib.ptr(out), _lib.stream()), what)


def _pack_winograd(lib, d, w, cout, cin, mode, owner):
    """Winograd form of a 3x3 weight (mode 5: forward, 6: data gradient) when the descriptor is inside that form, else None."""
    if not winograd_enabled() or not autotune_on() or lib.mp_conv_winograd_supported(ctypes.byref(d)) != 0:
        return None
    return _cached_pack(lib, w, owner, False, cout, cin, 3, mode, 0, 0)


def _pack(lib, w, cout, cin, k, mode, py=0, px=0, owner=None):
    return _cached_pack(lib, w, owner, False, cout, cin, k, mode, py, px)


# ---- amp O2: the same graph on channel-blocked fp16 activations ([N, ceil(C/8), H, W, 8] half tensors) -------------------
# fp16 conv operands / activations / activation gradients, fp32 accumulation, BatchNorm statistics and every PARAMETER
# gradient in fp32 (the parameters themselves stay fp32 "master" weights: the pack kernel rounds them to fp16 per step).


def _direct_grad(param):
    """The parameter's slot in a flat gradient arena when the owner allows kernels to accumulate into it directly
    (``GradientAverager`` without overlap hooks sets ``_mp_grad_direct``): saves one AccumulateGrad add launch per parameter
    (878 per HRNet-W32 step, 8 % of the graphed O2 step)."""
    if getattr(param, "_mp_grad_direct", False) and param.grad is not None and param.grad.is_contiguous():
        return param.grad
    return None


def _c8_shape(n, c, h, w):
    return (n, (c + 7) // 8, h, w, 8)


def _c8_alloc(n, c, h, w, device):
    """Uninitialised when every channel block is full; zero-filled when the last block has padding channels (the kernels
    keep them zero, but a fresh buffer must start that way)."""
    make = torch.empty if c % 8 == 0 else torch.zeros
    return make(_c8_shape(n, c, h, w), device=device, dtype=torch.float16)


_BN16_WS = {}


def _bn16_workspace(lib, c, device):
    """ONE persistent BatchNorm workspace per (device, stream): no allocation per layer."""
    need = lib.mp_bn_workspace_bytes(c)
    key = (device, torch.cuda.current_stream(device).cuda_stream)  # calls on one stream are ordered; streams do not share
    ws = _BN16_WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = torch.zeros(max(need, lib.mp_bn_workspace_bytes(2048)) // 4 + 1, device=device, dtype=torch.float32)
        _BN16_WS[key] = ws
    return ws, ws.numel() * 4


# ---- fp16 weight packings ------------------------------------------------------------------------------------------------
# The fp32 master weights change every step, so every step re-packs them (forward form + data-gradient forms: 700 packings
# per HRNet-W32 step).  Each parameter remembers its packed buffers (``param._mp_packs``); ``repack_weights(net)`` - called
# by ``Net.train_forward`` - refreshes ALL of them with ONE launch (mp_f16_pack_weight_batch) and the per-layer code then
# finds its packing fresh.  A packing is used once per refresh; anything else (first step, direct calls of the functions,
# a weight changed since the refresh) packs individually, as before.
_PACK_GEN = [0]


def invalidate_packs():
    """Master weights were written behind torch's back (optimizer kernels update through raw pointers): nothing packed
    before this call may be reused."""
    _PACK_GEN[0] += 1


class _PackEntry:
    __slots__ = ("buf", "fresh", "gen", "ptr", "version")

    def __init__(self, buf):
        self.buf, self.fresh, self.gen, self.ptr, self.version = buf, False, -1, 0, -1


class _PackJob(ctypes.Structure):  # mp_f16_pack_job
    _fields_ = [("w", ctypes.c_void_p), ("packed", ctypes.c_void_p)] + [(k, ctypes.c_int) for k in
                ("cout", "cin", "kh", "kw", "transposed", "phase_y", "phase_x", "reserved")]


def _cached_pack(lib, w, owner, half, cout, cin, k, mode, py, px):
    """Packed form of ``w`` (fp16 or fp32 kernels); with ``owner`` (the Parameter ``w`` was detached from) the buffer is
    persistent and a packing refreshed by ``repack_weights`` is handed out without a launch."""
    if half:
        numel, dtype = lib.mp_f16_packed_weight_bytes(cout, cin, k, k) // 2, torch.float16
    elif mode in (5, 6):  # Winograd forms of a 3x3 weight
        numel, dtype = lib.mp_conv_winograd_packed_weight_bytes(cout, cin) // 4, torch.float32
    else:
        numel, dtype = lib.mp_conv_packed_weight_bytes(cout, cin, k, k) // 4, torch.float32
    entry = None
    if owner is not None:
        packs = owner.__dict__.setdefault("_mp_packs", {})
        key = (half, cout, cin, k, mode, py, px)
        entry = packs.get(key)
        if entry is None:
            if half and mode == 3:
                # the four sub-pixel phase packings of one weight are slices (2 py + px) of ONE buffer: MP_CONV_PHASES4 launches
                # take the whole of it, per-phase launches their slice
                parents = owner.__dict__.setdefault("_mp_pack_parents", {})
                parent = parents.get(key[:5])
                if parent is None:
                    parent = parents[key[:5]] = torch.empty(4 * numel, device=w.device, dtype=dtype)
                entry = packs[key] = _PackEntry(parent[(2 * py + px) * numel:(2 * py + px + 1) * numel])
            else:
                entry = packs[key] = _PackEntry(torch.empty(numel, device=w.device, dtype=dtype))
        if (entry.fresh and entry.gen == _PACK_GEN[0] and entry.ptr == w.data_ptr() and entry.version == owner._version):
            entry.fresh = False
            return entry.buf
        entry.fresh = False
    packed = entry.buf if entry is not None else torch.empty(numel, device=w.device, dtype=dtype)
    fn = lib.mp_f16_pack_weight if half else lib.mp_conv_pack_weight
    _lib.check(fn(_lib.ptr(w), _lib.ptr(packed), cout, cin, k, k, mode, py, px, _lib.stream()), "pack_weight")
    return packed


def _pack16(lib, w, cout, cin, k, mode, py=0, px=0, owner=None):
    return _cached_pack(lib, w, owner, True, cout, cin, k, mode, py, px)


def phases4_enabled() -> bool:
    """``MINDPOSE_DGRAD_PHASES4=0``: the stride-2 3x3 data gradient as four phase launches (A/B; bit-identical: the
    four launches take the one launch's variant and leave the same BatchNorm backward sums in the same slots)."""
    return _lib.env_on("MINDPOSE_DGRAD_PHASES4")


def _dgrad16_stride2(lib, w, owner, dz, dx, n, cin, cout, h, wd, ho, wo, ones, zeros, below=None):
    """Data gradient of a 3x3 stride-2 padding-1 conv: four 2x2 sub-pixel phase convs over dz, each writing every second pixel
    of dx - as ONE launch (MP_CONV_PHASES4; phase = second grid dimension) when the weight has an owner whose four packings share
    a buffer, else as four launches.  ``below`` = (z, y, relu) of the BatchNorm whose output this conv read: the launch(es) then
    also mask the gradient and leave that BatchNorm's backward sums (returns (partials, n_parts), else (None, 0)) - the four
    launches of MINDPOSE_DGRAD_PHASES4=0 in the slots, and so the order, of the one launch."""
    if owner is not None and phases4_enabled():
        for py in (0, 1):
            for px in (0, 1):
                _pack16(lib, w, cin, cout, 2, 3, py, px, owner=owner)  # fresh slices (no launch after repack_weights)
        parent = owner.__dict__["_mp_pack_parents"][(True, cin, cout, 2, 3)]
        d = _desc(n, cout, ho, wo, cin, 2, 1, 0, 0, ho, wo, h, wd, out_mul=2, flags=_lib.MP_CONV_PHASES4)
        if below is not None:
            return _conv16_stats_launch(lib, d, dz, parent, ones, zeros, dx, None, 2, z=below[0], y=below[1], relu=below[2])
        _conv16_launch(lib, d, dz, parent, ones, zeros, dx, "conv dgrad phases")
        return None, 0
    slices = {(py, px): _pack16(lib, w, cin, cout, 2, 3, py, px, owner=owner) for py in (0, 1) for px in (0, 1)}
    part, n_parts = None, 0
    if owner is not None and below is not None:
        # four launches that leave what the one launch leaves: each phase runs the variant the merged launch takes and fills its
        # quarter of that launch's partial sums (same tiles, same slots) - the switch changes the launch count, not the arithmetic
        parent = owner.__dict__["_mp_pack_parents"][(True, cin, cout, 2, 3)]
        dm = _desc(n, cout, ho, wo, cin, 2, 1, 0, 0, ho, wo, h, wd, out_mul=2, flags=_lib.MP_CONV_PHASES4)
        stats = dict(mode=2, z=below[0], y=below[1], relu=below[2])
        v = tune_conv_variant(lib, dm, dz, parent, ones, zeros, None, None, dx, half=True, stats=stats)
        part, n_parts = _stats_alloc(lib, dm, v, (cin + 7) // 8, dx.device)
    for (py, px), packed in slices.items():
        d = _desc(n, cout, ho, wo, cin, 2, 1, 0, 0, ho, wo, h, wd, out_mul=2, off_y=py, off_x=px)
        if part is not None:
            _conv16_stats_launch(lib, d, dz, packed, ones, zeros, dx, None, 2, z=below[0], y=below[1], relu=below[2], into=(v, part))
        else:
            _conv16_launch(lib, d, dz, packed, ones, zeros, dx, "conv dgrad phase")
    return part, n_parts


def repack_weights(module):
    """Refresh every remembered packing of ``module``'s parameters: one launch for the fp16 forms, one for the fp32 forms
    (no-op until a first step has run)."""
    jobs = {True: [], False: []}
    for prm in module.parameters():
        packs = prm.__dict__.get("_mp_packs")
        if packs and prm.is_cuda and prm.dtype == torch.float32 and prm.is_contiguous():
            for key, entry in packs.items():
                jobs[key[0]].append((prm, key, entry))
    total = 0
    for half, group in jobs.items():
        if not group:
            continue
        lib = _lib.load()
        sig = tuple((prm.data_ptr(), entry.buf.data_ptr()) for prm, _, entry in group)
        tables = module.__dict__.setdefault("_mp_pack_tables", {})
        table = tables.get(half)
        if table is None or table[0] != sig:
            arr = (_PackJob * len(group))()
            first = np.zeros(len(group) + 1, dtype=np.uint32)
            for i, (prm, (_, cout, cin, k, mode, py, px), entry) in enumerate(group):
                arr[i] = _PackJob(prm.data_ptr(), entry.buf.data_ptr(), cout, cin, k, k, mode, py, px, 0)
                cp = (cout + 15) // 16 * 16
                # fp16: one thread per (group of 8 input channels, cout) pair - it walks the taps itself
                units = (cin + 31) // 32 * 4 * cp if half else (cin + 3) // 4 * 4 * k * k * (cp // 4)
                if not half and mode in (5, 6):  # Winograd forms: one thread per (cin, cout) pair
                    units = (cin + 3) // 4 * 4 * cp
                first[i + 1] = first[i] + (units + 255) // 256
            dev = group[0][0].device
            jobs_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            first_dev = torch.from_numpy(first.view(np.int32)).to(dev)
            table = tables[half] = (sig, jobs_dev, first_dev, int(first[-1]))
        _, jobs_dev, first_dev, blocks = table
        fn = lib.mp_f16_pack_weight_batch if half else lib.mp_conv_pack_weight_batch
        _lib.check(fn(_lib.ptr(jobs_dev), _lib.ptr(first_dev), len(group), blocks, _lib.stream()), "pack_weight_batch")
        gen = _PACK_GEN[0]
        for prm, _, entry in group:
            entry.fresh, entry.gen, entry.ptr, entry.version = True, gen, prm.data_ptr(), prm._version
        total += len(group)
    return total


def _ones_zeros16(c: int, device):
    return _ones_zeros((c + 15) // 16 * 16, device)


def _conv16_run(lib, d, v, x, packed, scale, shift, res1, out, what):
    """The plain fp16 conv launch with variant ``v`` (`_conv16_launch`, and `_conv16_stats_launch` when ``v`` has no statistics build)."""
    _lib.check(lib.mp_f16_conv2d_fwd(ctypes.byref(d), v, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(res1),
                                     None, _lib.ptr(out), _lib.stream()), what)


def _conv16_launch(lib, d, x, packed, scale, shift, out, what, res1=None):
    v = tune_conv_variant(lib, d, x, packed, scale, shift, res1, None, out, half=True)  # one-tile / multi-tile, cached per shape
    _conv16_run(lib, d, v, x, packed, scale, shift, res1, out, what)


# ---- one body per cell for both activation types -----------------------------------------------------------------------------------
# What differs between fp32 NCHW and channel-blocked fp16 is DATA (`_Precision`: how to allocate an activation, its constant
# epilogue vectors, its pack function and BatchNorm workspace policy); every cell body below is written once against it, and the
# autograd Functions further down are two-line shells that name their record.  Where the two types launch differently on purpose
# (another entry point of the library, another route) the bodies branch on ``P.half``, in place.  The launch helpers the tests patch (`_conv16_launch`, `_conv16_stats_launch`,
# `_wgrad_flush_key`, ...) are never bound into a record: the bodies look them up in the module when they run.


def _bn32_workspace(lib, c, device):
    """The fp32 BatchNorm's workspace: one allocation per call."""
    ws_bytes = lib.mp_bn_workspace_bytes(c)
    return torch.empty(ws_bytes // 4 + 1, device=device, dtype=torch.float32), ws_bytes


class _Precision:
    """One activation type: ``alloc(n, c, h, w, device)``, ``ones_zeros(c, device)`` (the constant epilogue vectors),
    ``pack(lib, w, cout, cin, k, mode, py, px, owner=)``, ``bn_workspace(lib, c, device)`` -> (tensor, bytes)."""
    __slots__ = ("half", "alloc", "ones_zeros", "pack", "bn_workspace")

    def __init__(self, half, alloc, ones_zeros, pack, bn_workspace):
        self.half, self.alloc, self.ones_zeros, self.pack, self.bn_workspace = half, alloc, ones_zeros, pack, bn_workspace


_F32 = _Precision(False, lambda n, c, h, w, device: torch.empty(n, c, h, w, device=device, dtype=torch.float32), _ones_zeros, _pack,
                  _bn32_workspace)
_F16 = _Precision(True, _c8_alloc, _ones_zeros16, _pack16, _bn16_workspace)


def _nhw(t):
    """(N, H, W) of an activation of either type: [N, C, H, W] or [N, C/8, H, W, 8]."""
    return t.shape[0], t.shape[2], t.shape[3]


def _conv_fwd_args(P, lib, x, weight, w, bias, stride, padding):
    """Geometry check, epilogue vectors, output, descriptor and packed weight of a forward conv:
    (d, packed, ones, shift, z, (n, cout, ho, wo))."""
    n, h, wd = _nhw(x)
    cout, cin, k, _ = w.shape
    if padding != k // 2 or k not in (1, 3) or stride not in (1, 2):
        raise NotImplementedError("training path covers k in {1,3}, stride in {1,2}, padding = k//2")
    ho, wo = (h + 2 * padding - k) // stride + 1, (wd + 2 * padding - k) // stride + 1
    ones, shift = P.ones_zeros(cout, x.device)
    if bias is not None and P.half:  # the fp16 epilogue reads whole 16-channel groups: a padded copy
        shift = torch.zeros_like(shift)
        shift[:cout] = bias.detach()
    elif bias is not None:
        shift = bias.detach().contiguous()
    z = P.alloc(n, cout, ho, wo, x.device)
    d = _desc(n, cin, h, wd, cout, k, stride, padding, padding, ho, wo, ho, wo)
    return d, P.pack(lib, w, cout, cin, k, 0, owner=weight), ones, shift, z, (n, cout, ho, wo)


def _conv_forward(P, ctx, x, weight, bias, stride, padding):
    lib = _lib.load()
    if not P.half:
        x = _lib.require_cuda_f32(x, "x")
    w = weight.detach().contiguous()
    d, packed, ones, shift, z, _ = _conv_fwd_args(P, lib, x, weight, w, bias, stride, padding)
    if P.half:
        _conv16_launch(lib, d, x, packed, ones, shift, z, "mp_f16_conv2d_fwd")
    else:  # the Winograd form of a 3x3 weight competes in the fp32 tuner
        _conv_launch(lib, d, x, packed, ones, shift, z, "mp_conv2d_fwd", packed_u=_pack_winograd(lib, d, w, d.cout, d.cin, 5, weight))
    ctx.save_for_backward(x, w)
    ctx.stride, ctx.padding, ctx.has_bias = stride, padding, bias is not None
    ctx.weight_param = weight
    return z


def _conv_dgrad(P, lib, x, w, owner, dz, s, pad, res1=None, below=None):
    """Data gradient of the conv that read ``x``; ``res1`` is added in the launch's epilogue.  ``below`` (fused chains) = (z, y, relu)
    of the BatchNorm whose output ``x`` is: the launch also masks the gradient and leaves that BatchNorm's backward sums.
    Returns (dx, partials, n_parts); partials None when nothing was reduced."""
    n, h, wd = _nhw(x)
    cout, cin, k, _ = w.shape
    ho, wo = dz.shape[2], dz.shape[3]
    ones, zeros = P.ones_zeros(cin, x.device)
    if s != 1 and (h != 2 * ho or wd != 2 * wo):
        raise NotImplementedError("stride-2 data gradient needs even input extents")
    if s != 1 and res1 is not None:
        raise NotImplementedError("a residual chain starts with a stride-1 conv")
    if s != 1 and k == 1 and not P.half:  # 1x1 stride 2 (ResNet down-sample): only the even positions receive gradient
        dx = torch.zeros_like(x)
    else:
        dx = P.alloc(n, cin, h, wd, x.device)
    if below is not None and tuple(below[0].shape) != tuple(dx.shape):
        below = None
    part, n_parts = None, 0
    if s == 1:
        d = _desc(n, cout, ho, wo, cin, k, 1, k - 1 - pad, k - 1 - pad, h, wd, h, wd)
        packed = P.pack(lib, w, cin, cout, k, 2, owner=owner)
        if below is not None:
            part, n_parts = _conv16_stats_launch(lib, d, dz, packed, ones, zeros, dx, res1, 2, z=below[0], y=below[1], relu=below[2])
        elif P.half:
            _conv16_launch(lib, d, dz, packed, ones, zeros, dx, "conv dgrad", res1=res1)
        else:
            _conv_launch(lib, d, dz, packed, ones, zeros, dx, "conv dgrad", res1=res1,
                         packed_u=_pack_winograd(lib, d, w, cin, cout, 6, owner) if k == 3 else None)
    elif k == 1:
        if P.half:
            dx.zero_()
        d = _desc(n, cout, ho, wo, cin, 1, 1, 0, 0, ho, wo, h, wd, out_mul=2)
        packed = P.pack(lib, w, cin, cout, 1, 2, owner=owner)
        (_conv16_launch if P.half else _conv_launch)(lib, d, dz, packed, ones, zeros, dx, "conv dgrad 1x1s2")
    elif P.half:  # 3x3 stride 2: one merged launch of the four sub-pixel phases (or four, MINDPOSE_DGRAD_PHASES4=0)
        part, n_parts = _dgrad16_stride2(lib, w, owner, dz, dx, n, cin, cout, h, wd, ho, wo, ones, zeros, below=below)
    else:  # ... in fp32: four launches
        for py in (0, 1):
            for px in (0, 1):
                d = _desc(n, cout, ho, wo, cin, 2, 1, 0, 0, ho, wo, h, wd, out_mul=2, off_y=py, off_x=px)
                packed = _pack(lib, w, cin, cout, 2, 3, py, px, owner=owner)
                _conv_launch(lib, d, dz, packed, ones, zeros, dx, "conv dgrad phase")
    return dx, part, n_parts


def _wgrad_launch(P, lib, d, x, dz, dw, acc, what, must=False):
    """THE weight-gradient launch: dW (+)= x (*) dz with its workspace; ``must``: a shape without a kernel is an error here
    (the transposed conv's 4x4 stride-2 form) instead of the library's."""
    ws_bytes = (lib.mp_f16_conv_wgrad_workspace_bytes if P.half else lib.mp_conv_wgrad_workspace_bytes)(ctypes.byref(d))
    if must and ws_bytes == 0:
        raise _lib.MindposeHipError("transposed-conv weight gradient: unsupported shape")
    ws = torch.empty(max(ws_bytes // 4, 1), device=x.device, dtype=torch.float32)
    if P.half:
        rc = lib.mp_f16_conv_wgrad(ctypes.byref(d), _lib.ptr(x), _lib.ptr(dz), _lib.ptr(dw), 1.0, acc, _lib.ptr(ws), ws_bytes, _lib.stream())
    else:
        rc = lib.mp_conv_wgrad(ctypes.byref(d), _lib.ptr(x), _lib.ptr(dz), _lib.ptr(dw), acc, _lib.ptr(ws), ws_bytes, _lib.stream())
    _lib.check(rc, what)


def _wgrad(P, lib, d, x, dz, w, owner, what, queue=False, must=False):
    """Launch or queue one weight gradient.  With an ``owner`` that allows it the gradient is ADDED into the owner's slot of the
    gradient arena (no AccumulateGrad launch) - ``queue``: later, grouped with the other layers of this shape - and None is
    returned; else a fresh tensor."""
    direct = _direct_grad(owner) if owner is not None else None
    if direct is not None and queue:
        _wgrad_enqueue(lib, d, x, dz, direct)
        return None
    dw = direct if direct is not None else torch.empty_like(w)
    _wgrad_launch(P, lib, d, x, dz, dw, int(direct is not None), what, must)
    return None if direct is not None else dw


def _conv_backward(P, ctx, dz):
    lib = _lib.load()
    x, w = ctx.saved_tensors
    dz = dz.contiguous()
    n, h, wd = _nhw(x)
    cout, cin, k, _ = w.shape
    s, pad = ctx.stride, ctx.padding
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
        # ResidualBlock*Fn: the gradient that reaches x through the identity is added in the launch's epilogue
        dx, _, _ = _conv_dgrad(P, lib, x, w, ctx.weight_param, dz, s, pad, res1=getattr(ctx, "dx_residual", None))
    if ctx.needs_input_grad[1]:
        d = _desc(n, cin, h, wd, cout, k, s, pad, pad, dz.shape[2], dz.shape[3], dz.shape[2], dz.shape[3])
        dw = _wgrad(P, lib, d, x, dz, w, ctx.weight_param, "mp_f16_conv_wgrad" if P.half else "mp_conv_wgrad")
    if ctx.has_bias and ctx.needs_input_grad[2]:  # the head conv's bias (17 values)
        db = dz.float().sum(dim=(0, 2, 3)).reshape(-1)[:cout] if P.half else dz.sum(dim=(0, 2, 3))
    return dx, dw, db, None, None


def _bn_fwd_job(P, lib, z, gamma, beta, res, moving_mean, moving_var, relu):
    """Outputs, saved statistics and workspace of one BatchNorm forward, as the job dict the launchers take."""
    n, h, w = _nhw(z)
    c = gamma.numel()
    ws, ws_bytes = P.bn_workspace(lib, c, z.device)
    return dict(z=z, g=gamma.detach().contiguous(), b=beta.detach().contiguous(), res=res.contiguous() if res is not None else None,
                y=torch.empty_like(z), mean=torch.empty(c, device=z.device), invstd=torch.empty(c, device=z.device), mm=moving_mean,
                mv=moving_var, n=n, c=c, hw=h * w, relu=int(relu), part=None, n_parts=0, ws=ws, ws_bytes=ws_bytes)


def _bn_fwd_launch(P, lib, j):
    """Reduce + apply, moving statistics updated in place."""
    args = (_lib.ptr(j["z"]), _lib.ptr(j["g"]), _lib.ptr(j["b"]), _lib.ptr(j["res"]), _lib.ptr(j["y"]), _lib.ptr(j["mean"]),
            _lib.ptr(j["invstd"]), _lib.ptr(j["mm"]), _lib.ptr(j["mv"]), j["n"], j["c"], j["hw"], BN_EPS, BN_MOMENTUM, j["relu"],
            _lib.ptr(j["ws"]), j["ws_bytes"], _lib.stream())
    if P.half:
        _lib.check(lib.mp_f16_bn_train_fwd(*args), "mp_f16_bn_train_fwd")
    else:
        _lib.check(lib.mp_bn_train_fwd(*args), "mp_bn_train_fwd")


def _bn_forward(P, ctx, z, gamma, beta, res, moving_mean, moving_var, relu):
    lib = _lib.load()
    if not P.half:
        z = _lib.require_cuda_f32(z, "z")
    j = _bn_fwd_job(P, lib, z, gamma, beta, res, moving_mean, moving_var, relu)
    _bn_fwd_launch(P, lib, j)
    ctx.save_for_backward(z, j["y"], j["g"], j["b"], j["mean"], j["invstd"])
    ctx.relu, ctx.has_res = relu, res is not None
    ctx.gamma_param, ctx.beta_param = gamma, beta
    return j["y"]


def _bn_bwd_job(P, lib, dy, z, g, b, mean, invstd, gamma, beta, relu):
    """Outputs and workspace of one BatchNorm backward; ``ga`` / ``ba``: the gradient-arena slots of gamma and beta when BOTH
    take direct accumulation (then the kernel adds into them), else None.  The caller fills ``yy`` (the mask source), ``dr`` (the
    residual's gradient) and ``pre`` (sums that came with a pre-masked ``dy``)."""
    n, h, w = _nhw(z)
    c = g.numel()
    ws, ws_bytes = P.bn_workspace(lib, c, z.device)
    ga, ba = _direct_grad(gamma), _direct_grad(beta)
    if ga is None or ba is None:
        ga = ba = None
    return dict(dy=dy, z=z, g=g, b=b, mean=mean, invstd=invstd, dz=torch.empty_like(z), dgamma=torch.empty(c, device=z.device),
                dbeta=torch.empty(c, device=z.device), ga=ga, ba=ba, n=n, c=c, hw=h * w, relu=int(relu), ws=ws, ws_bytes=ws_bytes,
                pre=None, yy=None, dr=None)


def _bn_bwd_launch(P, lib, j):
    """Reduce + apply.  The fp16 kernel re-derives the ReLU mask from z and beta when ``yy`` is None; the fp32 one takes no beta."""
    head = (_lib.ptr(j["dy"]), _lib.ptr(j["z"]), _lib.ptr(j["yy"]), _lib.ptr(j["g"]))
    tail = (_lib.ptr(j["mean"]), _lib.ptr(j["invstd"]), _lib.ptr(j["dz"]), _lib.ptr(j["dr"]), _lib.ptr(j["dgamma"]), _lib.ptr(j["dbeta"]),
            _lib.ptr(j["ga"]), _lib.ptr(j["ba"]), j["n"], j["c"], j["hw"], j["relu"], _lib.ptr(j["ws"]), j["ws_bytes"], _lib.stream())
    if P.half:
        _lib.check(lib.mp_f16_bn_train_bwd(*head, _lib.ptr(j["b"]), *tail), "mp_f16_bn_train_bwd")
    else:
        _lib.check(lib.mp_bn_train_bwd_acc(*head, *tail), "mp_bn_train_bwd")


def _bn_backward(P, ctx, dy):
    lib = _lib.load()
    z, y, g, b, mean, invstd = ctx.saved_tensors
    j = _bn_bwd_job(P, lib, dy.contiguous(), z, g, b, mean, invstd, ctx.gamma_param, ctx.beta_param, ctx.relu)
    # fp16 without a residual: the ReLU mask is re-derived from z (forward arithmetic), y is not read
    j["yy"] = None if (P.half and ctx.relu and not ctx.has_res and _lib.env_on("MINDPOSE_BN16_MASK_FROM_Z")) else y
    j["dr"] = torch.empty_like(z) if ctx.has_res else None
    _bn_bwd_launch(P, lib, j)
    if j["ga"] is not None:
        return j["dz"], None, None, j["dr"], None, None, None
    return j["dz"], j["dgamma"], j["dbeta"], j["dr"], None, None, None


def _scaled_ptrs(ts, scales):
    """The three (pointer, integer scale) operand slots of the exchange-unit kernels; a slot without a term is (NULL, 1)."""
    args = []
    for i in range(3):
        args += [_lib.ptr(ts[i]), int(scales[i])] if i < len(ts) else [None, 1]
    return args


def _fuse_sum_forward(P, ctx, base, scales, terms):
    lib = _lib.load()
    n, h, w = _nhw(base)
    c = base.shape[1] * (8 if P.half else 1)
    base = base.contiguous()
    ts = [t.contiguous() for t in terms]
    out = torch.empty_like(base)
    args = (_lib.ptr(base), *_scaled_ptrs(ts, scales), _lib.ptr(out), n, c, h, w, 1, _lib.stream())
    if P.half:
        _lib.check(lib.mp_f16_fuse_upsample_sum(*args), "mp_f16_fuse_upsample_sum")
    else:
        _lib.check(lib.mp_fuse_upsample_sum(*args), "mp_fuse_upsample_sum")
    ctx.save_for_backward(out)
    ctx.scales = [int(s) for s in scales[:len(ts)]]
    return out


def _fuse_sum_backward(P, ctx, dy):
    """(dbase, dts).  ``ctx.links`` (`FuseSum16Fn`): an operand whose link allows it gets its gradient from a launch of its own
    that also masks and reduces it for the BatchNorm that produced the operand; the plain kernel writes the rest."""
    lib = _lib.load()
    (out,) = ctx.saved_tensors
    dy = dy.contiguous()
    n, h, w = _nhw(out)
    c = out.shape[1] * (8 if P.half else 1)
    dbase = torch.empty_like(out)
    dts = [P.alloc(n, c, h // s, w // s, out.device) for s in ctx.scales]
    plain = [dbase] + dts
    for k, link in enumerate(getattr(ctx, "links", ())):
        dst, sc = plain[k], ([1] + ctx.scales)[k]
        if (link is not None and link.claimed == 1 and (_bn_fuse_parts() & 8) and tuple(link.z.shape) == tuple(dst.shape)):
            n_parts = lib.mp_f16_fuse_term_stats_parts(n, c, h, w, sc)
            part = torch.empty(c // 8 * n_parts * 16, device=out.device, dtype=torch.float32)
            _lib.check(lib.mp_f16_fuse_sum_bwd_term_stats(_lib.ptr(dy), _lib.ptr(out), _lib.ptr(dst), sc, n, c, h, w, 1,
                                                          _lib.ptr(link.z), _lib.ptr(link.y) if link.relu else None, int(link.relu),
                                                          _lib.ptr(part), part.numel() * 4, _lib.stream()),
                       "mp_f16_fuse_sum_bwd_term_stats")
            link.hand_over(part, n_parts, dst)
            plain[k] = None
    if any(p is not None for p in plain):
        fn = lib.mp_f16_fuse_upsample_sum_bwd if P.half else lib.mp_fuse_upsample_sum_bwd
        _lib.check(fn(_lib.ptr(dy), _lib.ptr(out), _lib.ptr(plain[0]), *_scaled_ptrs(plain[1:], ctx.scales), n, c, h, w, 1, _lib.stream()),
                   "mp_fuse_upsample_sum_bwd")
    return dbase, dts


def _deconv_forward(P, ctx, x, weight):
    lib = _lib.load()
    if not P.half:
        x = _lib.require_cuda_f32(x, "x")
    w = weight.detach().contiguous()
    n, h, wd = _nhw(x)
    cin, cout = w.shape[0], w.shape[1]
    # the fp32 form packs without an owner and keeps out of the gradient arena: `_deconv_backward` finds no owner either
    ctx.weight_param = weight if P.half else None
    ones, zeros = P.ones_zeros(cout, x.device)
    y = P.alloc(n, cout, 2 * h, 2 * wd, x.device)
    for py in (0, 1):
        for px in (0, 1):
            d = _desc(n, cin, h, wd, cout, 2, 1, 1 - py, 1 - px, h, wd, 2 * h, 2 * wd, out_mul=2, off_y=py, off_x=px)
            packed = P.pack(lib, w, cout, cin, 2, 1, py, px, owner=ctx.weight_param)
            (_conv16_launch if P.half else _conv_launch)(lib, d, x, packed, ones, zeros, y, "deconv phase")
    ctx.save_for_backward(x, w)
    return y


def _deconv_backward(P, ctx, dy):
    lib = _lib.load()
    x, w = ctx.saved_tensors
    dy = dy.contiguous()
    n, h, wd = _nhw(x)
    cin, cout = w.shape[0], w.shape[1]
    dx = dw = None
    if ctx.needs_input_grad[0]:
        ones, zeros = P.ones_zeros(cin, x.device)
        dx = P.alloc(n, cin, h, wd, x.device)
        phase = P.alloc(n, cout, h, wd, x.device)
        gather = lib.mp_f16_gather_phase if P.half else lib.mp_gather_phase
        for py in (0, 1):
            for px in (0, 1):
                _lib.check(gather(_lib.ptr(dy), _lib.ptr(phase), n, cout, h, wd, py, px, _lib.stream()), "mp_gather_phase")
                # y_phase[m] = sum_t x[m - (1-p) + t] wp[t]  =>  dx[j] = sum_t dy_phase[j + (1-p) - t] wp[t]:
                # a 2x2 conv over dy_phase with mirrored taps and padding p; the phases add up through the epilogue
                d = _desc(n, cout, h, wd, cin, 2, 1, py, px, h, wd, h, wd)
                packed = P.pack(lib, w, cin, cout, 2, 4, py, px, owner=ctx.weight_param)
                res1 = dx if (py or px) else None
                if P.half:
                    _conv16_launch(lib, d, phase, packed, ones, zeros, dx, "deconv dgrad phase", res1=res1)
                else:  # the untuned launch
                    _lib.check(lib.mp_conv2d_fwd(ctypes.byref(d), _lib.ptr(phase), _lib.ptr(packed), _lib.ptr(ones), _lib.ptr(zeros),
                                                 _lib.ptr(res1), None, _lib.ptr(dx), _lib.stream()), "deconv dgrad phase")
    if ctx.needs_input_grad[1]:
        # dW[ci][co][ky][kx] = sum_m x[m][ci] * dy[2m + ky - 1][co]: weight gradient of a 4x4 s2 p1 conv whose input is dy
        # and whose output gradient is x -> result laid out [ci][co][4][4] = the transposed conv's own weight layout
        d = _desc(n, cout, 2 * h, 2 * wd, cin, 4, 2, 1, 1, h, wd, h, wd)
        dw = _wgrad(P, lib, d, dy, x, w, ctx.weight_param, "deconv wgrad", must=True)
    return dx, dw


class ToC8Fn(torch.autograd.Function):
    """fp32 NCHW -> channel-blocked fp16 (the network input, or the output of ResNet's fp32 stem: then the gradient flows back
    as fp32 NCHW)."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _lib.require_cuda_f32(x, "x")
        n, c, h, w = x.shape
        out = _c8_alloc(n, c, h, w, x.device)
        _lib.check(lib.mp_f16_to_c8(_lib.ptr(x), _lib.ptr(out), n, c, h, w, _lib.stream()), "mp_f16_to_c8")
        ctx.c = c
        return out

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None
        lib = _lib.load()
        dy = dy.contiguous()
        n, _, h, w, _ = dy.shape
        dx = torch.empty(n, ctx.c, h, w, device=dy.device, dtype=torch.float32)
        _lib.check(lib.mp_f16_from_c8(_lib.ptr(dy), _lib.ptr(dx), n, ctx.c, h, w, _lib.stream()), "mp_f16_from_c8")
        return dx


class FromC8Fn(torch.autograd.Function):
    """channel-blocked fp16 -> fp32 NCHW (network output handed to the fp32 loss); backward rounds the loss gradient to fp16."""

    @staticmethod
    def forward(ctx, x, c):
        lib = _lib.load()
        n, _, h, w, _ = x.shape
        out = torch.empty(n, c, h, w, device=x.device, dtype=torch.float32)
        _lib.check(lib.mp_f16_from_c8(_lib.ptr(x), _lib.ptr(out), n, c, h, w, _lib.stream()), "mp_f16_from_c8")
        ctx.c = c
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        dy = dy.contiguous()
        n, c, h, w = dy.shape
        out = _c8_alloc(n, c, h, w, dy.device)
        _lib.check(lib.mp_f16_to_c8(_lib.ptr(dy), _lib.ptr(out), n, c, h, w, _lib.stream()), "mp_f16_to_c8")
        return out, None


class Conv2dFn(torch.autograd.Function):
    """z = conv2d(x, weight) (+ bias); k in {1, 3}, stride in {1, 2}, padding = k // 2."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding):
        return _conv_forward(_F32, ctx, x, weight, bias, stride, padding)

    @staticmethod
    def backward(ctx, dz):
        return _conv_backward(_F32, ctx, dz)


class Conv16Fn(torch.autograd.Function):
    """z = conv2d(x, fp16(weight)) (+ bias) on the fp16 matrix cores; k in {1, 3}, stride in {1, 2}, padding = k // 2."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding):
        return _conv_forward(_F16, ctx, x, weight, bias, stride, padding)

    @staticmethod
    def backward(ctx, dz):
        return _conv_backward(_F16, ctx, dz)


class BatchNormActFn(torch.autograd.Function):
    """y = act(BN_train(z) (+ res)); updates the moving statistics in place (mindspore.nn.BatchNorm2d training)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, res, moving_mean, moving_var, relu):
        return _bn_forward(_F32, ctx, z, gamma, beta, res, moving_mean, moving_var, relu)

    @staticmethod
    def backward(ctx, dy):
        return _bn_backward(_F32, ctx, dy)


class BatchNormAct16Fn(torch.autograd.Function):
    """y = act(BN_train(z) (+ res)) on channel-blocked fp16; statistics / gamma / beta (and their gradients) in fp32."""

    @staticmethod
    def forward(ctx, z, gamma, beta, res, moving_mean, moving_var, relu):
        return _bn_forward(_F16, ctx, z, gamma, beta, res, moving_mean, moving_var, relu)

    @staticmethod
    def backward(ctx, dy):
        return _bn_backward(_F16, ctx, dy)


class FuseSumFn(torch.autograd.Function):
    """out = relu(((base + up(t1)) + up(t2)) + up(t3)); terms at scale 1 are plain adds (hrnet.py:327-339)."""

    @staticmethod
    def forward(ctx, base, scales, *terms):
        return _fuse_sum_forward(_F32, ctx, base, scales, terms)

    @staticmethod
    def backward(ctx, dy):
        dbase, dts = _fuse_sum_backward(_F32, ctx, dy)
        return (dbase, None, *dts)


class FuseSum16Fn(torch.autograd.Function):
    """``links``: per operand (base, terms...) the BatchNorm link of the chain that produced it, or None - an operand whose only
    consumer is this sum gets its gradient masked and reduced by the backward kernel itself (``mp_f16_fuse_sum_bwd_term_stats``)."""

    @staticmethod
    def forward(ctx, base, scales, links, *terms):
        ctx.links = list(links) if links is not None else [None] * (1 + len(terms))
        return _fuse_sum_forward(_F16, ctx, base, scales, terms)

    @staticmethod
    def backward(ctx, dy):
        dbase, dts = _fuse_sum_backward(_F16, ctx, dy)
        return (dbase, None, None, *dts)


class StemConvFn(torch.autograd.Function):
    """ResNet stem: 7x7 stride-2 conv of the (3-channel, fp32 NCHW) image - forward on the fp32 MFMA kernel, weight gradient by
    the direct-reduction kernel (3 input channels leave the matrix cores nothing to do); the image gets no gradient."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding):
        lib = _lib.load()
        x = _lib.require_cuda_f32(x, "x")
        w = weight.detach().contiguous()
        n, cin, h, wd = x.shape
        cout, _, k, _ = w.shape
        if stride != 2 or padding != k // 2 or cin > 4:
            raise NotImplementedError("stem conv: stride 2, padding k//2, <= 4 input channels")
        ho, wo = (h + 2 * padding - k) // 2 + 1, (wd + 2 * padding - k) // 2 + 1
        ones, zeros = _ones_zeros(cout, x.device)
        z = torch.empty(n, cout, ho, wo, device=x.device, dtype=torch.float32)
        d = _desc(n, cin, h, wd, cout, k, 2, padding, padding, ho, wo, ho, wo)
        _conv_launch(lib, d, x, _pack(lib, w, cout, cin, k, 0), ones, zeros, z, "stem conv")
        ctx.save_for_backward(x, w)
        return z

    @staticmethod
    def backward(ctx, dz):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        dz = dz.contiguous()
        n, cin, h, wd = x.shape
        cout, _, k, _ = w.shape
        dw = torch.empty_like(w)
        _lib.check(lib.mp_stem_conv_wgrad(_lib.ptr(x), _lib.ptr(dz), _lib.ptr(dw), n, cin, h, wd, cout, k, _lib.stream()),
                   "mp_stem_conv_wgrad")
        return None, dw, None, None


class MaxPoolFn(torch.autograd.Function):
    """nn.MaxPool2d(3, 2, pad_mode="same") on fp32 NCHW (resnet.py:190)."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _lib.require_cuda_f32(x, "x")
        n, c, h, w = x.shape
        out = torch.empty(n, c, (h + 1) // 2, (w + 1) // 2, device=x.device, dtype=torch.float32)
        _lib.check(lib.mp_maxpool3x3s2_same(_lib.ptr(x), _lib.ptr(out), n, c, h, w, _lib.stream()), "mp_maxpool3x3s2_same")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        n, c, h, w = x.shape
        dx = torch.empty_like(x)
        _lib.check(lib.mp_maxpool3x3s2_same_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dx), n, c, h, w, _lib.stream()),
                   "mp_maxpool3x3s2_same_bwd")
        return dx


class Deconv16Fn(torch.autograd.Function):
    """Conv2dTranspose(k=4, s=2, p=1) on channel-blocked fp16 (simple_baseline_head.py:80-88), weight [Cin, Cout, 4, 4].
    Forward: four 2x2 sub-pixel phase convs.  Data gradient: per phase, the strided gather of dy followed by the 2x2 conv with
    roles swapped (running sum through the epilogue).  Weight gradient: the 4x4 stride-2 weight-gradient GEMM with the roles of
    input and output gradient exchanged."""

    @staticmethod
    def forward(ctx, x, weight):
        return _deconv_forward(_F16, ctx, x, weight)

    @staticmethod
    def backward(ctx, dy):
        return _deconv_backward(_F16, ctx, dy)


class DeconvFn(torch.autograd.Function):
    """fp32 NCHW form of ``Deconv16Fn``."""

    @staticmethod
    def forward(ctx, x, weight):
        return _deconv_forward(_F32, ctx, x, weight)

    @staticmethod
    def backward(ctx, dy):
        return _deconv_backward(_F32, ctx, dy)


def stem_conv_bn_relu(x, conv, bn):
    """ResNet stem group conv7x7 s2 + BatchNorm(train) + ReLU on the fp32 image."""
    z = StemConvFn.apply(x, conv.weight, conv.stride, conv.padding)
    return BatchNormActFn.apply(z, bn.gamma, bn.beta, None, bn.moving_mean, bn.moving_variance, True)


def maxpool3x3s2_same(x):
    return MaxPoolFn.apply(x)


def deconv_bn_relu(x, deconv, bn):
    """Conv2dTranspose(4, 2, 1) + BatchNorm(train) + ReLU of the SimpleBaseline head."""
    _claim(x)
    if _is_c8(x):
        y = Deconv16Fn.apply(x, deconv.weight)
        return BatchNormAct16Fn.apply(y, bn.gamma, bn.beta, None, bn.moving_mean, bn.moving_variance, True)
    y = DeconvFn.apply(x, deconv.weight)
    return BatchNormActFn.apply(y, bn.gamma, bn.beta, None, bn.moving_mean, bn.moving_variance, True)


def to_c8(x: torch.Tensor) -> torch.Tensor:
    return ToC8Fn.apply(x)


def from_c8(x: torch.Tensor, channels: int) -> torch.Tensor:
    _claim(x)
    return FromC8Fn.apply(x, channels)


def _is_c8(x) -> bool:
    return x.dtype == torch.float16 and x.dim() == 5


class _SubCtx:
    """The slice of an autograd context the per-cell bodies use, so that a composite Function can run them itself."""

    def __init__(self, n_inputs):
        self.needs_input_grad = (True,) * n_inputs
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def _residual_forward(P, ctx, x, meta, params):
    groups = []
    y = x
    n_groups = len(meta)
    for gi, (stride, padding, mm, mv) in enumerate(meta):
        w, gamma, beta = params[3 * gi: 3 * gi + 3]
        cc, bc = _SubCtx(5), _SubCtx(7)
        z = _conv_forward(P, cc, y, w, None, stride, padding)
        last = gi == n_groups - 1
        y = _bn_forward(P, bc, z, gamma, beta, x if last else None, mm, mv, True)
        groups.append((cc, bc))
    ctx.groups = groups
    return y


def _residual_backward(P, ctx, dy):
    grads = []
    g = dy
    dres = None
    for gi in range(len(ctx.groups) - 1, -1, -1):
        cc, bc = ctx.groups[gi]
        dz, dgamma, dbeta, dr, _, _, _ = _bn_backward(P, bc, g)
        if dr is not None:
            dres = dr
        if gi == 0:
            cc.dx_residual = dres
        g, dw, _, _, _ = _conv_backward(P, cc, dz)
        grads = [dw, dgamma, dbeta] + grads
    ctx.groups = None
    return (g, None, *grads)


class ResidualBlock16Fn(torch.autograd.Function):
    """A whole residual block - conv+BN+ReLU groups whose last BatchNorm adds the block input and applies the ReLU (BasicBlock: two
    groups, Bottleneck without down-sample: three) - as ONE autograd node.  Same launches as the per-cell Functions (it runs
    their bodies); what it saves is autograd's separate launch that sums the two gradients reaching the block input: the
    identity's gradient is added in the epilogue of the first conv's data-gradient launch (104 launches per HRNet-W32 step)."""

    @staticmethod
    def forward(ctx, x, meta, *params):
        return _residual_forward(_F16, ctx, x, meta, params)

    @staticmethod
    def backward(ctx, dy):
        return _residual_backward(_F16, ctx, dy)


class ResidualBlock32Fn(torch.autograd.Function):
    """`ResidualBlock16Fn` on fp32 NCHW."""

    @staticmethod
    def forward(ctx, x, meta, *params):
        return _residual_forward(_F32, ctx, x, meta, params)

    @staticmethod
    def backward(ctx, dy):
        return _residual_backward(_F32, ctx, dy)


# ---- amp O2: BatchNorm fused into the neighbouring convs (round 3) ----------------------------------------------------------------
# A chain  conv -> BN (-> ReLU) [-> conv -> BN ...] (+ chain input on the last BN)  is ONE autograd node whose conv launches also do
# the BatchNorm REDUCTIONS (csrc/conv_f16_dev.h):
#   forward   conv_i's epilogue leaves the partial sums of z_i, z_i^2        -> BN_i runs its apply pass only
#   backward  the data-gradient launch that produces the gradient reaching BN_i's OUTPUT (conv_{i+1}'s, or - across nodes - the
#             first conv of the NEXT chain, residual gradient included) masks it with y_i > 0 and leaves the partial sums of g, g z_i
#             -> BN_i's backward runs its apply pass only, on the pre-masked gradient (which is also the residual branch's gradient)
# The cross-node hand-over goes through a `_BnLink` the producing chain hangs on its output tensor.  It is used only when the
# consuming chain is the tensor's ONLY consumer: every function of this module that takes a channel-blocked activation counts
# itself on the link (`_claim`), so a second consumer - autograd then SUMS gradients, and the sum is not what the conv's epilogue
# saw - switches the hand-over off for that tensor and the BatchNorm falls back to its own reduction launch.
# MINDPOSE_BN_FUSE=0 keeps the per-cell functions everywhere (A/B, parity tests of the two paths against each other).


def bn_fuse_enabled() -> bool:
    return _lib.env_on("MINDPOSE_BN_FUSE")


def _bn_fuse_parts() -> int:
    """Bit mask of the fused pieces (debugging / A-B): 1 forward statistics, 2 backward statistics inside a chain, 4 across chains,
    8 from the element-wise gradient producers (fan-out sum, exchange-unit backward), 16 from the merged-phase launch of a
    stride-2 data gradient."""
    return int(os.environ.get("MINDPOSE_BN_FUSE_PARTS", "31"))


class _BnLink:
    """The last BatchNorm of a chain, as seen by whoever consumes the chain's output: its input z, its output y (mask), whether it
    has a ReLU.  ``claimed`` counts the consumers of y that know about links; ``partials`` is filled by the consumer's data-gradient
    launch together with ``g``, the pre-masked gradient tensor that launch wrote.  The producer trusts the partial sums only for a
    gradient that IS that tensor (`_link_pre`): a consumer outside this module (a plain torch op, a hook, an auxiliary loss) never
    calls `_claim`, but autograd then hands the producer the SUM of two gradients in a fresh tensor - the check fails and the
    BatchNorm falls back to its own reduce-and-apply pass."""
    __slots__ = ("z", "y", "relu", "claimed", "partials", "n_parts", "g")

    def __init__(self, z, y, relu):
        self.z, self.y, self.relu, self.claimed, self.partials, self.n_parts, self.g = z, y, relu, 0, None, 0, None

    def hand_over(self, part, n_parts, g):
        self.partials, self.n_parts, self.g = part, n_parts, g


def _link_pre(link, dy):
    """(partials, n_parts) when ``dy`` is the pre-masked gradient the link's consumer wrote, else None."""
    if link is None or link.partials is None or link.claimed != 1 or link.g is None:
        return None
    if link.g.data_ptr() != dy.data_ptr() or tuple(link.g.shape) != tuple(dy.shape) or link.g.dtype != dy.dtype:
        return None
    return link.partials, link.n_parts


def _claim(t):
    """A consumer of the activation ``t`` announces itself (see above); returns the link or None."""
    link = getattr(t, "_mp_bn_link", None)
    if link is not None:
        link.claimed += 1
    return link


def _stats_alloc(lib, d, v, c8out, device):
    """Partial-sum buffer of a conv launch with epilogue statistics: (tensor, n_parts) or (None, 0) when variant ``v`` has no
    statistics build for this shape."""
    n_parts = lib.mp_f16_conv_stats_parts(ctypes.byref(d), v)  # v = -1 (tiny layers, tuner off): the library's own choice
    if n_parts <= 0:
        return None, 0
    return torch.empty(c8out * n_parts * 16, device=device, dtype=torch.float32), n_parts


def bn_pre_enabled() -> bool:
    """``MINDPOSE_BN_PRE=1``: inside a chain, conv -> BatchNorm -> ReLU -> 3x3 conv runs WITHOUT an apply pass over the first conv's
    output: the statistics are finalised by a one-block launch and the second conv applies them while it stages its operand,
    writing the activation for the backward pass on the way (bit-identical to the apply pass at launch level,
    tests/test_gpu_bn_fuse.py).  Off by default: measured on HRNet-W32 N = 128 the eager step's kernel time drops 2 % (27.2 ->
    26.6 ms) but the graph-replayed multi-lane step gets 0.8 % SLOWER (5.59 -> 5.55 k img/s, four interleaved pairs on two boxes) -
    the apply passes it removes are HBM-bound launches that were already hidden under the other lanes' convs, the time it adds sits
    in CU-filling conv launches."""
    return _lib.env_on("MINDPOSE_BN_PRE", default=False)


_PRE_CAPABLE = {}


def _pre_capable(lib, d) -> bool:
    """Can a conv launch of shape ``d`` apply the BatchNorm of the layer below on its own operand?  (some variant of the
    weights-in-registers family takes it, and the layer is large enough for the tuner to pick variants at all)"""
    key = tuple(getattr(d, f) for f, _ in d._fields_)
    hit = _PRE_CAPABLE.get(key)
    if hit is None:
        macs = d.n * d.conv_h * d.conv_w * d.cout * d.cin * d.kh * d.kw
        hit = (autotune_on() and macs >= (1 << 26)
               and any(lib.mp_f16_conv_pre_supported(ctypes.byref(d), v) for v in range(F16_VARIANTS)))
        _PRE_CAPABLE[key] = hit
    return hit


def _conv16_stats_launch(lib, d, x, packed, scale, shift, out, res1, mode, z=None, y=None, relu=0, pre=None, into=None):
    """The tuned conv launch with epilogue statistics (mode 1 forward / 2 backward); returns (partials, n_parts) or (None, 0) after
    a PLAIN launch when the tuned variant has no statistics build.  ``pre`` = dict(scale, shift, y, relu): ``x`` is the RAW output of
    the conv below and the launch applies that layer's BatchNorm on its operand, writing the activation to ``pre["y"]`` (the caller
    checked `_pre_capable`).  ``into`` = (variant, partials): one phase of a stride-2 data gradient, launched with the merged
    launch's variant into the merged launch's partial-sum buffer (`_dgrad16_stride2`)."""
    stats = dict(mode=mode, z=z, y=y, relu=relu)
    if pre is not None:
        stats["pre"] = pre
    if into is not None:
        v, part = into
        n_parts = part.numel() // (((d.cout + 7) // 8) * 16)
    else:
        v = tune_conv_variant(lib, d, x, packed, scale, shift, res1, None, out, half=True, stats=stats)
        part, n_parts = _stats_alloc(lib, d, v, (d.cout + 7) // 8, out.device)
    if pre is not None and (part is None or v < 0):
        raise _lib.MindposeHipError("no conv variant applies the BatchNorm on its operand for a shape _pre_capable admitted")
    if part is None:
        _conv16_run(lib, d, v, x, packed, scale, shift, res1, out, "mp_f16_conv2d_fwd")
        return None, 0
    st = _lib.ConvStats(mode=mode, relu=int(relu), partials=part.data_ptr(), partials_bytes=part.numel() * 4,
                        z=_lib.ptr(z), y=_lib.ptr(y) if relu else None)
    if pre is not None:
        st.pre_scale, st.pre_shift, st.pre_out, st.pre_relu = _lib.ptr(pre["scale"]), _lib.ptr(pre["shift"]), _lib.ptr(pre["y"]), int(pre["relu"])
    _lib.check(lib.mp_f16_conv2d_fwd_stats(ctypes.byref(d), v, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(shift),
                                           _lib.ptr(res1), _lib.ptr(out), ctypes.byref(st), _lib.stream()), "mp_f16_conv2d_fwd_stats")
    return part, n_parts


# ---- deferred, grouped weight gradients ------------------------------------------------------------------------------------------------
# A weight gradient is a leaf of the backward pass: nothing reads it before the optimizer.  The fused chains therefore do not launch
# it per layer: the (input, output-gradient, arena slot) triple is queued under its launch shape and stream, and every
# ``WGRAD_GROUP`` layers of one shape - the eight 3x3 convs of an HRNet branch (hrnet.py:202-241) - run as ONE
# ``mp_f16_conv_wgrad_grouped`` launch pair: per layer fewer and longer pixel slabs (an eighth of the split-K traffic), an eighth of
# the launches.  ``flush_wgrad_jobs()`` runs the remainders; whoever reads the gradient arena calls it first (the arena optimizers'
# ``step``, ``GraphedTrainStep`` before its capture ends).  MINDPOSE_WGRAD_GROUP=1 launches every layer on its own as before.
WGRAD_GROUP = 8
_WGRAD_PENDING = {}


def _wgrad_group_size() -> int:
    return max(1, min(WGRAD_GROUP, int(os.environ.get("MINDPOSE_WGRAD_GROUP", str(WGRAD_GROUP)))))


def _wgrad_enqueue(lib, d, x, dz, dw):
    """Queue dW += x (*) dz (accumulating into the arena slot ``dw``); launches the group when it is full."""
    dev = x.device
    # one queue per launch shape, whatever stream a layer ran on: the groups - and with them the split-K partition, i.e. the bits -
    # are the same for a single-stream step and for one whose branches / exchange-unit rows run on side streams
    key = (tuple(getattr(d, f) for f, _ in d._fields_), dev)
    jobs = _WGRAD_PENDING.setdefault(key, [])
    jobs.append((d, x, dz, dw, torch.cuda.current_stream(dev).cuda_stream))
    if len(jobs) >= _wgrad_group_size():
        # (keeping a full group of the branch-0 chain queued for the side stream at the module boundary - instead of 140 us of
        # bandwidth-bound launches at the end of the longest chain - was measured SLOWER: 23.7 vs 22.0 ms per step; the concurrent
        # stream takes HBM from the chain it was meant to shorten)
        _wgrad_flush_key(lib, key)
    elif not _WGRAD_CALLBACK[0]:
        # the remainders are launched when THIS backward pass ends (autograd's final callbacks run after the engine has joined the
        # streams of the pass with the caller's stream): whoever looks at the gradient arena after backward() sees them
        _WGRAD_CALLBACK[0] = True
        torch.autograd.Variable._execution_engine.queue_callback(_wgrad_backward_done)


def _wgrad_flush_key(lib, key, joined: bool = False):
    jobs = _WGRAD_PENDING.pop(key, [])
    if not jobs:
        return
    d, dev = jobs[0][0], key[1]
    n = len(jobs)
    # the group runs on the current stream, behind the producers of every operand (layers that ran on other streams); ``joined``: the
    # caller's stream is already ordered behind all of them (the early flush below forks from such a point)
    cur = torch.cuda.current_stream(dev)
    for sid in sorted({j[4] for j in jobs}):
        if sid != cur.cuda_stream and not joined:
            cur.wait_stream(torch.cuda.ExternalStream(sid, device=dev))
    for _, x, dz, _, sid in jobs:
        if sid != cur.cuda_stream:
            # operands allocated on another stream's pool are read by a launch on THIS stream: tell the caching allocator, or the
            # blocks could be handed out again on their origin stream while the grouped kernel still reads them
            x.record_stream(cur)
            dz.record_stream(cur)
    with torch.cuda.device(dev):
        if n == 1:
            _, x, dz, dw, _ = jobs[0]
            _wgrad_launch(_F16, lib, d, x, dz, dw, 1, "mp_f16_conv_wgrad")
            return
        wsb = lib.mp_f16_conv_wgrad_grouped_workspace_bytes(ctypes.byref(d), n)
        ws = torch.empty(max(wsb // 4, 1), device=dev, dtype=torch.float32)
        arr = ctypes.c_void_p * n
        _lib.check(lib.mp_f16_conv_wgrad_grouped(ctypes.byref(d), arr(*[_lib.ptr(j[1]) for j in jobs]), arr(*[_lib.ptr(j[2]) for j in jobs]),
                                                 arr(*[_lib.ptr(j[3]) for j in jobs]), n, 1.0, 1, _lib.ptr(ws), wsb, _lib.stream()),
                   "mp_f16_conv_wgrad_grouped")


_WGRAD_CALLBACK = [False]
_WGRAD_AUTOFLUSH = [True]


def set_wgrad_autoflush(on: bool) -> bool:
    """Whether the end of EVERY backward() call launches the queued remainders (default).  A segmented step (utils/graph_step.py)
    runs one backward pass as several autograd calls and turns this off in between, so that the weight-gradient groups - and with
    them the split-K partitions, i.e. the bits - are those of the single-call pass; it flushes itself after the last segment.
    Returns the previous setting."""
    prev = _WGRAD_AUTOFLUSH[0]
    _WGRAD_AUTOFLUSH[0] = bool(on)
    return prev


def pending_wgrad_slots():
    """data_ptr of every gradient-arena slot that still has a queued (not yet launched) weight gradient."""
    return {j[3].data_ptr() for jobs in _WGRAD_PENDING.values() for j in jobs}


def _wgrad_backward_done() -> None:
    _WGRAD_CALLBACK[0] = False
    if _WGRAD_AUTOFLUSH[0]:
        flush_wgrad_jobs()


def drop_wgrad_jobs(lo: int = 0, hi: int = 1 << 63) -> None:
    """Forget queued weight gradients WITHOUT launching them (a backward pass that raised leaves jobs holding that pass's
    activations; the gradient arena's ``begin_step`` calls this so they can never be accumulated into the next step).  Only jobs
    whose destination slot lies in ``[lo, hi)`` - the caller's own arena - are dropped: a second model / optimizer in the process
    keeps its queue."""
    for key in list(_WGRAD_PENDING):
        keep = [j for j in _WGRAD_PENDING[key] if not (lo <= j[3].data_ptr() < hi)]
        if keep:
            _WGRAD_PENDING[key] = keep
        else:
            del _WGRAD_PENDING[key]
    if not _WGRAD_PENDING:
        _WGRAD_CALLBACK[0] = False


_WGRAD_SIDE = {}          # device -> the stream of the early flush
_WGRAD_SIDE_BUSY = set()  # devices whose early flush has not been joined yet


def flush_wgrad_jobs_early() -> None:
    """Launch what is queued NOW on a side stream forked from the current one, to be joined by the next `flush_wgrad_jobs`.  HRNet
    calls it (a gradient hook on the stage-1 output) when the backward pass reaches stage 1: the remainders of stages 2 - 4 - ~1.5 ms
    of bandwidth-bound launches that used to run alone behind the backward pass - then stream beside the branch-less stage-1 /
    stem backward (also bandwidth-bound, on ONE queue: two such streams together get more of the HBM than either alone).  The jobs
    and their groups are those the end-of-pass flush would have formed (no later layer has the shapes of stages 2 - 4): same bits.
    Only with the automatic end-of-pass flush on (a segmented capture carries its groups across the cuts itself)."""
    if not _WGRAD_PENDING or not _WGRAD_AUTOFLUSH[0] or not _lib.env_on("MINDPOSE_WGRAD_EARLY_FLUSH"):
        return
    dev = next(iter(_WGRAD_PENDING))[1]
    cur = torch.cuda.current_stream(dev)
    side = _WGRAD_SIDE.get(dev)
    if side is None:
        side = _WGRAD_SIDE[dev] = torch.cuda.Stream(device=dev)
    # every queued job was produced by a node upstream of the caller's gradient: the current stream is ordered behind all of them
    keys = [k for k in _WGRAD_PENDING if k[1] == dev]
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        lib = _lib.load()
        for key in keys:
            _wgrad_flush_key(lib, key, joined=True)
    _WGRAD_SIDE_BUSY.add(dev)


def flush_wgrad_jobs() -> None:
    """Launch every queued weight gradient on the current stream (each group behind the producers of its operands): the arena is
    complete for whatever the caller enqueues next."""
    _WGRAD_CALLBACK[0] = False
    for dev in list(_WGRAD_SIDE_BUSY):  # an early flush of this pass: its launches are part of "the arena is complete"
        torch.cuda.current_stream(dev).wait_stream(_WGRAD_SIDE[dev])
        _WGRAD_SIDE_BUSY.discard(dev)
    if not _WGRAD_PENDING:
        return
    lib = _lib.load()
    for key in list(_WGRAD_PENDING):
        _wgrad_flush_key(lib, key)


def _run_bn_fwd_job(lib, j):
    """The BatchNorm forward pass a chain yielded: apply-only when the statistics came with the conv, reduce + apply otherwise;
    statistics only (``pre``) when the next conv of the chain applies them on its operand."""
    if j.get("pre") is not None:
        _lib.check(lib.mp_f16_bn_train_finalize(_lib.ptr(j["g"]), _lib.ptr(j["b"]), _lib.ptr(j["mean"]), _lib.ptr(j["invstd"]), _lib.ptr(j["mm"]),
                                                _lib.ptr(j["mv"]), j["n"], j["c"], j["hw"], BN_EPS, BN_MOMENTUM, _lib.ptr(j["part"]),
                                                j["n_parts"], _lib.ptr(j["pre"]["scale"]), _lib.ptr(j["pre"]["shift"]), _lib.ptr(j["ws"]),
                                                j["ws_bytes"], _lib.stream()), "mp_f16_bn_train_finalize")
        return
    if j["part"] is None:
        _bn_fwd_launch(_F16, lib, j)
    else:
        _lib.check(lib.mp_f16_bn_train_fwd_stats(_lib.ptr(j["z"]), _lib.ptr(j["g"]), _lib.ptr(j["b"]), _lib.ptr(j["res"]), _lib.ptr(j["y"]),
                                                 _lib.ptr(j["mean"]), _lib.ptr(j["invstd"]), _lib.ptr(j["mm"]), _lib.ptr(j["mv"]), j["n"],
                                                 j["c"], j["hw"], BN_EPS, BN_MOMENTUM, j["relu"], _lib.ptr(j["part"]), j["n_parts"],
                                                 _lib.ptr(j["ws"]), j["ws_bytes"], _lib.stream()), "mp_f16_bn_train_fwd_stats")


def _run_bn_bwd_job(lib, j):
    """The backward counterpart: apply-only on a pre-masked gradient whose sums its producer delivered, else reduce + apply."""
    if j["pre"] is None:
        _bn_bwd_launch(_F16, lib, j)
    else:
        _lib.check(lib.mp_f16_bn_train_bwd_stats(_lib.ptr(j["dy"]), _lib.ptr(j["z"]), _lib.ptr(j["g"]), _lib.ptr(j["mean"]),
                                                 _lib.ptr(j["invstd"]), _lib.ptr(j["dz"]), _lib.ptr(j["dgamma"]), _lib.ptr(j["dbeta"]),
                                                 _lib.ptr(j["ga"]), _lib.ptr(j["ba"]), j["n"], j["c"], j["hw"], _lib.ptr(j["pre"][0]),
                                                 j["pre"][1], _lib.ptr(j["ws"]), j["ws_bytes"], _lib.stream()), "mp_f16_bn_train_bwd_stats")


def _chain16_fwd_steps(lib, x, meta, residual, res_ext, params):
    """Forward of one conv-BatchNorm chain as a generator: launches a group's conv, YIELDS the BatchNorm job (the driver runs it)
    and goes on; returns (groups, output)."""
    groups = []
    a = x
    n_groups = len(meta)
    pre = None  # the previous group's BatchNorm, left to THIS group's conv: dict(scale, shift, y, relu, z)
    for gi, (stride, padding, mm, mv, relu) in enumerate(meta):
        weight, gamma, beta = params[3 * gi: 3 * gi + 3]
        w = weight.detach().contiguous()
        d, packed, ones, zeros, z, (n, cout, ho, wo) = _conv_fwd_args(_F16, lib, a, weight, w, None, stride, padding)
        if pre is not None:  # operand = the raw output below; this launch applies its BatchNorm and writes the activation `a`
            part, n_parts = _conv16_stats_launch(lib, d, pre["z"], packed, ones, zeros, z, None, 1, pre=pre)
            pre = None
        elif _bn_fuse_parts() & 1:
            part, n_parts = _conv16_stats_launch(lib, d, a, packed, ones, zeros, z, None, 1)
        else:
            part, n_parts = None, 0
            _conv16_launch(lib, d, a, packed, ones, zeros, z, "mp_f16_conv2d_fwd")
        last = gi == n_groups - 1
        res = (x if residual else res_ext) if last else None
        job = _bn_fwd_job(_F16, lib, z, gamma, beta, res, mm, mv, relu)
        job["part"], job["n_parts"] = part, n_parts
        y = job["y"]
        if not last and part is not None and bn_pre_enabled() and cout % 8 == 0:
            # conv -> BatchNorm -> ReLU -> 3x3 conv (hrnet.py:67-72): when the next conv can take the raw z, only the statistics
            # are finalised here - no pass over z / y; the next launch writes y (the backward pass reads it) on the way
            ns, npad = meta[gi + 1][0], meta[gi + 1][1]
            nw = params[3 * (gi + 1)]
            if nw.shape[2] == 3 and ns == 1 and npad == 1:
                dn = _desc(n, cout, ho, wo, nw.shape[0], 3, 1, 1, 1, ho, wo, ho, wo)
                only = os.environ.get("MINDPOSE_BN_PRE_CH")  # kernel work: the operand route for these channel counts only
                min_hw = int(os.environ.get("MINDPOSE_BN_PRE_MINHW", "0"))  # ... and maps of at least this many pixels
                if _pre_capable(lib, dn) and (not only or str(cout) in only.split(",")) and ho * wo >= min_hw:
                    pre = dict(scale=torch.empty((cout + 7) // 8 * 8, device=z.device), shift=torch.empty((cout + 7) // 8 * 8, device=z.device),
                               y=y, relu=int(relu), z=z)
                    job["pre"] = pre
        yield job
        groups.append(dict(a=a, w=w, weight=weight, gamma=gamma, beta=beta, g=job["g"], b=job["b"], z=z, y=y, mean=job["mean"],
                           invstd=job["invstd"], stride=stride, padding=padding, relu=bool(relu), res=res is not None))
        a = y
    return groups, a


def _chain16_bwd_steps(lib, groups, dy, out_link, in_link, needs_dx, res_is_input):
    """Backward of one chain as a generator: YIELDS each group's BatchNorm backward job, then queues the weight gradient and
    launches the data gradient (which masks / reduces for the BatchNorm below); returns (dx, dres, grads)."""
    dy = dy.contiguous()
    grads = []
    # the gradient reaching the LAST BatchNorm: pre-masked with partial sums when the (only) consumer's data gradient made them
    pre = _link_pre(out_link, dy)
    dres = None
    for gi in range(len(groups) - 1, -1, -1):
        G = groups[gi]
        z, y, a, w = G["z"], G["y"], G["a"], G["w"]
        n, ho, wo = _nhw(z)
        cout, cin, k, _ = w.shape
        h, wd = a.shape[2], a.shape[3]
        job = _bn_bwd_job(_F16, lib, dy, z, G["g"], G["b"], G["mean"], G["invstd"], G["gamma"], G["beta"], G["relu"])
        job["pre"] = pre
        if pre is not None:  # apply pass only: dy is g = dy * mask, its sums came with it
            if G["res"]:
                dres = dy
        else:
            # without a residual the mask is re-derived from z, y is not read
            if G["relu"] and (G["res"] or not _lib.env_on("MINDPOSE_BN16_MASK_FROM_Z")):
                job["yy"] = y
            if G["res"]:
                dres = job["dr"] = torch.empty_like(z)
        yield job
        dz = job["dz"]
        dgamma, dbeta = (None, None) if job["ga"] is not None else (job["dgamma"], job["dbeta"])
        # ---- conv: weight gradient (a leaf; into the arena: queued, launched with the other layers of this shape), then the data
        # gradient that feeds the BatchNorm below
        s, pad = G["stride"], G["padding"]
        d = _desc(n, cin, h, wd, cout, k, s, pad, pad, ho, wo, ho, wo)
        dw = _wgrad(_F16, lib, d, a, dz, w, G["weight"], "mp_f16_conv_wgrad", queue=True)
        pre = None
        dx = None
        if gi > 0 or needs_dx:
            res1 = dres if (gi == 0 and res_is_input) else None  # the chain input's second path: added in this launch's epilogue
            # which BatchNorm does this gradient reach?  the previous group's - or, across nodes, the producer of the chain input
            below = link = None
            if gi > 0:
                if _bn_fuse_parts() & 2:
                    prev = groups[gi - 1]
                    below = (prev["z"], prev["y"], prev["relu"])
            elif in_link is not None and in_link.claimed == 1 and (_bn_fuse_parts() & 4):
                below, link = (in_link.z, in_link.y, in_link.relu), in_link
            if s != 1 and not (_bn_fuse_parts() & 16):  # the merged-phase launch of a stride-2 data gradient stays plain
                below = None
            dx, part, n_parts = _conv_dgrad(_F16, lib, a, w, G["weight"], dz, s, pad, res1=res1, below=below)
            if part is not None:
                if link is not None:
                    link.hand_over(part, n_parts, dx)
                else:
                    pre = (part, n_parts)
        elif gi == 0 and dres is not None and res_is_input:
            dx = dres
        grads = [dw, dgamma, dbeta] + grads
        dy = dx
    return dy, dres, grads


def _drive(gen, run_job, lib):
    """Run a chain generator to its end, executing the BatchNorm job it yields at every group; returns its return value.
    (The chains are generators so that a driver CAN interleave several of them - the lockstep experiment of DESIGN 4.9.)"""
    while True:
        try:
            job = next(gen)
        except StopIteration as stop:
            return stop.value
        run_job(lib, job)


class Chain16Fn(torch.autograd.Function):
    """``meta`` = per group (stride, padding, moving_mean, moving_var, relu); ``residual``: the chain input is added before the last
    group's activation (BasicBlock / Bottleneck without down-sample, hrnet.py:66-83, 126-146); ``params`` = (weight, gamma, beta)
    per group.  k in {1, 3}, stride in {1, 2}, padding = k // 2, no conv bias."""

    @staticmethod
    def forward(ctx, x, meta, residual, in_link, res_ext, *params):
        """``res_ext``: a second tensor added before the last group's activation instead of the chain input (the block with a
        down-sample path, hrnet.py:74-81: identity = bn(conv1x1(x)))."""
        lib = _lib.load()
        groups, a = _drive(_chain16_fwd_steps(lib, x, meta, residual, res_ext, params), _run_bn_fwd_job, lib)
        ctx.groups = groups
        ctx.in_link = in_link
        ctx.out_link = _BnLink(groups[-1]["z"], a, groups[-1]["relu"])
        ctx.needs_dx = x.requires_grad
        ctx.res_is_input = bool(residual)
        return a

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        groups, ctx.groups = ctx.groups, None
        dx, dres, grads = _drive(_chain16_bwd_steps(lib, groups, dy, ctx.out_link, ctx.in_link, ctx.needs_dx, ctx.res_is_input),
                                 _run_bn_bwd_job, lib)
        return (dx, None, None, None, None if ctx.res_is_input else dres, *grads)


def _chain16(x, groups, relus, residual, res_ext=None):
    """groups = [(conv, bn), ...] on a channel-blocked activation, as ONE fused node."""
    link = _claim(x)  # a residual chain's second use of x (the identity) is inside the node: still ONE consumer
    if res_ext is not None:
        _claim(res_ext)
    meta = tuple((cv.stride, cv.padding, bn.moving_mean, bn.moving_variance, bool(r)) for (cv, bn), r in zip(groups, relus))
    params = [t for cv, bn in groups for t in (cv.weight, bn.gamma, bn.beta)]
    y = Chain16Fn.apply(x, meta, bool(residual), link, res_ext, *params)
    out_link = getattr(y.grad_fn, "out_link", None)  # the node object IS the ctx of forward / backward
    if out_link is not None:
        y._mp_bn_link = out_link
    return y


def residual_block(x, groups):
    """``groups`` = [(conv, bn), ...]; relu(bn_k(conv_k(... relu(bn_1(conv_1 x)) ...)) + x).  Blocks with a stride-1 first conv take the
    one-node form above (both activation types); anything else composes the per-cell functions."""
    first = groups[0][0]
    if _is_c8(x) and bn_fuse_enabled() and first.stride == 1 and all(cv.bias is None for cv, _ in groups):
        return _chain16(x, groups, [True] * len(groups), residual=True)
    _claim(x)
    if first.stride == 1 and all(cv.bias is None for cv, _ in groups) and _lib.env_on("MINDPOSE_FUSE_RESIDUAL"):
        meta = tuple((cv.stride, cv.padding, bn.moving_mean, bn.moving_variance) for cv, bn in groups)
        params = [t for cv, bn in groups for t in (cv.weight, bn.gamma, bn.beta)]
        return (ResidualBlock16Fn if _is_c8(x) else ResidualBlock32Fn).apply(x, meta, *params)
    y = x
    for i, (cv, bn) in enumerate(groups):
        y = conv_bn_act(y, cv, bn, relu=True, res=x if i == len(groups) - 1 else None)
    return y


def conv_bn_act(x, conv, bn, relu: bool, res: Optional[torch.Tensor] = None):
    """One conv + BatchNorm(train) (+ residual) (+ ReLU) group of the reference's cells; the kernel family follows the
    activation type (fp32 NCHW, or channel-blocked fp16 under amp O2)."""
    if _is_c8(x):
        if bn is not None and conv.bias is None and bn_fuse_enabled():
            return _chain16(x, [(conv, bn)], [relu], residual=False, res_ext=res)
        _claim(x)
        if res is not None:
            _claim(res)
        z = Conv16Fn.apply(x, conv.weight, conv.bias, conv.stride, conv.padding)
        if bn is None:
            return z
        return BatchNormAct16Fn.apply(z, bn.gamma, bn.beta, res, bn.moving_mean, bn.moving_variance, relu)
    z = Conv2dFn.apply(x, conv.weight, conv.bias, conv.stride, conv.padding)
    if bn is None:
        return z
    return BatchNormActFn.apply(z, bn.gamma, bn.beta, res, bn.moving_mean, bn.moving_variance, relu)


class FanOutFn(torch.autograd.Function):
    """``k`` handles on one tensor for ``k`` consumers; the backward pass sums the ``k`` gradients in ONE launch
    (``mp_sum_tensors``: fp32 arithmetic, one rounding) instead of autograd's ``k - 1`` pairwise add kernels.  ``link``: the tensor
    is the output of a fused chain whose only consumer is this fan-out - the sum kernel then also masks the gradient and leaves the
    last BatchNorm's backward sums (``mp_f16_sum_tensors_stats``)."""

    @staticmethod
    def forward(ctx, x, k, link):
        ctx.set_materialize_grads(False)
        ctx.link = link
        return tuple(x.view_as(x) for _ in range(k))

    @staticmethod
    def backward(ctx, *grads):
        return _fan_in(grads, ctx.link), None, None


def _fan_in(grads, link):
    """The sum of one tensor's consumer gradients (None entries skipped) in one launch - with ``link`` (the tensor is the output of a
    fused chain whose only consumer is the fan-out) also the mask and the last BatchNorm's backward sums."""
    gs = [g.contiguous() for g in grads if g is not None]
    if not gs:
        return None
    if len(gs) == 1:
        return gs[0]
    lib = _lib.load()
    half = gs[0].dtype == torch.float16
    if (half and link is not None and link.claimed == 1 and len(gs) <= 4 and (_bn_fuse_parts() & 8)
            and tuple(link.z.shape) == tuple(gs[0].shape)):
        n, c8, h, w, _ = gs[0].shape
        n_parts = lib.mp_f16_ew_stats_parts(n, c8 * 8, h * w)
        part = torch.empty(c8 * n_parts * 16, device=gs[0].device, dtype=torch.float32)
        dst = torch.empty_like(gs[0])
        ops = gs + [None] * (4 - len(gs))
        _lib.check(lib.mp_f16_sum_tensors_stats(_lib.ptr(ops[0]), _lib.ptr(ops[1]), _lib.ptr(ops[2]), _lib.ptr(ops[3]), _lib.ptr(dst),
                                                _lib.ptr(link.z), _lib.ptr(link.y) if link.relu else None, int(link.relu), n, c8 * 8,
                                                h * w, _lib.ptr(part), part.numel() * 4, _lib.stream()), "mp_f16_sum_tensors_stats")
        link.hand_over(part, n_parts, dst)
        return dst
    out = gs[0]
    for i in range(1, len(gs), 3):  # up to four operands per launch (the running sum + three more)
        ops = gs[i:i + 3]
        dst = torch.empty_like(gs[0])
        _lib.check(lib.mp_sum_tensors(_lib.ptr(out), _lib.ptr(ops[0]), _lib.ptr(ops[1]) if len(ops) > 1 else None,
                                      _lib.ptr(ops[2]) if len(ops) > 2 else None, _lib.ptr(dst), dst.numel() * dst.element_size(),
                                      int(half), _lib.stream()), "mp_sum_tensors")
        out = dst
    return out


class FanOutManyFn(torch.autograd.Function):
    """`FanOutFn` for SEVERAL tensors as ONE autograd node: handles ``ks[j]`` on ``xs[j]``; the backward pass runs the tensors' fan-in
    sums one after the other inside one node.  Why one node: the branch chains of an HRModule's backward each start at "their"
    fan-in; as separate nodes on the current stream the fan-ins form a spine, every chain is released by an event behind a
    DIFFERENT kernel of it - and the hipGraph runtime then replays the chains almost one after the other (tools/probes/
    graph_spine_probe.py: 2217 us against 790 us concurrent / 2839 us serial), while chains forked from ONE point run concurrently
    (846 us).  As one node the engine records its consumers' events behind the LAST fan-in kernel: a single fork point."""

    @staticmethod
    def forward(ctx, ks, links, *xs):
        ctx.set_materialize_grads(False)
        ctx.ks, ctx.links = ks, links
        outs = []
        for x, k in zip(xs, ks):
            outs += [x.view_as(x) for _ in range(k)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        res, i = [], 0
        for k, link in zip(ctx.ks, ctx.links):
            res.append(_fan_in(grads[i:i + k], link))
            i += k
        return (None, None, *res)


class GradJoinFn(torch.autograd.Function):
    """Identity over several tensors as ONE autograd node: in the backward pass their gradients - produced at different points of
    the current stream - leave through one node, so the chains that consume them on side streams fork from a SINGLE point (see
    `FanOutManyFn`: chains released behind different kernels of a spine replay one after the other)."""

    @staticmethod
    def forward(ctx, *xs):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for x in xs)

    @staticmethod
    def backward(ctx, *grads):
        return grads  # the very tensors that came in: a BatchNorm hand-over (`_link_pre`) still recognises its gradient


def grad_join(xs):
    """``xs`` routed through `GradJoinFn` (the BatchNorm links travel with the tensors); a list of one, CPU tensors or tensors without
    gradient pass through."""
    xs = list(xs)
    if len(xs) < 2 or not all(x.is_cuda and x.requires_grad for x in xs) or not _lib.env_on("MINDPOSE_FAN_OUT_ONE_NODE"):
        return xs
    outs = GradJoinFn.apply(*xs)
    for o, x in zip(outs, xs):
        link = getattr(x, "_mp_bn_link", None)
        if link is not None:
            o._mp_bn_link = link
    return list(outs)


def fan_out_many(xs, ks):
    """``[fan_out(x, k) for x, k in zip(xs, ks)]`` with the fan-ins of the backward pass in ONE autograd node (`FanOutManyFn`);
    tensors with at most one consumer (or that `fan_out` would pass through) stay outside it."""
    outs = [None] * len(xs)
    pick = []
    for j, (x, k) in enumerate(zip(xs, ks)):
        if k <= 1 or not x.is_cuda or not x.requires_grad or (x.numel() * x.element_size()) % 16 or not _lib.env_on("MINDPOSE_FAN_OUT"):
            outs[j] = (x,) * k
        else:
            pick.append(j)
    if len(pick) == 1 or not _lib.env_on("MINDPOSE_FAN_OUT_ONE_NODE"):
        for j in pick:
            outs[j] = fan_out(xs[j], ks[j])
    elif pick:
        flat = FanOutManyFn.apply([ks[j] for j in pick], [_claim(xs[j]) for j in pick], *[xs[j] for j in pick])
        i = 0
        for j in pick:
            outs[j] = tuple(flat[i:i + ks[j]])
            i += ks[j]
    return outs


def fan_out(x, k: int):
    """``k`` handles on ``x`` whose gradients are summed by one kernel; needs 16-byte multiples (every activation here is)."""
    if k <= 1 or not x.is_cuda or not x.requires_grad or (x.numel() * x.element_size()) % 16 or not _lib.env_on("MINDPOSE_FAN_OUT"):
        return (x,) * k  # the consumers of the k handles count themselves on x's BatchNorm link (the same tensor object)
    return FanOutFn.apply(x, k, _claim(x))


def fuse_sum(base, terms):
    """terms = [(tensor, integer scale), ...] (1-3 entries)."""
    links = [_claim(base)] + [_claim(t) for t, _ in terms]
    if _is_c8(base):
        return FuseSum16Fn.apply(base, [s for _, s in terms], links, *[t for t, _ in terms])
    return FuseSumFn.apply(base, [s for _, s in terms], *[t for t, _ in terms])
