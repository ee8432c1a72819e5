"""The output bits of the fp16 convolution kernels (csrc/conv_f16*.hip), as digests: what tests/golden/gen_f16_conv_bits.py records on
the GPU from the library of the commit a change to those kernels starts from, and what tests/test_gpu_f16_conv_bits.py recomputes.

Cases: the served (case, variant) pairs of the tables of tests/f16_matrix.py, per kernel family and under the knobs the parity tests
use (``GROUPS``).  Each pair runs
  * the plain launch with the case's residual count,
  * ``mp_f16_conv2d_fwd_stats`` in mode 1 and in mode 2 (ReLU 1, at most one residual) wherever ``supported(..., stats=m)`` says so,
  * and, where ``mp_f16_conv_pre_supported`` answers 1, mode 1 with the BatchNorm of the layer below applied on the operand.
Inputs come from a seeded CPU generator (activations, packed weights, scale / shift, residuals, z / y, operand scale / shift); the
output, the partial sums and the operand-route activation tensor are pre-filled with a ramp, so that an element a kernel stops
writing changes the digest as well.  One record per (case, variant, knob set): the SHA-256 over the bytes every mode leaves behind.
"""
import ctypes
import functools
import hashlib

import numpy as np
import torch

from mindpose_amd import _lib
from tests import f16_matrix as fm

# name: (cases, variants, desc of a case, residuals of a case, knob sets)
GROUPS = {
    "tile": (fm.CONV_CASES, fm.TILE_VARIANTS, fm.conv_case_desc, fm.conv_case_res, [{}]),
    "mt": (fm.CONV_CASES, fm.MT_VARIANTS, fm.conv_case_desc, fm.conv_case_res, [{"MP_F16_MT_GROUPS": 1}, {"MP_F16_MT_GROUPS": 3}]),
    "wreg": (fm.WREG_CASES, fm.WREG_VARIANTS, fm.conv_case_desc, fm.conv_case_res, [{}]),
    "wreg_s2": (fm.WREG_S2_CASES, fm.WREG_S2_VARIANTS, fm.s2_case_desc, fm.s2_case_res, [{}]),
    "ws": (fm.WS_CASES, fm.WS_VARIANTS, fm.conv_case_desc, fm.conv_case_res, [{"MP_F16_WS_GROUPS": 2}, {"MP_F16_WS_GROUPS": 5}]),
    "phases4": (fm.PHASES4_CASES, fm.PHASES4_VARIANTS, fm.phases4_case_desc, lambda c: 0, [{}]),
}


def knob_id(env):
    return ",".join(f"{k}={v}" for k, v in sorted(env.items())) or "none"


def runs(group):
    """[(case index, knob set)] of a group: the unit one test covers"""
    cases, _, _, _, knob_sets = GROUPS[group]
    return [(ci, env) for env in knob_sets for ci in range(len(cases))]


def _round_up(v, m):
    return (v + m - 1) // m * m


def _c8(rng, n, c, h, w):
    """random activations in the channel-blocked layout [n][ceil(c/8)][h][w][8] fp16, padding channels zero"""
    c8 = (c + 7) // 8
    a = rng.standard_normal((n, c8 * 8, h, w), dtype=np.float32)
    a[:, c:] = 0
    return torch.from_numpy(a.reshape(n, c8, 8, h, w).transpose(0, 1, 3, 4, 2).astype(np.float16).copy())


def _ramp(shape, dtype):
    numel = int(np.prod(shape))
    return (-(1000.0 + (torch.arange(numel, dtype=torch.float32) % 251))).to(dtype).reshape(shape)


@functools.lru_cache(maxsize=2)
def _inputs(group, ci):
    """CPU tensors of a case, generated once per case and left unchanged"""
    cases, _, desc_of, _, _ = GROUPS[group]
    d = desc_of(cases[ci])
    rng = np.random.default_rng([sorted(GROUPS).index(group), ci])
    phases = 4 if d.flags & _lib.MP_CONV_PHASES4 else 1
    kq, taps, cp = _round_up(d.cin, 32) // 32, d.kh * d.kw, _round_up(d.cout, 16)
    w = rng.standard_normal((phases, kq, taps, 4, cp, 8), dtype=np.float32) / np.sqrt(d.cin * taps)
    w[:, :, :, :, d.cout:] = 0
    ci_of = np.arange(kq)[:, None, None] * 32 + np.arange(4)[None, :, None] * 8 + np.arange(8)[None, None, :]  # input channel of [q][g][j]
    w *= (ci_of < d.cin)[None, :, None, :, None, :]
    scale, shift = np.zeros(cp, np.float32), np.zeros(cp, np.float32)
    scale[:d.cout] = rng.random(d.cout, dtype=np.float32) + 0.5
    shift[:d.cout] = rng.standard_normal(d.cout, dtype=np.float32) * 0.1
    kp = _round_up(d.cin, 32)
    pre_scale, pre_shift = np.zeros(kp, np.float32), np.zeros(kp, np.float32)
    pre_scale[:d.cin] = rng.random(d.cin, dtype=np.float32) + 0.5
    pre_shift[:d.cin] = rng.standard_normal(d.cin, dtype=np.float32) * 0.2
    t = {"x": _c8(rng, d.n, d.cin, d.h, d.w), "w": torch.from_numpy(w.astype(np.float16)), "scale": torch.from_numpy(scale),
         "shift": torch.from_numpy(shift), "pre_scale": torch.from_numpy(pre_scale), "pre_shift": torch.from_numpy(pre_shift)}
    for name in ("res1", "res2", "z", "y"):
        t[name] = _c8(rng, d.n, d.cout, d.out_h, d.out_w)
    return d, t


def expected_keys(group):
    """the record names of a group, from the library's host-only answer (no GPU)"""
    cases, variants, desc_of, res_of, knob_sets = GROUPS[group]
    return [f"case{ci}-v{v}|{knob_id(env)}" for env in knob_sets for ci, case in enumerate(cases) for v in variants
            if fm.supported(desc_of(case), v, res_of(case), 0, **env)]


def pack(digests_of_run):
    """the stored form of one (case, knob set): {digest: [variants that leave these bytes]} (variants without a statistics build of
    their own share the plain launch's bytes)"""
    out = {}
    for key, digest in digests_of_run.items():
        out.setdefault(digest, []).append(int(key.split("-v")[1].split("|")[0]))
    return {digest: sorted(vs) for digest, vs in out.items()}


def run_id(ci, env):
    return f"case{ci}|{knob_id(env)}"


def _bytes(t):
    return t.cpu().contiguous().view(torch.uint8).numpy().tobytes()


def digests(group, ci, env):
    """{"case<ci>-v<variant>|<knobs>": SHA-256} of every served variant of one (case, knob set)"""
    cases, variants, _, res_of, _ = GROUPS[group]
    lib = _lib.load()
    d, cpu = _inputs(group, ci)
    n_res = res_of(cases[ci])
    out = {}
    with fm.knobs(**env):
        served = [v for v in variants if lib.mp_f16_conv_supported(ctypes.byref(d), v, n_res, 0)]
        if not served:
            return out
        dev = {k: v.cuda() for k, v in cpu.items()}
        p = {k: _lib.ptr(v) for k, v in dev.items()}
        o_shape = tuple(dev["z"].shape)
        for v in served:
            h = hashlib.sha256()
            o = _ramp(o_shape, torch.float16).cuda()
            _lib.check(lib.mp_f16_conv2d_fwd(ctypes.byref(d), v, p["x"], p["w"], p["scale"], p["shift"], p["res1"] if n_res >= 1 else None,
                                             p["res2"] if n_res >= 2 else None, _lib.ptr(o), _lib.stream()), f"{group} case {ci} variant {v}")
            h.update(b"plain")
            h.update(_bytes(o))
            r1 = min(n_res, 1)
            forms = [(m, False) for m in (1, 2) if lib.mp_f16_conv_supported(ctypes.byref(d), v, r1, m)]
            if lib.mp_f16_conv_pre_supported(ctypes.byref(d), v):
                forms.append((1, True))
            for mode, pre in forms:
                parts = lib.mp_f16_conv_stats_parts(ctypes.byref(d), v)
                assert parts > 0
                o = _ramp(o_shape, torch.float16).cuda()
                partials = _ramp((o_shape[1] * parts * 16,), torch.float32).cuda()
                pre_out = _ramp(tuple(dev["x"].shape), torch.float16).cuda()
                st = _lib.ConvStats(mode=mode, relu=1, partials=partials.data_ptr(), partials_bytes=partials.numel() * 4, z=p["z"], y=p["y"])
                if pre:
                    st.pre_scale, st.pre_shift, st.pre_out, st.pre_relu = p["pre_scale"], p["pre_shift"], _lib.ptr(pre_out), 1
                _lib.check(lib.mp_f16_conv2d_fwd_stats(ctypes.byref(d), v, p["x"], p["w"], p["scale"], p["shift"], p["res1"] if r1 else None,
                                                       _lib.ptr(o), ctypes.byref(st), _lib.stream()),
                           f"{group} case {ci} variant {v} statistics mode {mode}" + (" on the operand" if pre else ""))
                h.update(f"mode{mode}{'pre' if pre else ''}".encode())
                h.update(_bytes(o))
                h.update(_bytes(partials))
                if pre:
                    h.update(_bytes(pre_out))
            out[f"case{ci}-v{v}|{knob_id(env)}"] = h.hexdigest()
    return out
