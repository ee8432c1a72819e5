#!/usr/bin/env python3
"""fp16 weight-gradient kernel: LDS-DMA form vs the register-staged form on the HRNet layer shapes.
   python tools/bench_wgrad16.py [N] [--jobs J]     (--jobs J: J layers per launch through mp_f16_conv_wgrad_grouped, the path the
   training step takes; the time is per launch pair)"""
import ctypes, os, statistics, sys
os.environ.setdefault("MINDPOSE_EXPERIMENT_KNOBS", "1")  # the MP_* knobs below are honoured only then
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mindpose_amd import _lib
from mindpose_amd.models.act_c8 import ActC8
lib = _lib.load(); dev = torch.device("cuda:0")
argv = sys.argv[1:]
jobs = int(argv.pop(argv.index("--jobs") + 1)) if "--jobs" in argv else 0
argv = [a for a in argv if a != "--jobs"]
n = int(argv[0]) if argv else 128
SHAPES = [(32, 32, 64, 48, 3, 1), (64, 64, 32, 24, 3, 1), (128, 128, 16, 12, 3, 1), (256, 256, 8, 6, 3, 1), (64, 256, 64, 48, 1, 1),
          (256, 64, 64, 48, 1, 1), (64, 64, 64, 48, 3, 1), (32, 64, 64, 48, 3, 2), (64, 128, 32, 24, 3, 2)]
for cin, cout, h, w, k, st in SHAPES:
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    xs, dzs = [ActC8(n, cin, h, w, dev) for _ in range(max(jobs, 1))], [ActC8(n, cout, ho, wo, dev) for _ in range(max(jobs, 1))]
    for t in xs + dzs: t.c8_tensor.normal_()
    d = _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=st, pad_top=pad, pad_left=pad, conv_h=ho, conv_w=wo, out_h=ho,
                      out_w=wo, out_mul=1, out_rep=1, out_off_y=0, out_off_x=0, relu=0, flags=0)
    res, outs = {}, {}
    for mode in ("1", "0"):
        os.environ["MP_WGRAD16_DMA"] = mode
        dws = [torch.empty(cout, cin, k, k, device=dev) for _ in xs]
        if jobs:
            nb = lib.mp_f16_conv_wgrad_grouped_workspace_bytes(ctypes.byref(d), jobs)
            ws = torch.empty(nb // 4, device=dev)
            arr = ctypes.c_void_p * jobs
            fn, args = lib.mp_f16_conv_wgrad_grouped, (ctypes.byref(d), arr(*[_lib.ptr(t) for t in xs]), arr(*[_lib.ptr(t) for t in dzs]),
                                                       arr(*[_lib.ptr(t) for t in dws]), jobs, 1.0, 0, _lib.ptr(ws), nb, _lib.stream())
        else:
            nb = lib.mp_f16_conv_wgrad_workspace_bytes(ctypes.byref(d))
            ws = torch.empty(nb // 4, device=dev)
            fn, args = lib.mp_f16_conv_wgrad, (ctypes.byref(d), _lib.ptr(xs[0]), _lib.ptr(dzs[0]), _lib.ptr(dws[0]), 1.0, 0, _lib.ptr(ws), nb,
                                               _lib.stream())
        _lib.check(fn(*args), "wgrad")
        ts = []
        for _ in range(5):
            for _ in range(3): fn(*args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20): fn(*args)
            e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1) / 20 * 1e3)
        res[mode] = statistics.median(ts); outs[mode] = dws[-1].clone()
    gf = 2 * n * ho * wo * cout * cin * k * k * max(jobs, 1) / 1e9
    err = float((outs["1"] - outs["0"]).abs().max() / outs["0"].abs().max())
    print(f"{cin:3d}->{cout:3d} k{k} s{st} {h}x{w} N={n}{f' x{jobs}' if jobs else ''}: staged {res['0']:6.1f} us ({gf / res['0'] * 1e3:5.0f} TF)  "
          f"LDS-DMA {res['1']:6.1f} us ({gf / res['1'] * 1e3:5.0f} TF)  rel diff {err:.1e}", flush=True)
