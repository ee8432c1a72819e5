"""A launch trace of the training step that runs without a device: what `mindpose_amd/models/train_ops.py` hands to the C ABI, and
the torch ops around it, for whole training steps and for every autograd Function on its own.

The autograd Functions only marshal arguments.  With host tensors that claim to live on the device (``torch.Tensor.is_cuda``), a
null stream and a library whose every export is a recording callable, a whole HRNet-W32 step runs in half a second and leaves
an ordered list of events:

- a library call: ``[name, arg, ...]`` - scalars by value, ``ConvDesc`` (also behind ``byref``) as its field tuple, a pointer as
  ``None`` (null) or ``"p<i>"``, i = the first pointer slot of the SAME call that held this address (so aliasing - ``res1`` being
  ``out`` in the deconv data gradient - is kept, raw addresses are not); structures that carry pointers (``ConvStats``, the
  ``c_void_p`` arrays of the grouped weight gradient, the BatchNorm job arrays) field by field under the same rule;
- a torch op that is neither pure metadata nor an allocation: ``["torch", name]`` at its place in the order (a ``torch.zeros``
  that turns into ``torch.empty`` + ``zero_()``, or disappears, is seen);
- ``empty*`` allocations are only counted.

The fake library answers queries with constants: ``*_bytes`` 1024, ``*_parts`` 4, ``mp_conv_winograd_supported`` 0 (= inside the
form), ``mp_f16_conv_pre_supported`` 1, everything else 0 (= success).

``CASES`` maps a case name to a callable that runs it TWICE in a row on the same parameters (the second run meets the packings
`repack_weights` refreshed); ``trace_case(name)`` returns (events, number of ``empty*`` allocations) with every process-wide cache
of the training path cleared first, so a case traces the same wherever it stands in a run.
"""
import contextlib
import ctypes
import hashlib
import json
import os
from unittest import mock

import torch
from torch.utils._python_dispatch import TorchDispatchMode

import mindpose_amd as mp
from mindpose_amd import _lib
from mindpose_amd.models import train_ops as T
from mindpose_amd.models import tuner

# pure metadata: no kernel behind them
_METADATA = {"detach", "view", "_unsafe_view", "slice", "alias", "select", "as_strided", "expand", "permute", "transpose", "t",
             "unsqueeze", "squeeze", "reshape", "_reshape_alias", "unbind", "split", "lift_fresh", "view_as", "narrow", "unfold",
             "is_contiguous", "is_pinned", "size", "stride", "numel", "dim", "storage_offset", "sym_size", "sym_stride", "sym_numel",
             "is_same_size", "_local_scalar_dense"}
_ALLOCATION = {"empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided"}

_SWITCHES = ["MINDPOSE_FUSE_RESIDUAL", "MINDPOSE_BN_FUSE", "MINDPOSE_DGRAD_PHASES4", "MINDPOSE_BN16_MASK_FROM_Z", "MINDPOSE_BN_FUSE_PARTS",
             "MINDPOSE_WGRAD_GROUP", "MINDPOSE_FAN_OUT", "MINDPOSE_FAN_OUT_ONE_NODE", "MINDPOSE_BN_PRE", "MINDPOSE_BN_PRE_CH",
             "MINDPOSE_BN_PRE_MINHW", "MINDPOSE_WINOGRAD", "MINDPOSE_TUNE_CACHE", "MINDPOSE_F32_SMALL", "MINDPOSE_F16_WS",
             "MINDPOSE_TRAIN_BRANCH_STREAMS", "MINDPOSE_TRAIN_FUSE_STREAMS", "MINDPOSE_TRAIN_CHAIN_MODULES"]


class _Trace:
    def __init__(self):
        self.events, self.empties = [], 0


def _is_pointer_type(tp) -> bool:
    return tp is ctypes.c_void_p


class _Call:
    """Normalises the arguments of ONE library call; pointer slots are numbered in the order they are met."""

    def __init__(self):
        self.slots, self.first = 0, {}

    def pointer(self, value):
        slot, self.slots = self.slots, self.slots + 1
        if isinstance(value, ctypes.c_void_p):
            value = value.value
        if not value:
            return None
        return "p%d" % self.first.setdefault(int(value), slot)

    def struct(self, s):
        return [self.pointer(getattr(s, f)) if _is_pointer_type(tp) else self.value(getattr(s, f)) for f, tp in s._fields_]

    def value(self, a, tp=None):
        if tp is not None and _is_pointer_type(tp):
            return self.pointer(a)
        if a is None:  # a null behind a typed pointer
            self.slots += 1
            return None
        if hasattr(a, "_obj"):  # ctypes.byref(...)
            a = a._obj
        if isinstance(a, ctypes.Structure):
            return self.struct(a)
        if isinstance(a, ctypes.Array):
            if _is_pointer_type(a._type_):
                return [self.pointer(v) for v in a]
            return [self.value(v) for v in a]
        if isinstance(a, ctypes._SimpleCData):
            return a.value
        if isinstance(a, bool):
            return int(a)
        if isinstance(a, (int, float, str)):
            return a
        raise TypeError(f"train trace: no rule for a library argument of type {type(a).__name__}")


def _answer(name: str) -> int:
    if name.endswith("_bytes"):
        return 1024
    if name.endswith("_parts"):
        return 4
    if name == "mp_f16_conv_pre_supported":
        return 1
    return 0  # success / "mp_conv_winograd_supported": inside the form


class _FakeLib:
    """Every export of the C ABI as a recording callable (argument kinds from `_lib._PROTOTYPES`).  ``answers``: name -> a callable
    that takes the call's arguments and gives its return value, for the exports whose constant answer does not fit a case."""

    def __init__(self, trace, answers=None):
        self._trace, self._answers = trace, answers or {}

    def __getattr__(self, name):
        if name not in _lib._PROTOTYPES:
            raise AttributeError(name)
        argtypes = _lib._PROTOTYPES[name][1]

        def call(*args):
            if len(args) != len(argtypes):
                raise TypeError(f"{name}: {len(args)} arguments for {len(argtypes)} parameters")
            c = _Call()
            self._trace.events.append([name] + [c.value(a, tp) for a, tp in zip(args, argtypes)])
            return self._answers[name](*args) if name in self._answers else _answer(name)

        self.__dict__[name] = call
        return call


class _TorchOps(TorchDispatchMode):
    def __init__(self, trace):
        super().__init__()
        self._trace = trace

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.overloadpacket.__name__
        if name in _ALLOCATION:
            self._trace.empties += 1
        elif name not in _METADATA:
            self._trace.events.append(["torch", name])
        return func(*args, **(kwargs or {}))


class _NullStream:
    cuda_stream = 0


def _cold():
    """Every process-wide cache of the training path: a case starts as the first of its process would."""
    T._BN16_WS.clear()
    T._const_cache.clear()
    T._PRE_CAPABLE.clear()
    T._WGRAD_PENDING.clear()
    T._WGRAD_CALLBACK[0] = False
    tuner._TUNE_CACHE.clear()


@contextlib.contextmanager
def recording(env=None, answers=None):
    """The patches under which the training path runs on host tensors; yields the trace being filled."""
    trace = _Trace()
    fake = _FakeLib(trace, answers)
    _cold()
    settings = {k: None for k in _SWITCHES}
    settings.update({"MINDPOSE_AUTOTUNE": "0", "MINDPOSE_WGRAD_EARLY_FLUSH": "0"})
    settings.update(env or {})
    saved = {k: os.environ.get(k) for k in settings}
    try:
        for k, v in settings.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        with mock.patch.object(torch.Tensor, "is_cuda", property(lambda self: True)), \
                mock.patch.object(_lib, "load", lambda: fake), \
                mock.patch.object(_lib, "stream", lambda: 0), \
                mock.patch.object(torch.cuda, "current_stream", lambda device=None: _NullStream()), \
                mock.patch.object(torch.cuda, "device", lambda device=None: contextlib.nullcontext()), \
                _TorchOps(trace):
            yield trace
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _cold()


# ---- whole steps -------------------------------------------------------------------------------------------------------------------

def _direct(params):
    for p in params:
        p.grad = torch.zeros_like(p)
        p._mp_grad_direct = True


def _whole_step(backbone, head, amp, direct=True, env=None, stubs=None, size=64):
    def run():
        net = mp.create_network(backbone, head).train()  # (the trace does not depend on a value: no synthetic initialisation)
        if amp:
            mp.models.auto_mixed_precision(net, "O2")
        nwl = mp.create_network_with_loss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(2, 3, size, size, generator=g)
        target, weight = torch.rand(2, 17, size // 4, size // 4, generator=g), torch.ones(2, 17, 1)
        if direct:
            _direct(net.parameters())
        with recording(env) as trace, contextlib.ExitStack() as stack:
            for name, stub in (stubs or {}).items():
                stack.enter_context(mock.patch.object(T, name, stub))
            for _ in range(2):
                nwl(x, target, weight).backward()
                T.flush_wgrad_jobs()
        return trace
    return run


def _variant_stub(miss):
    """`tune_conv_variant` that takes the Winograd form wherever it is offered and answers ``miss`` elsewhere."""
    def stub(lib, d, x, packed, scale, shift, res1, res2, out, half=False, packed_u=None, stats=None):
        return T.F32_WINOGRAD if packed_u is not None else miss
    return stub


def _tuned(miss):
    return {"autotune_on": lambda: True, "tune_conv_variant": _variant_stub(miss)}


HR = ("hrnet_w32", "hrnet_head")
CASES = {
    "hrnet_fp32": _whole_step(*HR, amp=False),
    "hrnet_fp32_no_direct": _whole_step(*HR, amp=False, direct=False),
    "hrnet_fp32_fuse_residual0": _whole_step(*HR, amp=False, env={"MINDPOSE_FUSE_RESIDUAL": "0"}),
    "hrnet_fp32_winograd": _whole_step(*HR, amp=False, stubs=_tuned(-1)),
    "hrnet_o2": _whole_step(*HR, amp=True),
    "hrnet_o2_no_direct": _whole_step(*HR, amp=True, direct=False),
    "hrnet_o2_bn_fuse0": _whole_step(*HR, amp=True, env={"MINDPOSE_BN_FUSE": "0"}),
    "hrnet_o2_bn_fuse0_fuse_residual0": _whole_step(*HR, amp=True, env={"MINDPOSE_BN_FUSE": "0", "MINDPOSE_FUSE_RESIDUAL": "0"}),
    "hrnet_o2_dgrad_phases4_0": _whole_step(*HR, amp=True, env={"MINDPOSE_DGRAD_PHASES4": "0"}),
    "hrnet_o2_mask_from_z0": _whole_step(*HR, amp=True, env={"MINDPOSE_BN16_MASK_FROM_Z": "0"}),
    # the switch only shows where a BatchNorm backward derives its own mask: the per-cell path, and a chain without backward hand-over
    "hrnet_o2_bn_fuse0_mask_from_z0": _whole_step(*HR, amp=True, env={"MINDPOSE_BN_FUSE": "0", "MINDPOSE_BN16_MASK_FROM_Z": "0"}),
    "hrnet_o2_bn_fuse_parts1_mask_from_z0": _whole_step(*HR, amp=True, env={"MINDPOSE_BN_FUSE_PARTS": "1", "MINDPOSE_BN16_MASK_FROM_Z": "0"}),
    "hrnet_o2_wgrad_group1": _whole_step(*HR, amp=True, env={"MINDPOSE_WGRAD_GROUP": "1"}),
    "hrnet_o2_fan_out0": _whole_step(*HR, amp=True, env={"MINDPOSE_FAN_OUT": "0"}),
    "hrnet_o2_fan_out_one_node0": _whole_step(*HR, amp=True, env={"MINDPOSE_FAN_OUT_ONE_NODE": "0"}),
    "hrnet_o2_bn_pre1": _whole_step(*HR, amp=True, env={"MINDPOSE_BN_PRE": "1"}, stubs=_tuned(0)),
    # at 64 x 64 no conv reaches the 2^26 multiply-accumulates `_pre_capable` asks for; at 128 x 128 the stage-1 blocks do
    "hrnet_o2_bn_pre1_128": _whole_step(*HR, amp=True, env={"MINDPOSE_BN_PRE": "1"}, stubs=_tuned(0), size=128),
    "resnet50_fp32": _whole_step("resnet50", "simple_baseline_head", amp=False),
    "resnet50_o2": _whole_step("resnet50", "simple_baseline_head", amp=True),
}
for _parts in (0, 1, 3, 7, 15):
    CASES[f"hrnet_o2_bn_fuse_parts{_parts}"] = _whole_step(*HR, amp=True, env={"MINDPOSE_BN_FUSE_PARTS": str(_parts)})


# ---- one Function at a time: 2 x 8 -> 16 channels on an 8 x 6 map ----------------------------------------------------------------

def _act(half, c, h=8, w=6, seed=1):
    g = torch.Generator().manual_seed(seed)
    if half:
        return torch.randn(2, (c + 7) // 8, h, w, 8, generator=g).half().requires_grad_()
    return torch.randn(2, c, h, w, generator=g).requires_grad_()


def _param(*shape):
    return torch.nn.Parameter(torch.randn(*shape, generator=torch.Generator().manual_seed(2)))


def _function_case(half, direct, params, body):
    """``body(x..., *params)`` -> output(s); two forward + backward passes, `repack_weights` in front of each as a step has it."""
    def run():
        holder = torch.nn.Module()
        ps = [p() for p in params]
        for i, p in enumerate(ps):
            holder.register_parameter(f"p{i}", p)
        if direct:
            _direct(ps)
        with recording() as trace:
            for _ in range(2):
                T.repack_weights(holder)
                outs = body(half, *ps)
                outs = outs if isinstance(outs, (tuple, list)) else [outs]
                torch.autograd.backward(list(outs), [torch.ones_like(o) for o in outs])
                T.flush_wgrad_jobs()
        return trace
    return run


def _conv_body(k, s, cout=16, bias=False):
    def body(half, w, *b):
        fn = T.Conv16Fn if half else T.Conv2dFn
        return fn.apply(_act(half, 8), w, b[0] if bias else None, s, k // 2)
    params = [lambda: _param(cout, 8, k, k)] + ([lambda: _param(cout)] if bias else [])
    return params, body


def _bn_body(res, relu):
    def body(half, gamma, beta):
        fn = T.BatchNormAct16Fn if half else T.BatchNormActFn
        return fn.apply(_act(half, 16), gamma, beta, _act(half, 16, seed=5) if res else None, torch.zeros(16), torch.ones(16), relu)
    return [lambda: _param(16), lambda: _param(16)], body


def _fuse_body(scales):
    def body(half):
        # on a 16 x 8 map: a term at scale 8 still has a pixel
        return T.fuse_sum(_act(half, 16, 16, 8), [(_act(half, 16, 16 // s, 8 // s, seed=3 + s), s) for s in scales])
    return [], body


def _deconv_body():
    def body(half, w):
        return (T.Deconv16Fn if half else T.DeconvFn).apply(_act(half, 8), w)
    return [lambda: _param(8, 16, 4, 4)], body


def _layout_body():
    def body(half):
        return T.from_c8(T.to_c8(_act(False, 5)), 5)
    return [], body


def _add_function_cases():
    bodies = {}
    for k, s in ((3, 1), (3, 2), (1, 1), (1, 2)):
        bodies[f"conv_k{k}s{s}"] = _conv_body(k, s)
    bodies["conv_k3s1_bias_cout5"] = _conv_body(3, 1, cout=5, bias=True)
    for res in (False, True):
        for relu in (False, True):
            bodies[f"bn_res{int(res)}_relu{int(relu)}"] = _bn_body(res, relu)
    bodies["deconv"] = _deconv_body()
    for name, (params, body) in bodies.items():
        for half in (False, True):
            for direct in (False, True):
                CASES[f"fn_{name}_{'f16' if half else 'f32'}_{'direct' if direct else 'plain'}"] = _function_case(half, direct, params, body)
    for scales in ([1], [1, 2], [2, 4, 8]):
        for half in (False, True):
            CASES[f"fn_fuse_sum_{'_'.join(map(str, scales))}_{'f16' if half else 'f32'}"] = _function_case(half, False, *_fuse_body(scales))
    CASES["fn_to_from_c8_c5"] = _function_case(True, False, *_layout_body())


_add_function_cases()


# ---- the summary the golden file keeps -------------------------------------------------------------------------------------------

def trace_case(name):
    trace = CASES[name]()
    return trace.events, trace.empties


def summarise(events, empties):
    counts = {}
    for e in events:
        key = "torch." + e[1] if e[0] == "torch" else e[0]
        counts[key] = counts.get(key, 0) + 1
    canon = json.dumps(events, sort_keys=True, separators=(",", ":"))
    return {"events": len(events), "counts": dict(sorted(counts.items())), "empty": empties,
            "sha256": hashlib.sha256(canon.encode()).hexdigest()}


def dump_text(events) -> str:
    return "".join(json.dumps(e, separators=(",", ":")) + "\n" for e in events)
