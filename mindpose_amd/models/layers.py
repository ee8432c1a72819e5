"""Parameter holders and the launch-plan builder shared by the backbones and heads.

The modules only OWN parameters (named exactly like the reference's MindSpore cells so a mindpose
checkpoint maps 1:1); all arithmetic happens in ``libmindpose_hip.so``.  A network forward is
recorded once per input shape into a native launch plan (``mp_plan_*``) and replayed by one C call.
Which tile variant / kernel form a recorded conv runs is the tuner's choice (tuner.py).
"""
import ctypes
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .. import _lib
from .act_c8 import ActC8
from .tuner import (BLOCK_ROWS, F16_VARIANTS, F32_SMALL_WIDE, F32_WINOGRAD, _autotune, autotune_on, tune_conv_variant, tuned,
                    winograd_enabled)
from .tuner import _TUNE_MIN_MACS  # noqa: F401 - not used here: tests/test_gpu_bands.py restates `Plan._conv_served` from this module's names

BN_EPS = 1e-5  # mindspore.nn.BatchNorm2d default eps


class Conv2d(nn.Module):
    """Parameter holder for ``mindspore.nn.Conv2d`` (weight [Cout,Cin,k,k], optional bias)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, padding: int = 0,
                 has_bias: bool = False) -> None:
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if has_bias else None


class Conv2dTranspose(nn.Module):
    """Parameter holder for ``mindspore.nn.Conv2dTranspose(k=4, s=2, pad_mode="pad", padding=1)``
    (weight [Cin,Cout,4,4], no bias) - simple_baseline_head.py:80-88."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 4) -> None:
        super().__init__()
        if kernel_size != 4:
            raise ValueError("Invalid deconv_kernel.")  # only the k=4 / padding=1 recipe is implemented natively
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, 4, 4))


class BatchNorm2d(nn.Module):
    """Parameter holder for ``mindspore.nn.BatchNorm2d`` (gamma, beta, moving_mean, moving_variance)."""

    def __init__(self, num_features: int) -> None:
        super().__init__()
        self.num_features = num_features
        self.gamma = nn.Parameter(torch.ones(num_features))
        self.beta = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("moving_mean", torch.zeros(num_features))
        self.register_buffer("moving_variance", torch.ones(num_features))

    def folded(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Eval-mode affine: y = x*scale + shift."""
        scale = self.gamma.detach().float() / torch.sqrt(self.moving_variance.float() + BN_EPS)
        shift = self.beta.detach().float() - self.moving_mean.float() * scale
        return scale.contiguous(), shift.contiguous()



def conv_desc(n, cin, h, w, cout, k, stride, pad_top, pad_left, conv_h, conv_w, out_h, out_w, out_mul=1, out_rep=1, off_y=0, off_x=0,
              relu=False, flags=0):
    """``mp_conv_desc``: a k x k conv of [n, cin, h, w] computing conv_h x conv_w pixels per image, pixel (y, x) stored at
    (out_mul y + off_y, out_mul x + off_x) of the [n, cout, out_h, out_w] output as an out_rep x out_rep block."""
    return _lib.ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=stride, pad_top=pad_top, pad_left=pad_left,
                         conv_h=conv_h, conv_w=conv_w, out_h=out_h, out_w=out_w, out_mul=out_mul, out_rep=out_rep, out_off_y=off_y,
                         out_off_x=off_x, relu=int(relu), flags=flags)


def deconv_phase_desc(n, cin, h, w, cout, py, px, relu, c0=0, cw=None):
    """Phase (py, px) of Conv2dTranspose(k=4, s=2, p=1) on [n, cin, h, w] - a 2x2 stride-1 conv whose output pixel (y, j) lands on
    (2 y + py, 2 j + px) - for the columns j in [c0, c0 + cw) (default: all w of them): ``(start, width_in, ConvDesc)``, the conv
    reading input columns [start, start + width_in) as a tensor of its own (all of them: start 0, width_in w)."""
    cw = w - c0 if cw is None else cw
    first = c0 - (1 - px)  # input column of the first tap
    start, stop = max(first, 0), min(w, first + cw + 1)
    d = conv_desc(n, cin, h, stop - start, cout, 2, 1, 1 - py, max(-first, 0), h, cw, 2 * h, 2 * w, out_mul=2, off_y=py,
                  off_x=2 * c0 + px, relu=relu)
    return start, stop - start, d


def conv_column_bands(n, cin, h, w, cout, k, s, pad, relu, nb):
    """A conv layer [n, cin, h, w] -> cout channels (k x k, stride s, padding pad) as output-column bands of ceil(wo / nb) columns:
    per band ``(start, width_in, ConvDesc)`` - the band reads input columns [start, start + width_in) as a tensor of its own and
    writes output columns [out_off_x, out_off_x + conv_w) of the full [n, cout, ho, wo] output.  Only the first band keeps the left
    padding; the last one is clipped at the input's right edge, where the kernel's bounds check supplies the layer's own zeros."""
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    width = -(-wo // nb)
    bands = []
    for c0 in range(0, wo, width):
        cw = min(width, wo - c0)
        first = c0 * s - pad  # input column of the band's first tap
        start, stop = max(first, 0), min(w, (c0 + cw - 1) * s - pad + k)
        bands.append((start, stop - start, conv_desc(n, cin, h, stop - start, cout, k, s, pad, max(-first, 0), ho, cw, ho, wo,
                                                     off_x=c0, relu=relu)))
    return bands


def deconv_phase_column_bands(n, cin, h, w, cout, py, px, relu, nb):
    """`deconv_phase_desc` as input-column bands of ceil(w / nb) columns: per band ``(start, width_in, ConvDesc)`` as in
    `conv_column_bands`; column j of the band that starts at c0 lands on output column 2 (c0 + j) + px."""
    width = -(-w // nb)
    return [deconv_phase_desc(n, cin, h, w, cout, py, px, relu, c0, min(width, w - c0)) for c0 in range(0, w, width)]


def _macs(d) -> int:
    return d.n * d.conv_h * d.conv_w * d.cout * d.cin * d.kh * d.kw


class Plan:
    """A recorded forward: native ``mp_plan`` + the tensors it points into."""

    def __init__(self, device: torch.device, half: bool = False) -> None:
        self.lib = _lib.load()
        self.device = device
        self.half = half  # amp O2/O3: fp16 matrix-core kernels over channel-blocked fp16 activations
        self.lanes = _lib.env_on("MINDPOSE_PLAN_LANES")
        self.handle = ctypes.c_void_p(self.lib.mp_plan_create())
        if not self.handle:
            raise _lib.MindposeHipError("mp_plan_create failed")
        self.keep: List[torch.Tensor] = []  # every buffer the plan references
        self.input: Optional[torch.Tensor] = None
        self.output: Optional[torch.Tensor] = None
        self.layer_info: List[Dict] = []  # per entry: kind, shapes, MACs (for the roofline report)
        self._packed: Dict[Tuple[int, int, int], torch.Tensor] = {}
        self._folded: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._graph = None
        self._graph_ok = True
        self._runs = 0
        self._marks: List[Tuple[int, object]] = []  # (entry index, lane | "barrier"): the lane structure, for the captured replay
        self._multi = False
        self._lane_streams: List[torch.cuda.Stream] = []

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.mp_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def alloc(self, *shape: int):
        """Activation buffer of the plan's compute type (fp32 NCHW tensor, or ActC8 in fp16 mode)."""
        if self.half:
            t = ActC8(*shape, self.device)
            self.keep.append(t.c8_tensor)
            return t
        return self.alloc_f32(*shape)

    def alloc_f32(self, *shape: int) -> torch.Tensor:
        t = torch.empty(shape, device=self.device, dtype=torch.float32)
        self.keep.append(t)
        return t

    def _alloc_like(self, x, *shape: int):
        """Activation buffer of ``x``'s kind (the kernel family follows the activation, not the plan: the fp32 stem of an fp16 plan)."""
        return self.alloc(*shape) if isinstance(x, ActC8) else self.alloc_f32(*shape)

    def _conv_info(self, kind: str, k: int, stride: int, cin: int, cout: int, h: int, w: int, n: int, macs: int) -> None:
        self.layer_info.append(dict(kind=kind, k=k, stride=stride, cin=cin, cout=cout, h=h, w=w, n=n, macs=macs))

    def to_c8(self, x: torch.Tensor) -> "ActC8":
        """NCHW fp32 -> channel-blocked fp16 (first entry of an fp16 plan)."""
        n, c, h, w = x.shape
        out = self.alloc(n, c, h, w)
        _lib.check(self.lib.mp_plan_add_layout_f16(self.handle, 1, _lib.ptr(x), _lib.ptr(out), n, c, h, w), "mp_plan_add_layout_f16")
        self.layer_info.append(dict(kind="to_c8", n=n, c=c, h=h, w=w, macs=0))
        return out

    def enter(self, x):
        """Switch to the plan's compute type: in an fp16 plan an fp32 NCHW tensor is converted to channel-blocked fp16 here
        (HRNet: the input image; ResNet: after the fp32 7x7 stem and max-pool); otherwise ``x`` is returned unchanged."""
        if self.half and not isinstance(x, ActC8):
            return self.to_c8(x)
        return x

    def from_c8(self, x: "ActC8") -> torch.Tensor:
        """channel-blocked fp16 -> NCHW fp32 (the network output handed to the decoder / loss)."""
        n, c, h, w = x.shape
        out = self.alloc_f32(n, c, h, w)
        _lib.check(self.lib.mp_plan_add_layout_f16(self.handle, 0, _lib.ptr(x), _lib.ptr(out), n, c, h, w), "mp_plan_add_layout_f16")
        self.layer_info.append(dict(kind="from_c8", n=n, c=c, h=h, w=w, macs=0))
        return out

    # -- execution lanes ----------------------------------------------------------------------
    def set_lane(self, lane: int) -> None:
        """Entries recorded from now on replay on execution lane ``lane`` (0 = the caller's stream, 1..3 = side streams of
        the plan): independent sub-graphs overlap on the chip.  No-op when lanes are disabled (MINDPOSE_PLAN_LANES=0)."""
        if self.lanes:
            _lib.check(self.lib.mp_plan_set_lane(self.handle, int(lane) % 4), "mp_plan_set_lane")
            self._marks.append((int(self.lib.mp_plan_size(self.handle)), int(lane) % 4))
            if lane:
                # The native multi-lane replay (plain HIP streams and events inside mp_plan_run, all-to-all waits at a barrier)
                # cannot be captured: ROCm 7.2's capture_end faults on it.  The captured replay is driven from here instead
                # (_replay_lanes): the lanes as torch streams, every barrier a STAR - side lanes join the origin stream and fork
                # from it again - which is the only fork / join shape capture survives here (the captured training step has no
                # other).  Inside a hipGraph a cross-lane dependency costs ~10 us instead of the ~30 us of an event wait between
                # two queues (tools/timeline.sh on the inference plan: 12 barriers per HRNet-W32 forward): O2 inference +10 %, fp32 +2 %.
                # MINDPOSE_PLAN_GRAPH_LANES=0: keep replaying through the native call.
                self._multi = True
                if not _lib.env_on("MINDPOSE_PLAN_GRAPH_LANES"):
                    self._graph_ok = False

    def barrier(self) -> None:
        """Every lane waits for everything recorded so far on every other lane."""
        if self.lanes:
            self._marks.append((int(self.lib.mp_plan_size(self.handle)), "barrier"))
            _lib.check(self.lib.mp_plan_add_barrier(self.handle), "mp_plan_add_barrier")
            self.layer_info.append(dict(kind="barrier", macs=0))

    def run(self) -> None:
        """Replay the recorded forward: as one hipGraph launch once captured (MINDPOSE_HIP_GRAPH=0 disables it),
        otherwise as one native call that issues the launches back to back."""
        if self._graph is not None:
            self._graph.replay()
            return
        _lib.check(self.lib.mp_plan_run(self.handle, _lib.stream()), "mp_plan_run")
        self._runs += 1
        if self._runs == 2 and self._graph_ok and _lib.env_on("MINDPOSE_HIP_GRAPH"):
            self._capture()

    def _capture(self) -> None:
        # the plan has run twice (kernel attributes set, nothing allocates): capture the launch sequence
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                if self._multi:
                    self._replay_lanes()
                else:
                    _lib.check(self.lib.mp_plan_run(self.handle, _lib.stream()), "mp_plan_run (capture)")
            self._graph = graph
        except Exception as exc:  # capture unsupported in this context: keep direct launches (same kernels)
            self._graph_ok = False
            import warnings
            warnings.warn(f"hipGraph capture of the launch plan failed, using direct launches: {exc}")

    def _replay_lanes(self) -> None:
        """The recorded forward with lane l on torch stream l (0 = the current stream): what mp_plan_run does natively, in a
        form stream capture accepts.  Barrier entries become all-to-all wait_stream calls among the lanes in use."""
        cur = torch.cuda.current_stream(self.device)
        lanes_used = sorted({m for _, m in self._marks if m != "barrier"} | {0})
        while len(self._lane_streams) < max(lanes_used):
            self._lane_streams.append(torch.cuda.Stream(device=self.device))
        streams = [cur] + self._lane_streams
        for l in lanes_used[1:]:
            streams[l].wait_stream(cur)
        pos, lane = 0, 0
        for idx, what in self._marks + [(len(self), None)]:
            if idx > pos:
                with torch.cuda.stream(streams[lane]):
                    _lib.check(self.lib.mp_plan_run_range(self.handle, pos, idx - pos, _lib.stream()), "mp_plan_run_range")
                pos = idx
            if what == "barrier":
                pos = idx + 1  # the barrier entry itself launches nothing
                # star-shaped: every side lane joins the origin stream, then forks from it again.  Side-to-side waits (a stream
                # joining another FORKED stream) make ROCm 7.2's capture_end fault - the training step's captures never have them
                for l in lanes_used[1:]:
                    cur.wait_stream(streams[l])
                for l in lanes_used[1:]:
                    streams[l].wait_stream(cur)
            elif what is not None:
                lane = what
        for l in lanes_used[1:]:
            cur.wait_stream(streams[l])

    def run_range(self, first: int, count: int) -> None:
        _lib.check(self.lib.mp_plan_run_range(self.handle, first, count, _lib.stream()), "mp_plan_run_range")

    def entry_info(self, index: int) -> Dict[str, int]:
        """Launch geometry the native side chose for entry ``index`` (+ the python-side shape record)."""
        buf = (ctypes.c_int64 * 12)()
        _lib.check(self.lib.mp_plan_entry_info(self.handle, index, buf), "mp_plan_entry_info")
        keys = ["kind_id", "ks", "stride", "variant", "workgroups", "lds_bytes", "cout_tile", "pixel_tile", "cin_chunk",
                "images_per_tile", "rows_per_tile", "light"]
        info = dict(zip(keys, [int(v) for v in buf]))
        info.update(self.layer_info[index])
        return info

    def __len__(self) -> int:
        return int(self.lib.mp_plan_size(self.handle))

    @property
    def total_macs(self) -> int:
        return sum(e.get("macs", 0) for e in self.layer_info)

    # -- weights ------------------------------------------------------------------------------
    def _pack(self, weight: torch.Tensor, cout: int, cin: int, k: int, transposed: bool, py: int, px: int,
              half: bool = False) -> torch.Tensor:
        key = (id(weight), py if transposed else -1, px if transposed else -1, half)
        if key in self._packed:
            return self._packed[key]
        w = weight.detach().to(self.device, torch.float32).contiguous()
        if half:
            nbytes, pack, dtype = self.lib.mp_f16_packed_weight_bytes(cout, cin, k, k), self.lib.mp_f16_pack_weight, torch.float16
        else:
            nbytes, pack, dtype = self.lib.mp_conv_packed_weight_bytes(cout, cin, k, k), self.lib.mp_conv_pack_weight, torch.float32
        packed = torch.empty(nbytes // (2 if half else 4), device=self.device, dtype=dtype)
        _lib.check(pack(_lib.ptr(w), _lib.ptr(packed), cout, cin, k, k, int(transposed), py, px, _lib.stream()),
                   "mp_f16_pack_weight" if half else "mp_conv_pack_weight")
        self.keep += [w, packed]
        self._packed[key] = packed
        return packed

    def _pack_winograd(self, weight: torch.Tensor, cout: int, cin: int) -> torch.Tensor:
        """U = G w G^T of a 3x3 weight, [Cin_pad4][Cout_pad16][16] fp32 (mp_conv_winograd_pack_weight)."""
        key = (id(weight), "wino")
        if key in self._packed:
            return self._packed[key]
        w = weight.detach().to(self.device, torch.float32).contiguous()
        packed = torch.empty(self.lib.mp_conv_winograd_packed_weight_bytes(cout, cin) // 4, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.mp_conv_winograd_pack_weight(_lib.ptr(w), _lib.ptr(packed), cout, cin, _lib.stream()),
                   "mp_conv_winograd_pack_weight")
        self.keep += [w, packed]
        self._packed[key] = packed
        return packed

    def _affine(self, cout: int, bn: Optional[BatchNorm2d], bias: Optional[torch.Tensor], half: bool = False):
        # keyed on both parameter holders and the width: a conv with neither BatchNorm nor bias must not share the
        # ones / zeros pair of another width (the kernel reads cout entries)
        key = (id(bn) if bn is not None else None, id(bias) if bias is not None else None, cout, half)
        if key in self._folded:
            return self._folded[key]
        if bn is not None:
            scale, shift = bn.folded()
            scale, shift = scale.to(self.device), shift.to(self.device)
        else:
            scale = torch.ones(cout, device=self.device)
            shift = bias.detach().float().to(self.device).contiguous() if bias is not None else torch.zeros(cout, device=self.device)
        if half:  # the fp16 kernel reads 4 couts per lane: arrays padded to Cout_pad16 with zeros
            pad = (-cout) % 16
            scale = torch.cat([scale, scale.new_zeros(pad)]).contiguous()
            shift = torch.cat([shift, shift.new_zeros(pad)]).contiguous()
        self.keep += [scale, shift]
        self._folded[key] = (scale, shift)
        return scale, shift

    # -- ops ----------------------------------------------------------------------------------
    def conv(self, x: torch.Tensor, conv: Conv2d, bn: Optional[BatchNorm2d] = None, relu: bool = False,
             res1: Optional[torch.Tensor] = None, res2: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, upsample: int = 1) -> torch.Tensor:
        """conv (+BN or bias) (+res1) (+res2) (+ReLU); ``upsample`` = nearest factor applied while storing
        (``out`` / ``res*`` then live at the up-sampled resolution).  A layer no kernel serves at its full width is recorded as
        output-column bands (`_conv_by_columns`)."""
        n, cin, h, w = x.shape
        k, s, pad, cout = conv.kernel_size, conv.stride, conv.padding, conv.out_channels
        if cin != conv.in_channels:
            raise ValueError(f"conv expects {conv.in_channels} input channels, got {cin}")
        half = isinstance(x, ActC8)  # the kernel family follows the activation: fp32 NCHW tensors take the fp32 kernels
        if half and upsample != 1:
            raise NotImplementedError("fp16 plans add up-sampled terms with fuse_sum, not through the conv epilogue")
        ho = (h + 2 * pad - k) // s + 1
        wo = (w + 2 * pad - k) // s + 1
        d = conv_desc(n, cin, h, w, cout, k, s, pad, pad, ho, wo, ho * upsample, wo * upsample, upsample, upsample, relu=relu)
        if upsample == 1 and not self._conv_served(d, half, int(res1 is not None) + int(res2 is not None)):
            return self._conv_by_columns(x, conv, bn, relu, res1, res2, out)
        out = self._conv_out(x, d, res1, res2, out)
        return self._record_conv(d, x, self._pack(conv.weight, cout, cin, k, False, 0, 0, half), *self._affine(cout, bn, conv.bias, half),
                                 res1, res2, out, "conv_f16" if half else "conv", packed_u=self._winograd_weight(d, conv, half))

    def _conv_out(self, x, d, res1, res2, out):
        """The [n, cout, out_h, out_w] output of ``d``: the caller's ``out`` (checked, with the residuals), else a new buffer."""
        shape = (d.n, d.cout, d.out_h, d.out_w)
        if out is None:
            out = self._alloc_like(x, *shape)
        if tuple(out.shape) != shape:
            raise ValueError(f"bad out shape {tuple(out.shape)}")
        for r in (res1, res2):
            if r is not None and tuple(r.shape) != shape:
                raise ValueError(f"residual shape {tuple(r.shape)} != out shape {shape}")
        return out

    def _winograd_weight(self, d, conv: Conv2d, half: bool):
        """The Winograd form of ``conv``'s weight where it competes in the tuner for ``d`` (fp32, 3x3 stride 1), else None.  Asks
        for the tuner's switch only, not `tuned(macs)`: a small layer's tuner key carries the form too (its pick is then -1)."""
        if half or not (winograd_enabled() and autotune_on()) or self.lib.mp_conv_winograd_supported(ctypes.byref(d)) != 0:
            return None
        return self._pack_winograd(conv.weight, conv.out_channels, conv.in_channels)

    def _record_conv(self, d, x, packed, scale, shift, res1, res2, out, kind: str, packed_u=None, variant: Optional[int] = None):
        """THE place where a conv becomes a plan entry: the tuner picks the variant of ``d`` on the operand buffers (unless the
        caller already holds the pick), the entry is added in that form - ``packed_u``: the Winograd weight (fp32), which then
        competes - and its `layer_info` record follows (what ``d`` describes: a band reports the band).  Returns ``out``."""
        half = isinstance(x, ActC8)
        if variant is None:
            variant = tune_conv_variant(self.lib, d, x, packed, scale, shift, res1, res2, out, half=half, packed_u=packed_u)
        operands = [_lib.ptr(t) for t in (scale, shift, res1, res2, out)]
        if not half and variant == F32_WINOGRAD:
            kind = "conv_winograd"
            _lib.check(self.lib.mp_plan_add_conv_winograd(self.handle, ctypes.byref(d), _lib.ptr(x), _lib.ptr(packed_u), *operands),
                       "mp_plan_add_conv_winograd")
        else:
            add = self.lib.mp_plan_add_conv_f16 if half else self.lib.mp_plan_add_conv_variant
            _lib.check(add(self.handle, ctypes.byref(d), variant, _lib.ptr(x), _lib.ptr(packed), *operands), f"mp_plan_add_conv ({kind})")
        self._conv_info(kind, d.kh, d.stride, d.cin, d.cout, d.h, d.w, d.n, _macs(d))
        return out

    def _conv_served(self, d, half: bool, n_res: int) -> bool:
        """Does any kernel form (the library heuristic, a tile variant the tuner could pick, the Winograd form) take this conv?
        Forced variants count only where the tuner picks one: with ``MINDPOSE_AUTOTUNE=0``, or below its MAC threshold, the entry
        is recorded with the heuristic, which then has to take the layer itself (else: column bands)."""
        picks = tuned(_macs(d))
        if half:
            return any(self.lib.mp_f16_conv_supported(ctypes.byref(d), v, n_res, 0) == 1 for v in range(-1, F16_VARIANTS if picks else 0))
        if any(self.lib.mp_conv_supported(ctypes.byref(d), v) == 1 for v in range(-1, F32_SMALL_WIDE + 1 if picks else 0)):
            return True
        return picks and winograd_enabled() and self.lib.mp_conv_winograd_supported(ctypes.byref(d)) == 0

    def _fewest_bands(self, bands_of, half: bool, n_res: int, what: str):
        """``bands_of(nb)`` for the smallest nb in 2..32 whose every band some kernel serves."""
        for nb in range(2, 33):
            bands = bands_of(nb)
            if all(self._conv_served(d, half, n_res) for _, _, d in bands):
                return bands
        raise _lib.MindposeHipError(f"no kernel serves the {what}, not even in column bands")

    def col_slice(self, x, start: int, width: int):
        """Columns [start, start + width) of an activation of the plan's layout, as a new buffer (mp_plan_add_col_slice)."""
        n, c, h, w = x.shape
        half = isinstance(x, ActC8)
        out = self._alloc_like(x, n, c, h, width)
        rows = n * ((c + 7) // 8 if half else c) * h
        _lib.check(self.lib.mp_plan_add_col_slice(self.handle, _lib.ptr(x), _lib.ptr(out), rows, w, start, width, int(half)),
                   "mp_plan_add_col_slice")
        self.layer_info.append(dict(kind="col_slice", n=n, c=c, h=h, w=width, macs=0))
        return out

    def _conv_by_columns(self, x, conv: Conv2d, bn, relu, res1, res2, out):
        """A conv too wide for every kernel (the first convs of HRNet on 512 / 832-pixel images, the full-resolution layers of the
        HigherHRNet head): the fewest equal output-column bands that every band's kernel takes.  Each band copies its input
        columns (plus the kernel's reach) into a buffer of its own and writes its output columns in place (out_off_x); a band's
        arithmetic is the full layer's, per output pixel."""
        n, cin, h, w = x.shape
        k, s, pad, cout = conv.kernel_size, conv.stride, conv.padding, conv.out_channels
        half = isinstance(x, ActC8)
        bands = self._fewest_bands(lambda nb: conv_column_bands(n, cin, h, w, cout, k, s, pad, relu, nb), half,
                                   int(res1 is not None) + int(res2 is not None),
                                   f"conv {tuple(x.shape)} -> {cout} channels (k {k}, stride {s})")
        out = self._conv_out(x, bands[0][2], res1, res2, out)
        packed = self._pack(conv.weight, cout, cin, k, False, 0, 0, half)
        scale, shift = self._affine(cout, bn, conv.bias, half)
        for start, wb, d in bands:
            self._record_conv(d, self.col_slice(x, start, wb), packed, scale, shift, res1, res2, out, "conv_f16" if half else "conv",
                              packed_u=self._winograd_weight(d, conv, half))
        return out

    def fuses_basic_block(self, x: torch.Tensor, conv1: Conv2d, conv2: Conv2d) -> bool:
        """The fused fp16 BasicBlock kernels cover the 32-channel branch (four 8-channel blocks) and, round 4, the 64-channel branch
        and 128-channel branches (3x3 stride 1 both convs; the library says whether the map fits a band: ``mp_f16_basicblock_supported``);
        ``MINDPOSE_FUSE_BLOCK=0`` keeps the two-launch path, ``MINDPOSE_FUSE_BLOCK64=0`` for the 64 / 128-channel blocks only."""
        if not isinstance(x, ActC8) or not _lib.env_on("MINDPOSE_FUSE_BLOCK"):
            return False
        n, c, h, w = x.shape
        if not all(cv.in_channels == c and cv.out_channels == c and cv.kernel_size == 3 and cv.stride == 1 and cv.padding == 1
                   and cv.bias is None for cv in (conv1, conv2)):
            return False
        if c in (64, 128) and not _lib.env_on("MINDPOSE_FUSE_BLOCK64"):
            return False
        return (24 < c <= 32 or c in (64, 128)) and self.lib.mp_f16_basicblock_supported(n, c, h, w) == 1

    def basic_block(self, x: torch.Tensor, conv1: Conv2d, bn1: BatchNorm2d, conv2: Conv2d, bn2: BatchNorm2d) -> torch.Tensor:
        """relu(bn2(conv2(relu(bn1(conv1 x)))) + x) in ONE launch (mp_f16_basicblock_fwd): the intermediate tensor stays in LDS;
        bit-identical to the two conv launches."""
        n, c, h, w = x.shape
        out = self.alloc(n, c, h, w)
        p1, p2 = (self._pack(cv.weight, c, c, 3, False, 0, 0, True) for cv in (conv1, conv2))
        (s1, b1), (s2, b2) = self._affine(c, bn1, None, True), self._affine(c, bn2, None, True)
        # rows per workgroup band: 0 = the tallest band that fits (fewest halo rows: right when N x bands fills the chip); a handful
        # of crops leaves 2 - 8 workgroups per launch, and shorter bands trade recomputed halo rows for parallelism - timed per shape
        stream = _lib.stream()

        def launch(v):
            return self.lib.mp_f16_basicblock_fwd(_lib.ptr(x), _lib.ptr(p1), _lib.ptr(s1), _lib.ptr(b1), _lib.ptr(p2), _lib.ptr(s2), _lib.ptr(b2),
                                                  _lib.ptr(out), n, c, h, w, BLOCK_ROWS[v], stream)
        pick = _autotune(("basicblock_f16", n, c, h, w, str(out.device)), 2 * n * h * w * c * c * 9, len(BLOCK_ROWS), launch)
        rows = BLOCK_ROWS[pick] if pick >= 0 else 0
        _lib.check(self.lib.mp_plan_add_basicblock_f16(self.handle, _lib.ptr(x), _lib.ptr(p1), _lib.ptr(s1), _lib.ptr(b1),
                                                       _lib.ptr(p2), _lib.ptr(s2), _lib.ptr(b2), _lib.ptr(out), n, c, h, w, rows),
                   "mp_plan_add_basicblock_f16")
        self._conv_info("basicblock_f16", 3, 1, c, c, h, w, n, 2 * n * h * w * c * c * 9)
        return out

    def fuses_dual_pw(self, x: torch.Tensor, conv_a: Conv2d, conv_b: Conv2d) -> bool:
        """Two 1x1 convs on ONE 64-channel input as one launch (mp_f16_dual_pw_fwd): the down-sample conv (64 -> 256) and the reduce conv
        (64 -> 64) of stage 1's first Bottleneck.  fp16 plans, stride 1, no bias, pixel count a multiple of 64; switched with the chain
        launch (``MINDPOSE_FUSE_PWCHAIN``)."""
        if not isinstance(x, ActC8) or not _lib.env_on("MINDPOSE_FUSE_PWCHAIN"):
            return False
        return x.shape[1] == 64 and self._pw(conv_a, 64, 256) and self._pw(conv_b, 64, 64) and self._chain_fits(x, True)

    def dual_pw(self, x: torch.Tensor, conv_a: Conv2d, bn_a: BatchNorm2d, relu_a: bool, conv_b: Conv2d, bn_b: BatchNorm2d,
                relu_b: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        """(act_a(bn_a(conv_a x)), act_b(bn_b(conv_b x))) in one launch, x read once; bit-identical to the two conv launches."""
        n, c, h, w = x.shape
        ya, zb = self.alloc(n, conv_a.out_channels, h, w), self.alloc(n, conv_b.out_channels, h, w)
        pa = self._pack(conv_a.weight, conv_a.out_channels, c, 1, False, 0, 0, True)
        pb = self._pack(conv_b.weight, conv_b.out_channels, c, 1, False, 0, 0, True)
        (sa, ba), (sb, bb) = self._affine(conv_a.out_channels, bn_a, None, True), self._affine(conv_b.out_channels, bn_b, None, True)
        _lib.check(self.lib.mp_plan_add_dual_pw_f16(self.handle, _lib.ptr(x), _lib.ptr(pa), _lib.ptr(sa), _lib.ptr(ba), int(relu_a), _lib.ptr(pb),
                                                    _lib.ptr(sb), _lib.ptr(bb), int(relu_b), _lib.ptr(ya), _lib.ptr(zb), n, c,
                                                    conv_a.out_channels, conv_b.out_channels, h, w), "mp_plan_add_dual_pw_f16")
        self._conv_info("pwchain_f16", 1, 1, c, conv_a.out_channels, h, w, n, n * h * w * c * (conv_a.out_channels + conv_b.out_channels))
        return ya, zb

    def fuses_stem(self, x: torch.Tensor, conv: Conv2d) -> bool:
        """Can the first conv run as the dedicated streaming kernel with (tap, channel) as its k axis?  fp16 plans: mp_f16_stem_conv_fwd
        reads the fp32 NCHW image itself (no layout pass, the 27 real k positions of a 3-channel 3x3 conv in ONE k-step); fp32 plans:
        mp_stem_conv_fwd (seven k-steps of 4).  ``MINDPOSE_FUSE_STEM=0`` keeps (layout pass +) the general conv."""
        if isinstance(x, ActC8) or not _lib.env_on("MINDPOSE_FUSE_STEM"):
            return False
        n, c, h, w = x.shape
        lds = (6 if self.half else 12) * (w + 4) * 17 + 16  # the 17 staged rows of the three planes (fp16 / fp32)
        return (c == 3 and conv.in_channels == 3 and conv.out_channels == 64 and conv.kernel_size == 3 and conv.stride == 2
                and conv.padding == 1 and conv.bias is None and h % 2 == 0 and w % 32 == 0 and x.dtype == torch.float32
                and lds <= 64 * 1024 and n * 8 * (h // 2) * (w // 2) * 16 < 0x7FFFFFF0)

    def stem(self, x: torch.Tensor, conv: Conv2d, bn: BatchNorm2d):
        """relu(bn(conv x)) of the network's first conv (hrnet.py:377-385) in one launch of the dedicated kernel: fp16 plans - from the
        fp32 image to the channel-blocked fp16 activation; fp32 plans - NCHW to NCHW."""
        n, _, h, w = x.shape
        wt = conv.weight.detach().to(self.device, torch.float32).contiguous()
        self.keep.append(wt)
        # one argument list for both kernels; fp32 plans: the same (tap, channel) k axis on the fp32 matrix cores, NCHW in and out
        out = self.alloc(n, 64, h // 2, w // 2)
        scale, shift = self._affine(64, bn, None, self.half)
        add = self.lib.mp_plan_add_stem_conv_f16 if self.half else self.lib.mp_plan_add_stem_conv
        _lib.check(add(self.handle, _lib.ptr(x), _lib.ptr(wt), _lib.ptr(scale), _lib.ptr(shift), 1, _lib.ptr(out), n, h, w),
                   "mp_plan_add_stem_conv_f16" if self.half else "mp_plan_add_stem_conv")
        self._conv_info("stem_f16" if self.half else "stem_f32", 3, 2, 3, 64, h, w, n, n * (h // 2) * (w // 2) * 64 * 27)
        return out

    def fuses_expand_reduce(self, mid: torch.Tensor, res: torch.Tensor, conv3: Conv2d, conv1_next: Conv2d) -> bool:
        """Can the expand conv of a Bottleneck and the reduce conv of the next one run as ONE launch (fp16 plans:
        mp_f16_expand_reduce_fwd, bit-identical to the two launches; fp32 plans: mp_expand_reduce_fwd, the persistent weight-stationary
        form - same values up to the association of the k sums)?  The 64 -> 256 -> 64 widths of HRNet's stage 1, 1x1 stride-1 convs
        without bias, maps whose pixel count is a multiple of 64.  ``MINDPOSE_FUSE_PWCHAIN=0`` (fp16) / ``MINDPOSE_FUSE_PWCHAIN32=0``
        (fp32) keep the two launches."""
        half = isinstance(mid, ActC8)
        if half != isinstance(res, ActC8) or not _lib.env_on("MINDPOSE_FUSE_PWCHAIN" if half else "MINDPOSE_FUSE_PWCHAIN32"):
            return False
        n, cm, h, w = mid.shape
        return (cm == 64 and tuple(res.shape) == (n, 256, h, w) and self._pw(conv3, 64, 256) and self._pw(conv1_next, 256, 64)
                and self._chain_fits(mid, half))

    @staticmethod
    def _pw(cv: Conv2d, ci: int, co: int) -> bool:
        """A 1x1 stride-1 conv ci -> co without bias?"""
        return (cv.in_channels == ci and cv.out_channels == co and cv.kernel_size == 1 and cv.stride == 1 and cv.padding == 0
                and cv.bias is None)

    @staticmethod
    def _chain_fits(x, half: bool) -> bool:
        """Does the map of ``x`` fit the 64 -> 256 (-> 64) chain kernels: a multiple of 64 pixels, and the byte offsets of the
        256-channel tensor - fp16: 32 channel blocks of 16 bytes a pixel, fp32: 256 planes of 4 bytes - within 31 bits?"""
        n, _, h, w = x.shape
        return (h * w) % 64 == 0 and (n * 32 * h * w * 16 if half else n * 256 * h * w * 4) < 0x7FFFFFF0

    def fuses_ds_expand_reduce(self, x0: torch.Tensor, ds_conv: Conv2d, conv3: Conv2d, conv1_next: Conv2d) -> bool:
        """Can the FIRST Bottleneck's down-sample conv (hrnet.py:74-81, 64 -> 256 on the block's input) be computed inside the expand +
        reduce chain launch, instead of being written and read back as the residual tensor by a launch of its own?
        ``MINDPOSE_FUSE_PWCHAIN32_DS=0`` (fp32) / ``MINDPOSE_FUSE_PWCHAIN_DS=0`` (fp16: the dual 1x1 launch + the identity chain instead)
        keep the separate launch."""
        half = isinstance(x0, ActC8)
        switch = "MINDPOSE_FUSE_PWCHAIN" if half else "MINDPOSE_FUSE_PWCHAIN32"
        if not (_lib.env_on(switch) and _lib.env_on(switch + "_DS")):
            return False
        return (x0.shape[1] == 64 and self._pw(ds_conv, 64, 256) and self._pw(conv3, 64, 256) and self._pw(conv1_next, 256, 64)
                and self._chain_fits(x0, half))

    def fuses_expand_only(self, mid: torch.Tensor, res: torch.Tensor, conv3: Conv2d) -> bool:
        """fp32 plans: the LAST Bottleneck's expand conv + identity through the persistent weight-stationary kernel (no reduce conv
        follows).  ``MINDPOSE_FUSE_PWCHAIN32_LAST=0`` keeps the tuned general conv."""
        if isinstance(mid, ActC8) or isinstance(res, ActC8):
            return False
        if not (_lib.env_on("MINDPOSE_FUSE_PWCHAIN32") and _lib.env_on("MINDPOSE_FUSE_PWCHAIN32_LAST")):
            return False
        n, cm, h, w = mid.shape
        return cm == 64 and tuple(res.shape) == (n, 256, h, w) and self._pw(conv3, 64, 256) and self._chain_fits(mid, False)

    def expand_reduce(self, mid: torch.Tensor, res: Optional[torch.Tensor], conv3: Conv2d, bn3: BatchNorm2d, conv1_next: Optional[Conv2d],
                      bn1_next: Optional[BatchNorm2d], ds=None):
        """(y, z) = (relu(bn3(conv3 mid) + res), relu(bn1'(conv1' y))) in one launch: y never comes back from HBM for the second conv
        (hrnet.py:107-146).  fp16: bit-identical to the two conv launches; fp32: equal up to the association of the k sums.
        fp32 only: ``ds = (x0, conv, bn)`` - the residual is the block's down-sample conv of its input x0, computed in the launch
        (``res`` None); ``conv1_next`` None - the expand conv alone, returns y."""
        n, cm, h, w = mid.shape
        ce = conv3.out_channels
        cr = conv1_next.out_channels if conv1_next is not None else 0
        half = isinstance(mid, ActC8)
        if half and conv1_next is None:
            raise NotImplementedError("the expand conv alone is an fp32 form")
        x0, ds_conv, ds_bn = ds if ds is not None else (None, None, None)

        def operands(cv, bn, co, ci):  # (packed weight, scale, shift) pointers of one 1x1 conv of the chain; NULLs when it is absent
            if cv is None:
                return [None, None, None]
            return [_lib.ptr(t) for t in (self._pack(cv.weight, co, ci, 1, False, 0, 0, half), *self._affine(co, bn, None, half))]

        y = self._alloc_like(mid, n, ce, h, w)
        z = self._alloc_like(mid, n, cr, h, w) if conv1_next is not None else None
        expand, reduce, down = operands(conv3, bn3, ce, cm), operands(conv1_next, bn1_next, cr, ce), operands(ds_conv, ds_bn, ce, cm)
        if not half:
            _lib.check(self.lib.mp_plan_add_expand_reduce(self.handle, _lib.ptr(mid), _lib.ptr(res), _lib.ptr(x0), *down, *expand, *reduce,
                                                          _lib.ptr(y), _lib.ptr(z), n, cm, ce, cr if cr else 64, h, w),
                       "mp_plan_add_expand_reduce")
        elif ds is not None:
            _lib.check(self.lib.mp_plan_add_ds_expand_reduce_f16(self.handle, _lib.ptr(mid), _lib.ptr(x0), *down, *expand, 1, *reduce, 1,
                                                                 _lib.ptr(y), _lib.ptr(z), n, cm, ce, cr, h, w),
                       "mp_plan_add_ds_expand_reduce_f16")
        else:
            _lib.check(self.lib.mp_plan_add_expand_reduce_f16(self.handle, _lib.ptr(mid), _lib.ptr(res), *expand, 1, *reduce, 1,
                                                              _lib.ptr(y), _lib.ptr(z), n, cm, ce, cr, h, w),
                       "mp_plan_add_expand_reduce_f16")
        self._conv_info("pwchain_f16" if half else "pwchain_f32", 1, 1, cm, ce, h, w, n,
                        n * h * w * (cm * ce + ce * cr + (cm * ce if ds is not None else 0)))
        return (y, z) if conv1_next is not None else y

    def deconv4x4s2(self, x: torch.Tensor, deconv: Conv2dTranspose, bn: BatchNorm2d, relu: bool = True) -> torch.Tensor:
        """Conv2dTranspose(k=4, s=2, p=1) + BN + ReLU as four 2x2 sub-pixel phase convolutions - four launches with a tuned form each,
        or (fp32, where the tuner finds it faster: the small maps of the head) all four phases in ONE launch of the blocked-GEMM
        kernel (mp_plan_add_deconv4x4s2_gemm)."""
        half = isinstance(x, ActC8)
        n, cin, h, w = x.shape
        cout = deconv.out_channels
        out = self._alloc_like(x, n, cout, 2 * h, 2 * w)
        scale, shift = self._affine(cout, bn, None, half)
        phases = [(py, px) for py in (0, 1) for px in (0, 1)]
        descs = [deconv_phase_desc(n, cin, h, w, cout, py, px, relu)[2] for py, px in phases]
        if not all(self._conv_served(d, half, 0) for d in descs):
            return self._deconv_by_columns(x, deconv, out, scale, shift, relu)
        kind = "deconv_phase_f16" if half else "deconv_phase"
        if half:
            for d, (py, px) in zip(descs, phases):
                self._record_conv(d, x, self._pack(deconv.weight, cout, cin, 2, True, py, px, True), scale, shift, None, None, out, kind)
            return out
        # fp32: the four phase packings back to back in one buffer (the one-launch form reads them as slices)
        key = (id(deconv.weight), "deconv4")
        if key not in self._packed:
            wsrc = deconv.weight.detach().to(self.device, torch.float32).contiguous()
            per = self.lib.mp_conv_packed_weight_bytes(cout, cin, 2, 2) // 4
            buf = torch.empty(4 * per, device=self.device, dtype=torch.float32)
            for i, (py, px) in enumerate(phases):
                _lib.check(self.lib.mp_conv_pack_weight(_lib.ptr(wsrc), _lib.ptr(buf[i * per:(i + 1) * per]), cout, cin, 2, 2, 1, py, px,
                                                        _lib.stream()), "mp_conv_pack_weight(deconv phase)")
            self.keep += [wsrc, buf]
            self._packed[key] = buf
        buf = self._packed[key]
        per = buf.numel() // 4
        slices = [buf[i * per:(i + 1) * per] for i in range(4)]
        # the four picks come first: the one-launch form is timed against the four launches in THEIR tuned forms
        variants = [tune_conv_variant(self.lib, d, x, pk, scale, shift, None, None, out) for d, pk in zip(descs, slices)]
        fused = False
        # the tuner's switch only, not `tuned(macs)`: below the threshold `_autotune` records its -1 under the key all the same
        if autotune_on() and self.lib.mp_deconv4x4s2_gemm_supported(ctypes.byref(descs[0])) == 0:
            stream = _lib.stream()

            def launch(form):
                if form == 1:
                    return self.lib.mp_deconv4x4s2_gemm_fwd(ctypes.byref(descs[0]), _lib.ptr(x), _lib.ptr(buf), _lib.ptr(scale),
                                                            _lib.ptr(shift), _lib.ptr(out), stream)
                rc = 0
                for d, pk, v in zip(descs, slices, variants):
                    rc = rc or self.lib.mp_conv2d_fwd_variant(ctypes.byref(d), v, _lib.ptr(x), _lib.ptr(pk), _lib.ptr(scale),
                                                              _lib.ptr(shift), None, None, _lib.ptr(out), stream)
                return rc

            tkey = ("deconv4x4s2",) + tuple(getattr(descs[0], f) for f, _ in descs[0]._fields_) + (str(out.device),)
            fused = _autotune(tkey, 4 * _macs(descs[0]), 2, launch) == 1
        if fused:
            _lib.check(self.lib.mp_plan_add_deconv4x4s2_gemm(self.handle, ctypes.byref(descs[0]), _lib.ptr(x), _lib.ptr(buf),
                                                             _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(out)),
                       "mp_plan_add_deconv4x4s2_gemm")
            self._conv_info("deconv_gemm", 2, 1, cin, cout, h, w, n, 4 * _macs(descs[0]))
            return out
        for d, pk, v in zip(descs, slices, variants):
            self._record_conv(d, x, pk, scale, shift, None, None, out, kind, variant=v)
        return out

    def _deconv_by_columns(self, x, deconv: Conv2dTranspose, out, scale, shift, relu: bool):
        """`deconv4x4s2` on a map too wide for every phase kernel (the HigherHRNet head on 832-pixel images): each 2x2 phase conv
        in the fewest input-column bands every band's kernel takes (`_conv_by_columns`; phase px of band column j lands on output
        column 2 j + px)."""
        half = isinstance(x, ActC8)
        n, cin, h, w = x.shape
        cout = deconv.out_channels
        for py, px in [(py, px) for py in (0, 1) for px in (0, 1)]:
            packed = self._pack(deconv.weight, cout, cin, 2, True, py, px, half)
            bands = self._fewest_bands(lambda nb: deconv_phase_column_bands(n, cin, h, w, cout, py, px, relu, nb), half, 0,
                                       f"transposed conv {tuple(x.shape)} -> {cout} channels (k 4, stride 2)")
            for start, wb, d in bands:
                self._record_conv(d, self.col_slice(x, start, wb), packed, scale, shift, None, None, out,
                                  "deconv_phase_f16" if half else "deconv_phase")
        return out

    def fuse_sum(self, base: torch.Tensor, terms, out: torch.Tensor, relu: bool = True) -> torch.Tensor:
        """out = act(((base + up(t1)) + up(t2)) + up(t3)); ``terms`` = [(low-res tensor, integer scale), ...] (1-3)."""
        n, c, h, w = base.shape
        if not 1 <= len(terms) <= 3:
            raise ValueError("fuse_sum takes 1 to 3 up-sampled terms")
        args = []
        for t, sc in list(terms) + [(None, 1)] * (3 - len(terms)):
            if t is not None and tuple(t.shape) != (n, c, h // sc, w // sc):
                raise ValueError(f"fuse term shape {tuple(t.shape)} does not match {(n, c, h // sc, w // sc)}")
            args += [_lib.ptr(t), int(sc)]
        add = self.lib.mp_plan_add_fuse_sum_f16 if isinstance(base, ActC8) else self.lib.mp_plan_add_fuse_sum
        _lib.check(add(self.handle, _lib.ptr(base), *args, _lib.ptr(out), n, c, h, w, int(relu)), "mp_plan_add_fuse_sum")
        self.layer_info.append(dict(kind="fuse_sum", n=n, c=c, h=h, w=w, terms=len(terms), macs=0))
        return out

    def concat(self, a, b):
        """``ops.concat((a, b), 1)`` of two activations of the plan's layout into a new buffer (mp_plan_add_concat): fp32 NCHW, or
        channel-blocked fp16 when ``a`` has a multiple of 8 channels (one block copy per image)."""
        n, ca, h, w = a.shape
        cb = b.shape[1]
        half = isinstance(a, ActC8)
        if half != isinstance(b, ActC8) or tuple(b.shape) != (n, cb, h, w):
            raise ValueError(f"concat operands {tuple(a.shape)} / {tuple(b.shape)} do not match")
        out = self.alloc(n, ca + cb, h, w) if half else self.alloc_f32(n, ca + cb, h, w)
        _lib.check(self.lib.mp_plan_add_concat(self.handle, _lib.ptr(a), ca, _lib.ptr(b), cb, _lib.ptr(out), n, h, w, int(half)),
                   "mp_plan_add_concat")
        self.layer_info.append(dict(kind="concat", n=n, c=ca + cb, h=h, w=w, macs=0))
        return out

    def maxpool3x3s2_same(self, x: torch.Tensor) -> torch.Tensor:
        if isinstance(x, ActC8):
            raise NotImplementedError("max-pool runs on fp32 NCHW activations (the ResNet stem stays fp32 under amp O2)")
        n, c, h, w = x.shape
        out = self.alloc_f32(n, c, (h + 1) // 2, (w + 1) // 2)
        _lib.check(self.lib.mp_plan_add_maxpool(self.handle, _lib.ptr(x), _lib.ptr(out), n, c, h, w), "mp_plan_add_maxpool")
        self.layer_info.append(dict(kind="maxpool", n=n, c=c, h=h, w=w, macs=0))
        return out


class PlannedModule(nn.Module):
    """Base of every module whose forward is a recorded HIP launch plan.

    Sub-classes implement ``emit(plan, x) -> out`` (record launches, return the output buffer, or a list / tuple of them for a
    multi-output network such as HigherHRNet).
    ``forward`` copies the batch into the plan's static input buffer (skipped when the caller already
    wrote into ``input_buffer(shape)``), replays the plan and returns the plan's output buffer - or the list of them
    (views that the next call overwrites - clone them if they must outlive the next forward).
    """

    def __init__(self) -> None:
        super().__init__()
        self._plans: Dict[Tuple, Plan] = {}
        self.training = False  # like mindspore.nn.Cell: inference mode until .train() / set_train(True)
        self.amp_level = "O0"  # see auto_mixed_precision()

    def set_train(self, mode: bool = True):
        """mindspore.nn.Cell.set_train alias."""
        return self.train(mode)

    def train_forward(self, x: torch.Tensor) -> torch.Tensor:
        """Training-mode forward (batch-statistics BatchNorm, autograd through the HIP backward kernels)."""
        raise NotImplementedError("this module has no training path yet")

    def emit(self, plan: Plan, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError("Child class must implement this method.")

    def invalidate_plans(self) -> None:
        """Call after parameters change (checkpoint load, optimizer step): packed weights are re-built."""
        for m in self.modules():
            if isinstance(m, PlannedModule):
                m._plans.clear()

    def _load_from_state_dict(self, *args, **kwargs):
        self._plans.clear()
        return super()._load_from_state_dict(*args, **kwargs)

    def get_plan(self, shape, device) -> Plan:
        half = self.amp_level in ("O2", "O3")
        key = (tuple(shape), str(device), half)
        plan = self._plans.get(key)
        if plan is None:
            if device.type != "cuda":
                raise _lib.MindposeHipError(
                    "mindpose_amd networks run on the MI355X HIP path only (no CPU fallback): move the module and "
                    "its inputs to a CUDA device")
            with torch.no_grad():
                plan = Plan(device, half=half)
                plan.input = plan.alloc_f32(*shape)
                out = self.emit(plan, plan.input)  # backbones switch to the fp16 layout themselves (plan.enter)
                if isinstance(out, (list, tuple)):
                    plan.output = [plan.from_c8(o) if isinstance(o, ActC8) else o for o in out]
                else:
                    plan.output = plan.from_c8(out) if isinstance(out, ActC8) else out
            self._plans[key] = plan
        return plan

    def input_buffer(self, shape, device=None) -> torch.Tensor:
        device = device or next(self.parameters()).device
        return self.get_plan(shape, torch.device(device)).input

    def forward(self, x: torch.Tensor, flip_width: bool = False) -> torch.Tensor:
        """``flip_width``: run the network on the horizontally mirrored batch (the flip test's second run,
        topdown_inferencer.py:168-170): the mirror is written straight into the plan's input buffer by ``mp_flip_width``."""
        x = _lib.require_cuda_f32(x, "input")
        if self.training:
            if flip_width:
                raise ValueError("flip_width is an inference-time option")
            self._plans.clear()  # parameters are about to change: packed weights of recorded plans go stale
            return self.train_forward(x)
        plan = self.get_plan(x.shape, x.device)
        if flip_width:
            if x.data_ptr() == plan.input.data_ptr():
                x = x.clone()  # the caller wrote the batch into the plan's own input buffer: mirror from a copy
            n, c, h, w = x.shape
            _lib.check(plan.lib.mp_flip_width(_lib.ptr(x), _lib.ptr(plan.input), n, c, h, w, _lib.stream()), "mp_flip_width")
        elif x.data_ptr() != plan.input.data_ptr():
            plan.input.copy_(x)
        plan.run()
        return plan.output

    def forward_flip_pair(self, x: torch.Tensor) -> torch.Tensor:
        """The flip test's two runs (topdown_inferencer.py:168-170: ``net(img)``, ``net(flip_W(img))``) as ONE forward of the batch
        [x | mirror(x)]: ``mp_flip_width`` writes the mirrored crops straight into the second half of a 2N plan's input buffer.
        Returns the [2N, K, h, w] output (first N = the crops, last N = their mirrors).  Every sample's arithmetic is what the
        N-crop plan does (inference BatchNorm is per sample); the persistent kernels amortise their weight prologue over twice
        the tiles and the step has half the launches."""
        x = _lib.require_cuda_f32(x, "input")
        if self.training:
            raise ValueError("the flip test is an inference-time path")
        n, c, h, w = x.shape
        plan = self.get_plan((2 * n, c, h, w), x.device)
        first, second = plan.input[:n], plan.input[n:]
        if x.data_ptr() != first.data_ptr():
            first.copy_(x)
        _lib.check(plan.lib.mp_flip_width(_lib.ptr(first), _lib.ptr(second), n, c, h, w, _lib.stream()), "mp_flip_width")
        plan.run()
        return plan.output


def flip_pair_batched() -> bool:
    """``MINDPOSE_FLIP_BATCHED=0``: the flip test runs two forwards of N crops through one plan (rounds 1 - 3) instead of ONE
    forward of the 2N-crop batch [crops | mirrored crops]."""
    return _lib.env_on("MINDPOSE_FLIP_BATCHED")


def auto_mixed_precision(network: nn.Module, amp_level: str = "O0") -> nn.Module:
    """``mindspore.amp.auto_mixed_precision(network, amp_level)`` for the planned networks (what
    ``mindspore.Model(amp_level=...)`` applies in the reference's tools/train.py:176-181).

    O0: fp32 everywhere (fp32 MFMA kernels).  O2 / O3: inference runs the fp16 matrix-core kernels - fp16 conv operands
    and activations, fp32 accumulation, BatchNorm folded in fp32 - and hands fp32 heat maps to the decoder.  (O1 is not
    offered: its white-list casts are a graph rewrite of the MindSpore cells with no counterpart here.)"""
    if amp_level not in ("O0", "O2", "O3"):
        raise ValueError(f"amp_level must be one of O0, O2, O3, got {amp_level!r}")
    for m in network.modules():
        if isinstance(m, PlannedModule):
            m.amp_level = amp_level
            m._plans.clear()
    return network
