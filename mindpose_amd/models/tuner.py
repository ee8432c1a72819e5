"""The per-shape autotuner of the conv launches: which tile variant / kernel form serves a launch shape fastest, timed once on the
layer's real buffers, cached per process, optionally persisted (``MINDPOSE_TUNE_CACHE``) and shared between the ranks of a job
(`share_tuner_choices`).  The plan builder (layers.py) and the training ops (train_ops.py) both pick their variants here."""
import ctypes
import os
from typing import Dict, Optional, Tuple

import torch

from .. import _lib
from .act_c8 import ActC8

F16_VARIANTS = 48  # csrc/conv_f16.h F_COUNT: tile shapes the fp16 autotuner times per launch shape
F16_WS_BASE = 37   # csrc/conv_f16.h F_WS_BASE: first weight-stationary persistent shape (conv_f16_ws.hip)

_TUNE_CACHE: Dict[Tuple, int] = {}
_TUNE_FILE_LOADED = False


def _tune_file() -> Optional[str]:
    """MINDPOSE_TUNE_CACHE=<path>: persist the autotuner's choices (JSON, keyed by launch shape) so that a later process
    - a profiling run, a production worker - replays them without timing trial launches."""
    return os.environ.get("MINDPOSE_TUNE_CACHE") or None


_BUILD_ID = None


def _tune_stamp() -> str:
    """Variant indices only mean something for one BUILD of the kernels: the stamp carries the library's version string and a
    digest of the shared object itself (a rebuilt kernel invalidates the persisted choices without a hand-bumped version)."""
    global _BUILD_ID
    if _BUILD_ID is None:
        import hashlib
        h = hashlib.sha1()
        try:
            with open(_lib.LIB_PATH, "rb") as f:
                for block in iter(lambda: f.read(1 << 20), b""):
                    h.update(block)
            _BUILD_ID = h.hexdigest()[:16]
        except OSError:
            _BUILD_ID = "unknown"
    return f"{_lib.load().mp_version().decode()}|{_BUILD_ID}"


def _tune_load() -> None:
    global _TUNE_FILE_LOADED
    path = _tune_file()
    if _TUNE_FILE_LOADED or not path:
        return
    _TUNE_FILE_LOADED = True
    try:
        import json
        with open(path) as f:
            doc = json.load(f)
        if doc.get("stamp") != _tune_stamp():  # written by another library version: variant indices may have moved
            return
        for k, v in doc.get("choices", {}).items():
            _TUNE_CACHE.setdefault(k, int(v))
    except (OSError, ValueError, AttributeError):
        pass


def _dist_rank_world():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return 0, 1


def share_tuner_choices(group=None) -> int:
    """THE collective of the tuner, at a point the CALLER chooses: rank 0's whole choice table is broadcast once
    (``broadcast_object_list``) and every other rank adopts it, so that the ranks of one job run the same numeric form of every
    layer (the fp32 candidates differ numerically: Winograd vs direct, one GEMM launch vs four phase convs).  Every rank of
    ``group`` must call it, at the same point of its program - e.g. right after rank 0's warm-up (`tune_on_rank0_first`).  The
    tuner itself never communicates: a plan that only one rank builds (EvalCallback's rank-0 evaluation, a no-grad probe) can
    therefore never strand or cross-match a collective.  Returns the number of choices adopted (0 on rank 0 / one rank)."""
    if _dist_rank_world()[1] == 1:
        return 0
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)  # ranks OF THE GROUP: a sub-group without global rank 0 has its own sender
    if world <= 1:
        return 0
    box = [{k: v for k, v in _TUNE_CACHE.items() if isinstance(k, str)} if rank == 0 else None]
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if rank == 0:
        return 0
    _TUNE_CACHE.update(box[0])
    return len(box[0])


def tune_on_rank0_first(build, group=None):
    """``build()`` - anything that records plans / runs warm-up passes and contains NO collective - on rank 0 first (it tunes),
    then `share_tuner_choices`, then on the other ranks (every shape is a cache hit: nothing is timed twice, all ranks run rank 0's
    forms).  One rank: just ``build()``.  Rank 0 reaches the broadcast even when its ``build()`` raised (the exception is re-raised
    behind it), so a failure on rank 0 cannot leave the other ranks waiting."""
    if _dist_rank_world()[1] == 1:
        return build()
    import torch.distributed as dist
    rank = dist.get_rank(group)
    out, failure = None, None
    if rank == 0:
        try:
            out = build()
        except Exception as exc:  # noqa: BLE001 - re-raised below, after the collective every rank is waiting in
            failure = exc
    share_tuner_choices(group)
    if failure is not None:
        raise failure
    return out if rank == 0 else build()


def _tune_save() -> None:
    """Whole-file replace through a temporary (a torn file would silently drop the cache); rank 0 is the only writer of a job."""
    path = _tune_file()
    if not path or _dist_rank_world()[0] != 0:
        return
    try:
        import json
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump({"stamp": _tune_stamp(), "choices": {k: v for k, v in _TUNE_CACHE.items() if isinstance(k, str)}}, f)
        os.replace(tmp, path)
    except OSError:
        pass


# launches below this many multiply-accumulates keep the library's heuristic (MINDPOSE_TUNE_MIN_MACS overrides).  Round 4 tuned from
# 2^26 up - which left EVERY layer of a one-crop forward (28 M MACs per 32-channel conv at N = 1) on the heuristic: a top-down
# pipeline serves a handful of crops per frame, and there the tile choice decides whether a launch covers 8 or 64 CUs
_TUNE_MIN_MACS = int(os.environ.get("MINDPOSE_TUNE_MIN_MACS", str(1 << 22)))


def autotune_on() -> bool:
    """``MINDPOSE_AUTOTUNE=0``: no trial launches, every launch keeps the library's heuristic (`_autotune` returns -1)."""
    return _lib.env_on("MINDPOSE_AUTOTUNE")


def tuned(macs: int) -> bool:
    """THE policy: is a launch of this many multiply-accumulates given a timed variant (else: the library's heuristic)?  Whoever
    has to know what `_autotune` will record - the plan builder's "does any kernel serve this conv" - asks here."""
    return autotune_on() and macs >= _TUNE_MIN_MACS


def _autotune(key, macs, n_variants, launch) -> int:
    """Time ``launch(v)`` for every tile variant (HIP events, best of two groups of 5 launches; MP_ERR_UNSUPPORTED = variant not
    available, any other error code raises) and cache the winner per launch shape; -1 = library heuristic when tuning is off (MINDPOSE_AUTOTUNE=0) or
    pointless (tiny layers)."""
    if not autotune_on():
        return -1
    _tune_load()
    key = repr(key)
    hit = _TUNE_CACHE.get(key)
    if hit is not None:
        return hit
    best, best_t = -1, None
    if tuned(macs):  # a miss is timed on whichever rank meets it - no communication here (share_tuner_choices)
        for v in range(n_variants):
            rc = launch(v)
            if rc == _lib.MP_ERR_UNSUPPORTED:  # this variant does not serve the shape
                continue
            _lib.check(rc, f"tuner trial launch, variant {v}, {key}")  # any other code (a HIP error) must not silently drop a candidate
            t = None
            for _ in range(2):  # best of two groups of five: one group of three mis-ranked close candidates run to run (+-1.5 %)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    launch(v)
                e1.record()
                e1.synchronize()
                dt = e0.elapsed_time(e1)
                t = dt if t is None or dt < t else t
            if best_t is None or t < best_t:
                best, best_t = v, t
            log = os.environ.get("MINDPOSE_TUNE_LOG")  # per-candidate timings (ms per 5 launches), for kernel work
            if log:
                with open(log, "a") as fh:
                    fh.write(f"{key}\t{v}\t{t:.4f}\n")
    _TUNE_CACHE[key] = best
    if tuned(macs):
        _tune_save()
    return best


BLOCK_ROWS = (0, 4, 2, 1)  # band heights the fused-BasicBlock tuner times (0 = the tallest that fits)
F32_VARIANTS = 9   # direct MFMA tile variants 0..7 (csrc/conv_mfma.h ConvVariant) + 8 = the streaming 1x1 kernel (conv_pw_f32.hip)
F32_WINOGRAD = 9   # the tuner's index of the Winograd F(2x2,3x3) form (csrc/conv_wino_f32.hip)
F32_GEMM = 10      # the blocked-GEMM 1x1 kernel (csrc/conv_gemm_f32.hip; conv_api.hip kGemm)
F32_SMALL = 11     # the K-split kernel for small problems - a handful of crops (csrc/conv_small_f32.hip; conv_api.hip kSmall)
F32_SMALL_WIDE = 12  # ... with 48 / 64 pixels per workgroup (a few dozen crops: the weights of a workgroup serve more pixels)


def winograd_enabled() -> bool:
    """``MINDPOSE_WINOGRAD=0`` keeps every fp32 3x3 convolution on the direct kernel (bit-identical to round 1's results)."""
    return _lib.env_on("MINDPOSE_WINOGRAD")


def tune_conv_variant(lib, d, x, packed, scale, shift, res1, res2, out, half: bool = False, packed_u=None, stats=None) -> int:
    """Pick the tile variant for one conv launch shape by timing the candidates on the layer's real buffers.  Results
    are cached per shape, so a network's ~40 distinct shapes are tuned once per process.  ``packed_u`` (fp32 only): the
    Winograd-transformed weights; the Winograd form then competes as index ``F32_WINOGRAD``.  ``stats`` (fp16 training):
    ``dict(mode, z, y, relu)`` - the launch is the one with BatchNorm statistics in its epilogue (mp_f16_conv2d_fwd_stats: other
    register budgets, two more tensor reads in mode 2), timed as such and cached under its own key; with ``pre = dict(scale, shift, y,
    relu)`` the launch also applies the BatchNorm of the layer below on its operand (candidates: mp_f16_conv_pre_supported)."""
    key = tuple(getattr(d, f) for f, _ in d._fields_) + (res1 is not None, res2 is not None, str(out.device), half)
    if packed_u is not None:
        key += ("wino",)
    if stats is not None:
        key += ("stats", int(stats["mode"]), int(bool(stats.get("relu"))))
        if stats.get("pre") is not None:  # BatchNorm apply of the layer below on the operand: its own candidate set, its own key
            key += ("pre",)
    macs = d.n * d.conv_h * d.conv_w * d.cout * d.cin * d.kh * d.kw
    stream = _lib.stream()
    # in-place accumulation (out aliases res1) must not be disturbed by trial launches: tune into a scratch copy
    alias = res1 is not None and res1.data_ptr() == out.data_ptr()
    trial_out = out
    if alias:
        trial_out = torch.empty_like(out) if torch.is_tensor(out) else ActC8(*out.shape, out.device)
    fn = lib.mp_f16_conv2d_fwd if half else lib.mp_conv2d_fwd_variant

    stats_buf = {}
    # a statistics build that leaves more than 512 partial slots per channel costs its consumer an extra fold launch (~5 us): such
    # variants compete only when no variant of the shape stays within 512
    slot_cap = [512]
    with_pre = stats is not None and stats.get("pre") is not None
    if stats is not None and not any(0 < lib.mp_f16_conv_stats_parts(ctypes.byref(d), v) <= 512 for v in range(F16_VARIANTS)
                                     if not with_pre or lib.mp_f16_conv_pre_supported(ctypes.byref(d), v)):
        slot_cap[0] = 1 << 30

    no_small = not _lib.env_on("MINDPOSE_F32_SMALL")  # before / after evidence: the candidate set without the small-problem kernel
    no_ws = half and not _lib.env_on("MINDPOSE_F16_WS")  # before / after evidence: the round-3 candidate set

    def launch(v):
        if no_ws and v >= F16_WS_BASE:  # (the round-4 weights-in-registers shapes 45.. included)
            return _lib.MP_ERR_UNSUPPORTED
        if stats is not None:
            n_parts = lib.mp_f16_conv_stats_parts(ctypes.byref(d), v)
            if n_parts <= 0 or n_parts > slot_cap[0]:
                return _lib.MP_ERR_UNSUPPORTED
            need = (d.cout + 7) // 8 * n_parts * 16
            if stats_buf.get("n", 0) < need:
                stats_buf["t"], stats_buf["n"] = torch.empty(need, device=out.device, dtype=torch.float32), need
            st = _lib.ConvStats(mode=int(stats["mode"]), relu=int(bool(stats.get("relu"))), partials=stats_buf["t"].data_ptr(),
                                partials_bytes=need * 4, z=_lib.ptr(stats.get("z")), y=_lib.ptr(stats.get("y")) if stats.get("relu") else None)
            pre = stats.get("pre")
            if pre is not None:
                if not lib.mp_f16_conv_pre_supported(ctypes.byref(d), v):
                    return _lib.MP_ERR_UNSUPPORTED
                st.pre_scale, st.pre_shift, st.pre_out, st.pre_relu = _lib.ptr(pre["scale"]), _lib.ptr(pre["shift"]), _lib.ptr(pre["y"]), int(pre["relu"])
            return lib.mp_f16_conv2d_fwd_stats(ctypes.byref(d), v, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(shift),
                                               _lib.ptr(res1), _lib.ptr(trial_out), ctypes.byref(st), stream)
        if not half and v in (F32_SMALL, F32_SMALL_WIDE) and no_small:
            return _lib.MP_ERR_UNSUPPORTED
        if not half and v == F32_WINOGRAD:
            if packed_u is None:
                return _lib.MP_ERR_UNSUPPORTED  # no Winograd form of this layer
            return lib.mp_conv2d_winograd_fwd(ctypes.byref(d), _lib.ptr(x), _lib.ptr(packed_u), _lib.ptr(scale), _lib.ptr(shift),
                                              _lib.ptr(res1), _lib.ptr(res2), _lib.ptr(trial_out), stream)
        return fn(ctypes.byref(d), v, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(res1),
                  _lib.ptr(res2), _lib.ptr(trial_out), stream)

    return _autotune(key, macs, F16_VARIANTS if half else F32_SMALL_WIDE + 1, launch)
