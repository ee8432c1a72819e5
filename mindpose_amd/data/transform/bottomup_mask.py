"""The bottom-up training mask (reference: mindpose/data/dataset/coco_bottomup.py:146-189 ``_get_encoded_mask``).

The reference rasterises the crowd regions and the segmentations of persons without key points with pycocotools, sums and thresholds
them into a "valid" plane, erodes that plane per heat-map level with a filled ``cv2.circle`` and keeps the packed bits of all 64 k
training images in memory.  Neither library is installed here; this module is what the project has instead:

* a REGION is one COCO run-length encoding - uint32 counts that alternate zeros / ones, starting with zeros, over the column-major
  pixel index ``x * H + y``, summing to ``H * W``.  ``regions_of_annotation`` turns an annotation's segmentation into regions: a
  dict with a list of counts is one region as it stands, a list of polygons gives one region per polygon (``rle_from_polygon``)
* ``mask_info = dict(regions=[...], shape=(S, H, W), radii=[r_0 .. r_{S-1}])`` is what the mask is made FROM, a few hundred bytes per
  image; ``stage_radii`` restates the reference's 3-sigma radii, all zero without ``expand_mask``
* the mask itself: ``invalid(y, x)`` when any region covers the pixel; stage ``i`` is 1 where no invalid pixel lies under the disc of
  radius ``r_i`` centred on the pixel, pixels outside the image counting as valid (``cv2.erode``'s default border).  The disc is the
  table of per-row half widths of ``disc_half_widths``
* ``decode_mask_info`` computes that on the host in numpy (the oracle of the device path), ``bottomup_masks_batch`` per batch on the
  device in two launches of ``mp_bottomup_train_masks`` (csrc/bottomup_mask_ops.hip) - no start-up pass, no resident mask store.

``rle_from_polygon`` restates pycocotools' ``rleFrPoly`` and ``disc_half_widths`` OpenCV's filled-circle raster from knowledge of
their sources [pycocotools-knowledge] [cv2-knowledge]: PARITY with either library is UNPINNED, neither is installed."""
import ctypes
import math
from typing import Any, Dict, List, Sequence

import numpy as np
import torch

from ... import _lib

__all__ = ["rle_from_polygon", "region_from_counts", "regions_of_annotation", "decode_region", "disc_half_widths", "stage_radii",
           "decode_mask_info", "bottomup_masks_batch", "launch_bottomup_masks", "pack_mask_tables", "MAX_RADIUS"]

MAX_RADIUS = 127  # of the device path: a half width stays below the saturated uint8 row clearance


def rle_from_polygon(xy: Sequence[float], h: int, w: int) -> np.ndarray:
    """The uint32 counts of one polygon ``[x0, y0, x1, y1, ...]`` on an ``h x w`` image: pycocotools' ``rleFrPoly``
    [pycocotools-knowledge, parity unpinned].  The boundary is walked on a grid five times finer; where it crosses from one fine
    column to the next AT a pixel column's centre line, the crossing's row (rounded up, clamped to ``[0, h]``) toggles the column from
    there on - the sorted crossings, differenced, are the runs."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1)
    k = len(xy) // 2
    if k < 1 or len(xy) != 2 * k:
        raise ValueError(f"a polygon is a flat list of x, y pairs, got {len(xy)} numbers")
    scale = 5.0  # every int(...) below is C's (int) of a double: truncation towards zero
    px = [int(scale * xy[2 * j] + .5) for j in range(k)]
    py = [int(scale * xy[2 * j + 1] + .5) for j in range(k)]
    px.append(px[0])
    py.append(py[0])
    us: List[int] = []
    vs: List[int] = []
    for j in range(k):  # every edge along its longer axis, one point per unit step, in the polygon's order
        xs, xe, ys, ye = px[j], px[j + 1], py[j], py[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else 0.0  # a repeated vertex (dx == dy == 0) is the single point t = 0
            for d in range(dx + 1):
                t = dx - d if flip else d
                us.append(t + xs)
                vs.append(int(ys + s * t + .5))
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                vs.append(t + ys)
                us.append(int(xs + s * t + .5))
    crossings = []
    for j in range(1, len(us)):
        if us[j] == us[j - 1]:
            continue
        xd = float(us[j] if us[j] < us[j - 1] else us[j] - 1)
        xd = (xd + .5) / scale - .5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(vs[j] if vs[j] < vs[j - 1] else vs[j - 1])
        yd = (yd + .5) / scale - .5
        yd = math.ceil(min(max(yd, 0.0), float(h)))
        crossings.append(int(xd) * h + int(yd))
    crossings.append(h * w)
    a = np.diff(np.sort(np.asarray(crossings, dtype=np.int64)), prepend=0)
    counts = [int(a[0])]
    j = 1
    while j < len(a):  # a zero-length run after the first joins its neighbours
        if a[j] > 0:
            counts.append(int(a[j]))
            j += 1
        else:
            j += 1
            if j < len(a):
                counts[-1] += int(a[j])
                j += 1
    return np.asarray(counts, dtype=np.uint32)


def region_from_counts(counts: Sequence[int], h: int, w: int, what: str = "region") -> np.ndarray:
    """A list of counts as a region: non-negative integers that sum to ``h * w``."""
    arr = np.asarray(counts)
    if arr.ndim != 1 or arr.size == 0 or not np.issubdtype(arr.dtype, np.integer) or (arr < 0).any():
        raise ValueError(f"{what}: the counts of a run-length encoding are a non-empty list of non-negative integers")
    if int(arr.sum(dtype=np.int64)) != h * w:
        raise ValueError(f"{what}: the counts sum to {int(arr.sum(dtype=np.int64))}, the image has {h} x {w} = {h * w} pixels")
    return arr.astype(np.uint32)


def regions_of_annotation(obj: Dict[str, Any], h: int, w: int) -> List[np.ndarray]:
    """The regions of one annotation's ``segmentation`` (``pycocotools.mask.frPyObjects``): a dict with a list of counts is one
    region, checked against the image; a list of polygons is one region each.  ``ValueError`` names the annotation id; a dict whose
    counts are a compressed string is refused - COCO's key-point files hold none."""
    seg, what = obj["segmentation"], f"annotation {obj.get('id')}"
    if isinstance(seg, dict):
        if isinstance(seg.get("counts"), (str, bytes)):
            raise ValueError(f"{what}: compressed run-length strings are not supported, only lists of counts")
        if [int(v) for v in seg.get("size", ())] != [h, w]:
            raise ValueError(f"{what}: segmentation size {seg.get('size')} is not the image's {[h, w]}")
        return [region_from_counts(seg["counts"], h, w, what)]
    if isinstance(seg, (list, tuple)):
        try:
            return [rle_from_polygon(poly, h, w) for poly in seg]
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
    raise ValueError(f"{what}: segmentation of type {type(seg).__name__} is not supported")


def decode_region(counts: np.ndarray, h: int, w: int) -> np.ndarray:
    """uint8 [h, w], 1 inside the region (``pycocotools.mask.decode``)."""
    counts = np.asarray(counts, dtype=np.int64)
    if int(counts.sum()) != h * w:
        raise ValueError(f"the counts sum to {int(counts.sum())}, the image has {h * w} pixels")
    values = (np.arange(len(counts)) & 1).astype(np.uint8)
    return np.repeat(values, counts).reshape(w, h).T.copy()


def disc_half_widths(r: int) -> np.ndarray:
    """int32 [2 r + 1]: the half width of row ``dy = -r .. r`` of the filled ``cv2.circle(kernel, (r, r), r, 1, -1)``
    [cv2-knowledge, parity unpinned].  OpenCV fills a circle of thickness -1 by its integer midpoint walk: from ``(dx, dy) = (r, 0)``
    while ``dx >= dy`` it draws the spans ``+-dx`` on rows ``+-dy`` and ``+-dy`` on rows ``+-dx``, then steps ``dy`` and lets the
    error term pull ``dx`` in.  The table is symmetric in ``dy``, ``hw[0] == r``, non-increasing in ``|dy|`` and within one pixel of
    ``sqrt(r^2 - dy^2)``."""
    r = int(r)
    if r < 0:
        raise ValueError("a radius is not negative")
    half = np.zeros(r + 1, dtype=np.int32)
    err, dx, dy, plus, minus = 0, r, 0, 1, (r << 1) - 1
    while dx >= dy:
        half[dy] = max(half[dy], dx)
        half[dx] = max(half[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return np.concatenate([half[:0:-1], half])


def stage_radii(sigma: float, num_levels: int) -> List[int]:
    """The erosion radius of every level, the 3-sigma rule of coco_bottomup.py:179-181."""
    return [int(3 * sigma * (2 ** (num_levels - i))) for i in range(num_levels)]


def _check_mask_info(info: Dict[str, Any]):
    s, h, w = (int(v) for v in info["shape"])
    radii = [int(r) for r in info["radii"]]
    if len(radii) != s or s < 1 or h < 1 or w < 1 or min(radii) < 0:
        raise ValueError(f"mask_info: shape {info['shape']} and radii {info['radii']} do not describe [S, H, W] planes")
    return s, h, w, radii


def decode_mask_info(mask_info: Dict[str, Any]) -> np.ndarray:
    """The uint8 [S, H, W] training mask on the host.  Per stage and row distance ``dy`` the invalid plane is widened along its rows by
    the disc's half width (a window count over a running sum) and ORed into the rows ``dy`` away."""
    s, h, w, radii = _check_mask_info(mask_info)
    invalid = np.zeros((h, w), dtype=bool)
    for counts in mask_info["regions"]:
        invalid |= decode_region(counts, h, w).astype(bool)
    out = np.empty((s, h, w), dtype=np.uint8)
    if not invalid.any():
        out[:] = 1
        return out
    running = np.concatenate([np.zeros((h, 1), np.int64), np.cumsum(invalid, axis=1, dtype=np.int64)], axis=1)
    xs = np.arange(w)
    for i, r in enumerate(radii):
        half = disc_half_widths(r)[r:]
        bad = np.zeros((h, w), dtype=bool)
        for d in range(min(r, h - 1) + 1):
            wide = (running[:, np.minimum(w, xs + half[d] + 1)] - running[:, np.maximum(0, xs - half[d])]) > 0
            bad[d:] |= wide[:h - d]   # the row d above
            bad[:h - d] |= wide[d:]   # the row d below
        out[i] = ~bad
    return out


def _align(v: int, to: int = 16) -> int:
    return (v + to - 1) // to * to


def pack_mask_tables(mask_infos: Sequence[Dict[str, Any]], out_offsets: Sequence[int]) -> Dict[str, Any]:
    """The host side of a launch: the four tables of ``mp_bottomup_train_masks`` (``prefix``, ``region_ptr``, ``image_tab``,
    ``offsets``), ``blob`` - the same four back to back for ONE host-to-device copy, ``starts`` their byte offsets in it in the order
    (offsets, image_tab, region_ptr, prefix) -, ``radii``, ``half`` and the workspace size ``clear_bytes``."""
    n = len(mask_infos)
    if n == 0 or len(out_offsets) != n:
        raise ValueError("one output offset per mask_info, at least one")
    s, _, _, radii = _check_mask_info(mask_infos[0])
    image_tab = np.zeros((n, 4), np.int32)
    offsets = np.zeros((n, 2), np.int64)
    region_ptr, prefixes, clear_bytes = [0], [], 0
    for i, info in enumerate(mask_infos):
        si, h, w, ri = _check_mask_info(info)
        if si != s or ri != radii:
            raise ValueError("every image of a batch must have the same stages and radii")
        image_tab[i] = (h, w, len(region_ptr) - 1, len(info["regions"]))
        offsets[i] = (int(out_offsets[i]), clear_bytes)
        if info["regions"]:
            clear_bytes += _align(h * w)
        for counts in info["regions"]:
            counts = np.asarray(counts)
            if counts.ndim != 1 or counts.size == 0:
                raise ValueError("a region is a non-empty one-dimensional array of counts")
            prefixes.append(np.cumsum(counts, dtype=np.uint64).astype(np.uint32))  # a wrong sum is the entry's MP_ERR_SHAPE
            region_ptr.append(region_ptr[-1] + counts.size)
    if max(radii) > MAX_RADIUS:
        raise ValueError(f"the device path serves radii up to {MAX_RADIUS}, got {radii}")
    region_ptr = np.asarray(region_ptr, np.int32)
    prefix = np.concatenate(prefixes) if prefixes else np.zeros(1, np.uint32)
    half = np.zeros((s, MAX_RADIUS + 1), np.uint8)
    for i, r in enumerate(radii):
        half[i, :r + 1] = disc_half_widths(r)[r:]
    parts = [offsets, image_tab, region_ptr, prefix]  # the 8-byte table first: every part starts aligned to its element
    starts = np.cumsum([0] + [_align(p.nbytes) for p in parts])
    blob = np.zeros(int(starts[-1]), np.uint8)
    for p, a in zip(parts, starts):
        blob[a:a + p.nbytes] = p.view(np.uint8).reshape(-1)
    return dict(prefix=prefix, region_ptr=region_ptr, image_tab=image_tab, offsets=offsets, blob=blob, starts=[int(a) for a in starts],
                radii=radii, half=half, clear_bytes=clear_bytes)


def launch_bottomup_masks(mask_infos: Sequence[Dict[str, Any]], out: torch.Tensor, out_offsets: Sequence[int]) -> List[torch.Tensor]:
    """``mp_bottomup_train_masks`` on a caller's buffer: image ``i``'s [S, H_i, W_i] block starts ``out_offsets[i]`` bytes into the
    flat CUDA uint8 tensor ``out``.  Every image of a batch has the same number of stages and the same radii.  The counts go up as
    prefix sums with the per-region and per-image tables in ONE host-to-device copy.  Returns the views of ``out``."""
    if not torch.is_tensor(out) or not out.is_cuda:
        raise _lib.MindposeHipError("out must be a CUDA uint8 tensor: the HIP path has no CPU fallback")
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("out must be a flat contiguous CUDA uint8 tensor")
    t = pack_mask_tables(mask_infos, out_offsets)
    dev, s = out.device, len(t["radii"])
    tables = torch.from_numpy(t["blob"]).to(dev)
    workspace = torch.empty(max(t["clear_bytes"], 16), dtype=torch.uint8, device=dev)
    base, starts = tables.data_ptr(), t["starts"]
    as_p = lambda a, c: a.ctypes.data_as(ctypes.POINTER(c))  # noqa: E731
    _lib.check(_lib.load().mp_bottomup_train_masks(
        as_p(t["prefix"], ctypes.c_uint32), as_p(t["region_ptr"], ctypes.c_int), as_p(t["image_tab"], ctypes.c_int),
        as_p(t["offsets"], ctypes.c_longlong), base + starts[3], base + starts[2], base + starts[1], base + starts[0],
        (ctypes.c_int * s)(*t["radii"]), as_p(t["half"], ctypes.c_uint8), out.data_ptr(), out.numel(), workspace.data_ptr(),
        workspace.numel(), len(mask_infos), s, _lib.stream()), "mp_bottomup_train_masks")
    # tables and workspace go back to the allocator of this stream: nothing reuses them before the launches have run
    return [out[off:off + s * h * w].view(s, h, w) for (h, w), off in zip(t["image_tab"][:, :2].tolist(), t["offsets"][:, 0].tolist())]


def bottomup_masks_batch(mask_infos: Sequence[Dict[str, Any]], device) -> List[torch.Tensor]:
    """The training masks of a batch on the device: one contiguous CUDA uint8 [S, H_i, W_i] tensor per ``mask_info``, views of ONE
    packed buffer (every block 16-byte aligned), made by the two launches of ``mp_bottomup_train_masks`` whatever the batch size.
    Bit-equal to ``decode_mask_info``.  ``bottomup_augment_batch`` takes the tensors as its ``masks``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.MindposeHipError("bottomup_masks_batch runs on the GPU: the HIP path has no CPU fallback")
    offsets, total = [], 0
    for info in mask_infos:
        s, h, w, _ = _check_mask_info(info)
        offsets.append(total)
        total += _align(s * h * w)
    if not offsets:
        raise ValueError("at least one mask_info")
    out = torch.empty(total, dtype=torch.uint8, device=device)
    return launch_bottomup_masks(mask_infos, out, offsets)
