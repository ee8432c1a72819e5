"""Bottom-up evaluation transforms: rescale / resize to the network input and the pad (reference:
mindpose/data/transform/bottomup_transform.py:26-85, :143-301, :601-645).

Names, constructors, config keys and the keys ``transform(state)`` returns are the reference's.  The geometry - the target size,
``center``, ``scale``, ``image_shape`` - is the reference's own Python / numpy arithmetic.  ``transform`` is the host (numpy) path;
the pipeline (data_factory.py ``BottomUpPipeline``) recognises these transforms, records their geometry with ``geometry`` and does
the pixel work of a batch in ONE launch (``mp_resize_pad_normalize`` for rescale + pad, ``mp_warp_affine`` for resize), for which
the host path is the oracle.

``cv2.resize`` and ``cv2.warpAffine`` are restated from OpenCV's 8-bit fixed-point linear paths [cv2-knowledge]: cv2 is not a
dependency and parity with cv2 itself is unpinned.

``BottomUpGenerateTarget`` (:463-598) writes the ``target`` / ``tag_ind`` arrays of the training losses: ``transform`` is the
reference's numpy arithmetic for one image, ``generate_batch`` one ``mp_bottomup_target`` launch for a batch on the device.

The train-time augmentations ``BottomUpRandomAffine`` (:304-460) and ``BottomUpHorizontalRandomFlip`` (:88-140) have the same two
forms: ``transform`` is the host path - the reference's random draws through the global ``np.random`` in its order, its matrices and
key-point arithmetic, the mask through ``warp_affine_nearest_u8`` (``cv2.warpAffine(..., INTER_NEAREST)`` restated [cv2-knowledge],
parity with cv2 itself unpinned) - and ``bottomup_augment_batch`` draws per image exactly as the two ``transform`` s would, computes
the key points on the host with the same functions and does the pixel work of the batch - the image warp, every stage's mask warp,
the flip, Normalize and HWC2CHW - in ONE ``mp_bottomup_train_augment`` launch (``mp_bottomup_train_augment_stages`` when a mask
comes as [S, H, W], one source plane per stage, as ``bottomup_masks_batch`` of bottomup_mask.py makes them).  Its result is what
``generate_batch`` and ``AEMultiLoss`` take.  No pipeline runs in train mode yet.
"""
import ctypes
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from ...register import register
from ..column_names import COLUMN_MAP
from ._launch import norm255, source_batch
from .topdown_transform import fliplr_joints, get_affine_transform
from .utils import pad_to_same, warp_affine_joints

__all__ = ["BottomUpTransform", "BottomUpRescale", "BottomUpResize", "BottomUpPad", "BottomUpGenerateTarget", "BottomUpRandomAffine",
           "BottomUpHorizontalRandomFlip", "bottomup_augment_batch", "resize_linear_u8", "warp_affine_linear_u8",
           "warp_affine_nearest_u8", "launch_resize_pad_normalize"]

NORMALIZE_MEAN = (0.485, 0.456, 0.406)  # data_factory.py:78-79 (the reference's std really ends in 0.255)
NORMALIZE_STD = (0.229, 0.224, 0.255)


def _resize_terms(dst: int, src: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Source index and the two 11-bit coefficients of every destination coordinate of one axis: scale = src / dst in double,
    f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; s < 0 -> (0, 0); s >= src - 1 -> (src - 1, 0); the coefficients
    are saturate_cast<short>((1 - f) * 2048) and saturate_cast<short>(f * 2048) (round half to even)."""
    scale = src / dst
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    c0 = np.clip(np.rint((np.float32(1) - f) * np.float32(2048)), -32768, 32767).astype(np.int32)
    c1 = np.clip(np.rint(f * np.float32(2048)), -32768, 32767).astype(np.int32)
    return s, c0, c1


def resize_linear_u8(image: np.ndarray, size: Tuple[int, int]) -> np.ndarray:
    """``cv2.resize(image, (w, h), interpolation=cv2.INTER_LINEAR)`` of a uint8 [H, W, C] image: horizontal pass int32
    S[sx] * a0 + S[sx + 1] * a1, vertical pass (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, saturated."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3:
        raise ValueError(f"image must be uint8 [H, W, C], got {image.dtype} {image.shape}")
    tw, th = int(size[0]), int(size[1])
    h, w = image.shape[:2]
    sx, a0, a1 = _resize_terms(tw, w)
    sy, b0, b1 = _resize_terms(th, h)
    src = image.astype(np.int32)
    rows = src[:, sx] * a0[None, :, None] + src[:, np.minimum(sx + 1, w - 1)] * a1[None, :, None]  # [H, tw, C]
    r0, r1 = rows[sy], rows[np.minimum(sy + 1, h - 1)]
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def _invert_affine(trans: np.ndarray) -> Tuple[float, float, float, float, float, float]:
    """The inverse of a 2 x 3 forward matrix as ``cv::warpAffine`` forms it (no WARP_INVERSE_MAP), in double."""
    m = np.array(trans, dtype=np.float64).reshape(2, 3)
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    det = 1.0 / det if det != 0 else 0.0
    i00, i01, i10, i11 = m[1, 1] * det, m[0, 1] * -det, m[1, 0] * -det, m[0, 0] * det
    i02, i12 = -i00 * m[0, 2] - i01 * m[1, 2], -i10 * m[0, 2] - i11 * m[1, 2]
    return i00, i01, i02, i10, i11, i12


def _warp_coords(trans: np.ndarray, size: Tuple[int, int], round_delta: int, shift: int) -> Tuple[np.ndarray, np.ndarray]:
    """The fixed-point source coordinates (X, Y), int64 [h, w] each, of every pixel of a (w, h) destination as ``cv::warpAffine``
    forms them: the matrix inverted in double, the 10-bit terms of a row and of a column rounded separately,
    X = (cvRound((i01 y + i02) 1024) + round_delta + cvRound(i00 x 1024)) >> shift and likewise Y."""
    out_w, out_h = int(size[0]), int(size[1])
    i00, i01, i02, i10, i11, i12 = _invert_affine(trans)
    xs, ys = np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64)

    def grid(col, row, offset):
        return ((np.rint((row * ys + offset) * 1024.0).astype(np.int64) + round_delta)[:, None]
                + np.rint(col * xs * 1024.0).astype(np.int64)[None]) >> shift

    return grid(i00, i01, i02), grid(i10, i11, i12)


def warp_affine_linear_u8(image: np.ndarray, trans: np.ndarray, size: Tuple[int, int]) -> np.ndarray:
    """``cv2.warpAffine(image, trans, (w, h), flags=cv2.INTER_LINEAR)`` of a uint8 [H, W, C] image, border constant 0: the matrix
    inverted in double, coordinates in 10-bit fixed point quantised to 1 / 32 pixel, exact 15-bit bilinear weights - the
    arithmetic of ``mp_warp_affine`` (csrc/loader_ops.hip)."""
    img = np.asarray(image)
    h, w, _ = img.shape
    big_x, big_y = _warp_coords(trans, size, 16, 5)
    sx, sy = np.clip(big_x >> 5, -32768, 32767), np.clip(big_y >> 5, -32768, 32767)
    fx, fy = big_x & 31, big_y & 31
    acc = np.zeros(big_x.shape + (img.shape[2],), np.int64)
    for dy, dx, weight in ((0, 0, (32 - fx) * (32 - fy) * 32), (0, 1, fx * (32 - fy) * 32), (1, 0, (32 - fx) * fy * 32),
                           (1, 1, fx * fy * 32)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        px = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64)
        acc += np.where(inside[..., None], px, 0) * weight[..., None]
    return np.minimum((acc + (1 << 14)) >> 15, 255).astype(np.uint8)


def warp_affine_nearest_u8(mask: np.ndarray, trans: np.ndarray, size: Tuple[int, int]) -> np.ndarray:
    """``cv2.warpAffine(mask, trans, (w, h), flags=cv2.INTER_NEAREST)`` of a uint8 [H, W] (or [H, W, C]) array, border constant 0
    [cv2-knowledge]: the matrix inverted in double as in ``warp_affine_linear_u8``, the 10-bit fixed-point coordinate terms of a
    row and of a column rounded separately, X = (cvRound((i01 y + i02) 1024) + 512 + cvRound(i00 x 1024)) >> 10 and likewise Y,
    saturated to int16; the source pixel when (X, Y) lies inside the array, else 0.  cv2 is not a dependency: parity with cv2
    itself is UNPINNED, exactly as for the linear warp.  The mask arithmetic of ``mp_bottomup_train_augment``."""
    src = np.asarray(mask)
    if src.dtype != np.uint8 or src.ndim not in (2, 3):
        raise ValueError(f"mask must be uint8 [H, W] or [H, W, C], got {src.dtype} {src.shape}")
    h, w = src.shape[:2]
    sx, sy = (np.clip(v, -32768, 32767) for v in _warp_coords(trans, size, 512, 10))
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    px = src[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
    return np.where(inside if src.ndim == 2 else inside[..., None], px, 0).astype(np.uint8)


def launch_resize_pad_normalize(images: Sequence[torch.Tensor], target_sizes: Sequence[Tuple[int, int]], padded_size: Tuple[int, int],
                                mean, std) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``mp_resize_pad_normalize`` launch: image ``i`` (CUDA uint8 [H, W, 3], all views of one buffer or separate tensors)
    resized to ``target_sizes[i]`` = (w, h), zero-padded to ``padded_size`` = (w, h), normalised with ``mean`` / ``std`` (of the
    0..1 range) and written as planes.  Returns (image [N, 3, PH, PW] fp32, mask [N, PH, PW] uint8)."""
    lib = _lib.load()
    n = len(images)
    if n == 0 or len(target_sizes) != n:
        raise ValueError("one target size per image, at least one image")
    base, offs, hw, dev = source_batch(images)
    pw, ph = int(padded_size[0]), int(padded_size[1])
    twh = (ctypes.c_int * (2 * n))(*[int(v) for size in target_sizes for v in size[:2]])
    out = torch.empty(n, 3, ph, pw, device=dev, dtype=torch.float32)
    mask = torch.empty(n, ph, pw, device=dev, dtype=torch.uint8)
    m3, s3 = norm255(mean, std)
    _lib.check(lib.mp_resize_pad_normalize(base, _lib.ptr(offs), _lib.ptr(hw), twh, _lib.ptr(out), _lib.ptr(mask), n, ph, pw, m3, s3,
                                           _lib.stream()), "mp_resize_pad_normalize")
    return out, mask


class BottomUpTransform:
    """Base of the bottom-up transforms (bottomup_transform.py:26-85): ``is_train``, ``config`` and the parsed ``_transform_cfg``.
    A child implements ``transform(state) -> dict`` of the updated keys."""

    def __init__(self, is_train: bool = True, config: Optional[Dict[str, Any]] = None) -> None:
        self.is_train = is_train
        self.config = config if config else dict()
        self._transform_cfg = self.load_transform_cfg()
        self._required_field = self.setup_required_field()

    def setup_required_field(self) -> List[str]:
        return COLUMN_MAP["bottomup"]["train" if self.is_train else "val"]

    def load_transform_cfg(self) -> Dict[str, Any]:
        """:54-85 - same keys (a missing one is a KeyError), same derived ``flip_index``."""
        cfg = dict()
        cfg["image_size"] = np.array(self.config["image_size"])
        cfg["max_image_size"] = np.array(self.config["max_image_size"])
        cfg["heatmap_sizes"] = np.array(self.config["heatmap_sizes"])
        assert len(cfg["image_size"]) == 2
        for x in cfg["heatmap_sizes"]:
            assert len(x) == 2
        flip_pairs = np.array(self.config["flip_pairs"])
        if len(flip_pairs.shape) == 2:
            flip_index = flip_pairs[:, ::-1].flatten()
            flip_index = np.insert(flip_index, 0, 0)
        else:
            flip_index = flip_pairs
        cfg["flip_pairs"] = flip_pairs
        cfg["flip_index"] = flip_index
        cfg["pixel_std"] = float(self.config["pixel_std"])
        cfg["tag_per_joint"] = self.config["tag_per_joint"]
        return cfg

    def transform(self, state: Dict[str, Any]) -> Dict[str, Any]:
        raise NotImplementedError("Child class must implement this method.")

    def __call__(self, *args: Any) -> Tuple[np.ndarray, ...]:
        states = dict(zip(self._required_field, args))
        states.update(self.transform(states))
        return tuple(np.asarray(states[k]) for k in self._required_field)


@register("transform", extra_name="bottomup_horizontal_random_flip")
class BottomUpHorizontalRandomFlip(BottomUpTransform):
    """Random horizontal flip of the augmented sample (:88-140): the image, the ``[:height, :width]`` corner of every stage's mask
    and every stage's key points (mirrored in that stage's width, left / right joints swapped)."""

    def __init__(self, is_train: bool = True, config: Optional[Dict[str, Any]] = None, flip_prob: float = 0.5) -> None:
        super().__init__(is_train, config)
        self.flip_prob = flip_prob

    def draw(self) -> bool:
        """The one random number of a sample (:128): flip or not."""
        return bool(np.random.rand() <= self.flip_prob)

    def flip_keypoints(self, keypoints: np.ndarray) -> np.ndarray:
        """[S, M, K, 3] key points, stage i mirrored in stage i's width, in place (:135-137)."""
        for i, heatmap_size in enumerate(self._transform_cfg["heatmap_sizes"]):
            keypoints[i] = fliplr_joints(keypoints[i], heatmap_size[0], flip_index=self._transform_cfg["flip_index"])
        return keypoints

    def transform(self, state: Dict[str, Any]) -> Dict[str, Any]:
        """Required: image, mask, keypoints.  Returned: image, mask, keypoints (mask and keypoints are changed in place)."""
        image, keypoints, mask = state["image"], state["keypoints"], state["mask"]
        if self.draw():
            image = np.ascontiguousarray(image[:, ::-1])  # cv2.flip(image, 1)
            for i, (width, height) in enumerate(self._transform_cfg["heatmap_sizes"]):
                mask[i, :height, :width] = mask[i, :height, :width][:, ::-1].copy()  # the padding does not move
            self.flip_keypoints(keypoints)
        return dict(image=image, keypoints=keypoints, mask=mask)


@register("transform", extra_name="bottomup_rescale")
class BottomUpRescale(BottomUpTransform):
    """Rescale the image into ``max_image_size`` keeping its aspect ratio (:143-208)."""

    def _get_new_size(self, image_size: Tuple[int, int], max_size: Tuple[int, int]) -> Tuple[int, int]:
        w, h = image_size
        max_w, max_h = max_size
        if w < h:  # portrait: the limits swap
            max_w, max_h = max_h, max_w
        if w / h > max_w / max_h:
            target_w = max_w
            target_h = round(h * max_w / w)
        else:
            target_h = max_h
            target_w = round(w * max_h / h)
        return int(target_w), int(target_h)

    def geometry(self, width: int, height: int) -> Dict[str, Any]:
        """center, scale and image_shape = (target_w, target_h) of an image of this size: everything but the pixels."""
        target_size = self._get_new_size([width, height], self._transform_cfg["max_image_size"])
        pixel_std = self._transform_cfg["pixel_std"]
        return dict(center=np.array([round(width / 2), round(height / 2)]), scale=np.array([width / pixel_std, height / pixel_std]),
                    image_shape=target_size)

    def transform(self, state: Dict[str, Any]) -> Dict[str, Any]:
        """Required: image.  Returned: image, center, scale, image_shape."""
        image = state["image"]
        height, width = image.shape[:2]
        out = self.geometry(width, height)
        out["image"] = resize_linear_u8(image, out["image_shape"])
        return out


@register("transform", extra_name="bottomup_resize")
class BottomUpResize(BottomUpTransform):
    """Resize so that the short side becomes ``size`` and both sides multiples of ``base_length``, by an affine warp about the
    image centre (:211-301)."""

    def __init__(self, is_train: bool = True, config: Optional[Dict[str, Any]] = None, size: int = 512, base_length: int = 64) -> None:
        super().__init__(is_train, config)
        self.size = size
        self.base_length = base_length

    @staticmethod
    def _ceil_to_base_length(x: int, base_length: int) -> int:
        return int(np.ceil(x / base_length)) * base_length

    def _get_new_size(self, image_size: Tuple[int, int], size: int, base_length: int = 64,
                      pixel_std: float = 200.0) -> Tuple[Tuple[int, int], np.ndarray, np.ndarray]:
        w, h = image_size
        min_size = self._ceil_to_base_length(size, base_length)
        if w < h:
            target_w = min_size
            target_h = self._ceil_to_base_length(min_size / w * h, base_length)
            scale_w = w / pixel_std
            scale_h = target_h / target_w * w / pixel_std
        else:
            target_h = min_size
            target_w = self._ceil_to_base_length(min_size / h * w, base_length)
            scale_h = h / pixel_std
            scale_w = target_w / target_h * h / pixel_std
        center = np.array([round(w / 2), round(h / 2)])
        scale = np.array([scale_w, scale_h])
        return (target_w, target_h), center, scale

    def geometry(self, width: int, height: int) -> Dict[str, Any]:
        """center, scale, image_shape and the 2 x 3 warp matrix ``_trans`` of an image of this size."""
        target_size, center, scale = self._get_new_size([width, height], self.size, base_length=self.base_length,
                                                        pixel_std=self._transform_cfg["pixel_std"])
        return dict(center=center, scale=scale, image_shape=target_size, _trans=get_affine_transform(center, scale, 0, target_size))

    def transform(self, state: Dict[str, Any]) -> Dict[str, Any]:
        """Required: image.  Returned: image, mask, center, scale, image_shape."""
        image = state["image"]
        height, width = image.shape[:2]
        out = self.geometry(width, height)
        out["image"] = warp_affine_linear_u8(image, out.pop("_trans"), out["image_shape"])
        out["mask"] = np.ones(out["image"].shape[:2], dtype=np.uint8)
        return out


@register("transform", extra_name="bottomup_pad")
class BottomUpPad(BottomUpTransform):
    """Zero-pad on the right and bottom to ``max_image_size`` (swapped for a portrait image) and make the mask (:601-645)."""

    def padded_size(self, width: int, height: int) -> Tuple[int, int]:
        target_width, target_height = (int(v) for v in self._transform_cfg["max_image_size"])
        if width < height:
            target_height, target_width = target_width, target_height
        assert target_width >= width
        assert target_height >= height
        return target_width, target_height

    def transform(self, state: Dict[str, Any]) -> Dict[str, Any]:
        """Required: image.  Returned: image, mask."""
        image = state["image"]
        height, width = image.shape[:2]
        target_width, target_height = self.padded_size(width, height)
        image = np.pad(image, ((0, target_height - height), (0, target_width - width), (0, 0)))
        mask = np.zeros((target_height, target_width), dtype=np.uint8)
        mask[:height, :width] = 1
        return dict(image=image, mask=mask)


@register("transform", extra_name="bottomup_random_affine")
class BottomUpRandomAffine(BottomUpTransform):
    """Random scale, rotation and translation about the image centre (:304-460): the image is warped to ``image_size``, the mask
    and the key points of stage i to ``heatmap_sizes[i]``, each by a matrix of its own from the same draw."""

    def __init__(self, is_train: bool = True, config: Optional[Dict[str, Any]] = None, rot_factor: float = 30.0,
                 scale_factor: Tuple[float, float] = (0.75, 1.5), scale_type: str = "short", trans_factor: float = 40.0) -> None:
        super().__init__(is_train=is_train, config=config)
        self.max_rotation = rot_factor
        self.min_scale = scale_factor[0]
        self.max_scale = scale_factor[1]
        self.scale_type = scale_type
        self.trans_factor = trans_factor

    def _get_scale(self, image_size: Tuple[int, int], resized_size: Tuple[int, int]) -> np.ndarray:
        """The source extent that maps onto ``resized_size`` with its aspect ratio (:337-363): the long or the short side of the
        image fills the output."""
        if self.scale_type not in ("long", "short"):
            raise ValueError(f"Unknown scale type: {self.scale_type}")
        w, h = image_size
        w_resized, h_resized = resized_size
        fit_height = (w / w_resized < h / h_resized) == (self.scale_type == "long")
        if fit_height:
            w_pad, h_pad = h / h_resized * w_resized, h
        else:
            w_pad, h_pad = w, w / w_resized * h_resized
        return np.array([w_pad, h_pad], dtype=np.float32)

    def draw(self, width: int, height: int) -> Dict[str, Any]:
        """The random numbers of one sample, drawn from the global ``np.random`` in the reference's order with its argument
        expressions (:389-409): scale, rotation and - only with a positive ``trans_factor`` - dx, then dy."""
        center = np.array((width / 2, height / 2))
        img_scale = np.array([width, height], dtype=np.float32)
        aug_scale = np.random.uniform(self.min_scale, self.max_scale)
        img_scale *= aug_scale
        aug_rot = np.random.uniform(-self.max_rotation, self.max_rotation)
        pixel_std = self._transform_cfg["pixel_std"]
        if self.trans_factor > 0:
            dx = np.random.randint(-self.trans_factor * img_scale[0] / pixel_std, self.trans_factor * img_scale[0] / pixel_std)
            dy = np.random.randint(-self.trans_factor * img_scale[1] / pixel_std, self.trans_factor * img_scale[1] / pixel_std)
            center[0] += dx
            center[1] += dy
        return dict(center=center, img_scale=img_scale, rot=aug_rot)

    def matrices(self, draw: Dict[str, Any]) -> np.ndarray:
        """The 2 x 3 forward matrices of a draw, float64 [S + 1, 2, 3]: the heat-map stages first, the image last (:414-444)."""
        pixel_std = self._transform_cfg["pixel_std"]
        sizes = list(self._transform_cfg["heatmap_sizes"]) + [self._transform_cfg["image_size"]]
        return np.stack([get_affine_transform(center=draw["center"], scale=self._get_scale(draw["img_scale"], size) / pixel_std,
                                              rot=draw["rot"], output_size=size, pixel_std=pixel_std) for size in sizes])

    @staticmethod
    def warp_keypoints(keypoints: np.ndarray, mats: np.ndarray) -> np.ndarray:
        """[S, M, K, 3] key points, stage i through ``mats[i]``, in place (:434)."""
        for i in range(keypoints.shape[0]):
            keypoints[i, :, :, 0:2] = warp_affine_joints(keypoints[i, :, :, 0:2], mats[i])
        return keypoints

    def transform(self, state: Dict[str, Any]) -> Dict[str, Any]:
        """Required: image (uint8 [H, W, 3]), mask (uint8 [S, H, W]), keypoints (float32 [S, M, K, 3], changed in place).
        Returned: image at ``image_size``, mask [S, Hmax, Wmax] (stage i in its ``[:H_i, :W_i]`` corner), keypoints."""
        image, mask, keypoints = state["image"], state["mask"], state["keypoints"]
        height, width = image.shape[:2]
        mats = self.matrices(self.draw(width, height))
        masks = [warp_affine_nearest_u8(mask[i], mats[i], (int(size[0]), int(size[1])))
                 for i, size in enumerate(self._transform_cfg["heatmap_sizes"])]
        self.warp_keypoints(keypoints, mats)
        image_size = self._transform_cfg["image_size"]
        image = warp_affine_linear_u8(image, mats[-1], (int(image_size[0]), int(image_size[1])))
        return dict(image=image, mask=np.stack(pad_to_same(masks)), keypoints=keypoints)


def bottomup_augment_batch(affine: BottomUpRandomAffine, flip: Optional[BottomUpHorizontalRandomFlip], images: Sequence[torch.Tensor],
                           masks: Sequence[torch.Tensor], keypoints: Sequence[np.ndarray], normalize_mean=NORMALIZE_MEAN,
                           normalize_std=NORMALIZE_STD, out: Optional[torch.Tensor] = None) -> Dict[str, Any]:
    """The two augmentations, Normalize and HWC2CHW for a batch: the device path.

    ``images[i]`` is a contiguous CUDA uint8 [H, W, 3] tensor, ``masks[i]`` the contiguous CUDA uint8 mask of the same image -
    [H, W], one plane tiled over the stages (the reference dataset without ``expand_mask``), or [S, H, W], one plane per stage (what
    ``bottomup_masks_batch`` returns; stage i is warped from plane i) -, ``keypoints[i]`` a host float32 [M_i, K, 3] array in source pixels.
    Per image, in batch order, ``affine.draw`` and then ``flip.draw()`` consume the global ``np.random`` exactly as the two
    ``transform`` s run sample by sample would; the S stage key-point sets come from the very functions ``transform`` uses, padded
    to M = max(M_i); matrices and flags are uploaded and ONE ``mp_bottomup_train_augment`` launch does the pixel work.

    Returns ``dict(image [N, 3, h, w] fp32 - ``out`` when given -, mask [N, S, Hmax, Wmax] uint8, keypoints [N, S, M, K, 3] CUDA fp32,
    num_persons [N] int32 on the host)``: ``BottomUpGenerateTarget.generate_batch(keypoints, num_persons)`` takes the last two as
    they are, ``AEMultiLoss(preds, target, mask, tag_ind)`` the mask."""
    n = len(images)
    if n == 0 or len(masks) != n or len(keypoints) != n:
        raise ValueError("one mask and one key-point array per image, at least one image")
    cfg = affine._transform_cfg
    sizes = np.asarray(cfg["heatmap_sizes"]).reshape(-1, 2)
    s = len(sizes)
    base, offs, hw, dev = source_batch(images, layout_error=ValueError)
    # [S, H, W]: S planes of H * W bytes, back to back (a 3-d tensor that is not contiguous stays 3-d and is refused as a layout)
    per_stage = [torch.is_tensor(mk) and mk.dim() == 3 and mk.is_contiguous() for mk in masks]
    mbase, moffs, _, _ = source_batch([mk.view(-1, mk.shape[2]) if st else mk for mk, st in zip(masks, per_stage)], pixel=(),
                                      layout_error=ValueError)
    if any(tuple(mk.shape) != ((s,) if st else ()) + tuple(im.shape[:2]) for im, mk, st in zip(images, masks, per_stage)):
        raise ValueError("every mask must be a contiguous uint8 [H, W] or [S, H, W] tensor of its image's size")
    lib = _lib.load()
    out_w, out_h = (int(v) for v in cfg["image_size"])
    wmax, hmax = int(sizes[:, 0].max()), int(sizes[:, 1].max())
    mats, flags, stage_kps = [], [], []
    for im, kp in zip(images, keypoints):
        kp = np.asarray(kp, dtype=np.float32)
        if kp.ndim != 3 or kp.shape[2] != 3:
            raise ValueError(f"keypoints must be [M, K, 3] per image, got {kp.shape}")
        drawn = affine.draw(int(im.shape[1]), int(im.shape[0]))
        flipped = flip.draw() if flip is not None else False
        m = affine.matrices(drawn)
        staged = affine.warp_keypoints(np.repeat(kp[None], s, axis=0), m)  # np.repeat copies: the caller's array is not changed
        if flipped:
            flip.flip_keypoints(staged)
        mats.append(m)
        flags.append(int(flipped))
        stage_kps.append(staged)
    k = stage_kps[0].shape[2]
    if any(a.shape[2] != k for a in stage_kps):
        raise ValueError("every image must have the same number of joints")
    num_persons = np.array([a.shape[1] for a in stage_kps], dtype=np.int32)
    kp_all = np.zeros((n, s, max(1, int(num_persons.max())), k, 3), np.float32)
    for i, a in enumerate(stage_kps):
        kp_all[i, :, :a.shape[1]] = a
    trans = torch.from_numpy(np.ascontiguousarray(np.stack(mats), dtype=np.float64).reshape(n, s + 1, 6)).to(dev)
    fl = None if flip is None else torch.tensor(flags, dtype=torch.int32, device=dev)
    if out is None:
        out = torch.empty(n, 3, out_h, out_w, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != (n, 3, out_h, out_w) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"out must be a contiguous CUDA fp32 {(n, 3, out_h, out_w)} tensor")
    mask_out = torch.empty(n, s, hmax, wmax, device=dev, dtype=torch.uint8)
    wh = (ctypes.c_int * (2 * s))(*[int(v) for v in sizes.reshape(-1)])
    m3, s3 = norm255(normalize_mean, normalize_std)
    if any(per_stage):  # the byte stride from one stage's source plane to the next; 0 where one plane serves every stage
        stride = torch.tensor([im.shape[0] * im.shape[1] if st else 0 for im, st in zip(images, per_stage)], dtype=torch.int64, device=dev)
        _lib.check(lib.mp_bottomup_train_augment_stages(base, _lib.ptr(offs), _lib.ptr(hw), mbase, _lib.ptr(moffs), _lib.ptr(stride),
                                                        _lib.ptr(trans), _lib.ptr(fl), wh, _lib.ptr(out), _lib.ptr(mask_out), n, s, out_h,
                                                        out_w, hmax, wmax, m3, s3, _lib.stream()), "mp_bottomup_train_augment_stages")
    else:
        _lib.check(lib.mp_bottomup_train_augment(base, _lib.ptr(offs), _lib.ptr(hw), mbase, _lib.ptr(moffs), _lib.ptr(trans), _lib.ptr(fl),
                                                 wh, _lib.ptr(out), _lib.ptr(mask_out), n, s, out_h, out_w, hmax, wmax, m3, s3,
                                                 _lib.stream()), "mp_bottomup_train_augment")
    return dict(image=out, mask=mask_out, keypoints=torch.from_numpy(kp_all).to(dev), num_persons=num_persons)


@register("transform", extra_name="bottomup_generate_target")
class BottomUpGenerateTarget(BottomUpTransform):
    """Heat maps and tag positions of every resolution level from the key points (:463-598).

    ``transform`` needs ``keypoints`` - one [M, K, 3] array per level, already in that level's pixels - and returns ``target``
    [S, K, Hmax, Wmax] fp32 (smaller levels zero-padded) and ``tag_ind`` [S, max_num, K, 2] int32 ([S, max_num, 2] without
    ``tag_per_joint``), each entry (flat index of the rounded centre, 1) or (0, 0).
    """

    def __init__(self, is_train: bool = True, config: Optional[Dict[str, Any]] = None, sigma: float = 2.0, max_num: int = 30) -> None:
        super().__init__(is_train=is_train, config=config)
        self.sigma = sigma
        self.max_num = max_num

    def transform(self, state: Dict[str, Any]) -> Dict[str, Any]:
        targets, tag_inds = [], []
        for keypoints, heatmap_size in zip(state["keypoints"], self._transform_cfg["heatmap_sizes"]):
            target, tag_ind = self._generate_heatmap_and_tag_ind(np.asarray(keypoints), heatmap_size)
            targets.append(target)
            tag_inds.append(tag_ind)
        return dict(target=np.stack(pad_to_same(targets)), tag_ind=np.stack(tag_inds))

    def _generate_heatmap_and_tag_ind(self, keypoints: np.ndarray, heatmap_size: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """One level (:527-598).  The heat map of a joint is the maximum over the persons of a (6 sigma + 1)^2 Gaussian patch
        around the joint's rounded position (Python ``round``: half to even) with the sub-pixel offset kept; a patch is skipped
        when its window misses the map; the tag index is written only when the rounded centre is inside.  The arithmetic of the
        exponent stays in the key points' float32, operation by operation, as numpy leaves a float32 scalar against Python
        numbers."""
        width, height = (int(v) for v in heatmap_size)
        num_persons, num_joints, _ = keypoints.shape
        if num_persons > self.max_num:
            raise ValueError(f"Number of persons in one image `{num_persons}` exceeds the maximum num: `{self.max_num}`")
        tag_per_joint = self._transform_cfg["tag_per_joint"]
        target = np.zeros((num_joints, height, width), dtype=np.float32)
        tag_ind = np.zeros((self.max_num, num_joints, 2) if tag_per_joint else (self.max_num, 2), dtype=np.int32)

        radius = self.sigma * 3  # 3-sigma rule
        side = 2 * radius + 1
        gx = np.arange(0, side, 1, np.float32)
        gy = gx[:, None]
        centre = side // 2
        for m in range(num_persons):
            for j in range(num_joints):
                pt = keypoints[m, j]
                if not pt[2] > 0:
                    continue
                mu_x, mu_y = round(pt[0]), round(pt[1])
                left, top = int(mu_x - radius), int(mu_y - radius)
                right, bottom = int(mu_x + radius + 1), int(mu_y + radius + 1)
                if left >= width or top >= height or right < 0 or bottom < 0:
                    continue
                cx = centre + pt[0] - mu_x
                cy = centre + pt[1] - mu_y
                patch = np.exp(-((gx - cx) ** 2 + (gy - cy) ** 2) / (2 * self.sigma**2))
                x0, x1 = max(0, left), min(right, width)
                y0, y1 = max(0, top), min(bottom, height)
                target[j, y0:y1, x0:x1] = np.maximum(target[j, y0:y1, x0:x1], patch[y0 - top:y1 - top, x0 - left:x1 - left])
                if mu_x >= width or mu_y >= height or mu_x < 0 or mu_y < 0:
                    continue
                if tag_per_joint:
                    tag_ind[m, j] = (mu_y * width + mu_x, 1)
                else:
                    tag_ind[m] = (mu_y * width + mu_x, 1)
        return target, tag_ind

    def generate_batch(self, keypoints: torch.Tensor, num_persons: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The device path: one ``mp_bottomup_target`` launch for a batch.  ``keypoints`` is CUDA fp32 [N, S, M, K, 3] (level
        ``s`` of image ``n`` in that level's pixels, rows beyond ``num_persons[n]`` ignored); returns ``target``
        [N, S, K, Hmax, Wmax] fp32 and ``tag_ind`` [N, S, max_num, K, 2] int32 ([N, S, max_num, 2] without ``tag_per_joint``)."""
        lib = _lib.load()
        if not torch.is_tensor(keypoints) or not keypoints.is_cuda:
            raise _lib.MindposeHipError("keypoints must be a CUDA tensor: the HIP path has no CPU fallback")
        sizes = np.asarray(self._transform_cfg["heatmap_sizes"]).reshape(-1, 2)
        if keypoints.dim() != 5 or keypoints.shape[1] != len(sizes) or keypoints.shape[4] != 3:
            raise ValueError(f"keypoints must be [N, S = {len(sizes)}, M, K, 3], got {tuple(keypoints.shape)}")
        n, s, m, k, _ = keypoints.shape
        counts = np.asarray(num_persons.cpu() if torch.is_tensor(num_persons) else num_persons).astype(np.int64).reshape(-1)
        if counts.shape[0] != n or (counts < 0).any() or (counts > m).any():
            raise ValueError(f"num_persons must hold one count in [0, M = {m}] per image, got {counts.tolist()}")
        if (counts > self.max_num).any():
            raise ValueError(f"Number of persons in one image `{int(counts.max())}` exceeds the maximum num: `{self.max_num}`")
        if float(self.sigma * 3).is_integer() is False:
            raise ValueError("the device path needs a whole 3 * sigma (the reference's patch and window only agree there)")
        keypoints = keypoints.float().contiguous()
        tag_per_joint = bool(self._transform_cfg["tag_per_joint"])
        wmax, hmax = int(sizes[:, 0].max()), int(sizes[:, 1].max())
        counts_dev = torch.tensor(counts, dtype=torch.int32, device=keypoints.device)
        target = torch.empty(n, s, k, hmax, wmax, device=keypoints.device, dtype=torch.float32)
        tag_shape = (n, s, self.max_num, k, 2) if tag_per_joint else (n, s, self.max_num, 2)
        tag_ind = torch.empty(tag_shape, device=keypoints.device, dtype=torch.int32)
        wh = (ctypes.c_int * (2 * s))(*[int(v) for v in sizes.reshape(-1)])
        _lib.check(lib.mp_bottomup_target(_lib.ptr(keypoints), _lib.ptr(counts_dev), wh, _lib.ptr(target), _lib.ptr(tag_ind), n, s, m, k,
                                          hmax, wmax, int(self.max_num), int(tag_per_joint), float(self.sigma), _lib.stream()),
                   "mp_bottomup_target")
        return target, tag_ind
