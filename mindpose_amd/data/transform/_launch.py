"""What every loader launch (``mp_warp_affine``, ``mp_resize_pad_normalize``, ``mp_bottomup_train_augment``) marshals the same way:
the packed uint8 sources and the Normalize constants."""
import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib


def source_batch(images: Sequence[torch.Tensor], index: Optional[Sequence[int]] = None, pixel: Tuple[int, ...] = (3,),
                 layout_error=_lib.MindposeHipError) -> Tuple[int, torch.Tensor, torch.Tensor, torch.device]:
    """The source arguments of a launch.  Every tensor of ``images`` must be a contiguous CUDA uint8 [H, W, *pixel] tensor - views
    of one buffer or separate tensors; anything not on the device is a ``MindposeHipError`` (no CPU fallback), a wrong dtype or
    layout a ``layout_error``.  Entry ``i`` of the batch is ``images[index[i]]`` (every image in order without ``index``).
    Returns (base address, byte offsets from it [n] int64, (height, width) [n, 2] int32 - both on the device -, the device)."""
    what = f"contiguous CUDA uint8 tensors [H, W{''.join(f', {c}' for c in pixel)}]"
    for im in images:
        if not torch.is_tensor(im) or not im.is_cuda:
            raise _lib.MindposeHipError(f"sources must be {what}: the HIP path has no CPU fallback")
        if im.dtype != torch.uint8 or tuple(im.shape[2:]) != tuple(pixel) or im.dim() != 2 + len(pixel) or not im.is_contiguous():
            raise layout_error(f"sources must be {what}, got {im.dtype} {tuple(im.shape)}")
    batch = list(images) if index is None else [images[i] for i in index]
    dev = images[0].device
    base = min(im.data_ptr() for im in images)
    offs = torch.tensor([im.data_ptr() - base for im in batch], dtype=torch.int64, device=dev)
    hw = torch.tensor([[im.shape[0], im.shape[1]] for im in batch], dtype=torch.int32, device=dev)
    return base, offs, hw, dev


def norm255(mean, std):
    """``mean`` and ``std`` of the 0..1 range as the kernels take them: times 255, rounded to float32, one ``float[3]`` each."""
    return tuple((ctypes.c_float * 3)(*[float(np.float32(v * 255.0)) for v in vals]) for vals in (mean, std))
