"""CPU-side checks of what the three loader launches share on the host: the source marshaller and the Normalize constants
(``data/transform/_launch.py``) and the fixed-point coordinate grids of the two host warps (``bottomup_transform._warp_coords``)."""
import numpy as np
import pytest
import torch

from mindpose_amd import _lib
from mindpose_amd.data.transform._launch import norm255, source_batch
from mindpose_amd.data.transform.bottomup_transform import _warp_coords, warp_affine_linear_u8, warp_affine_nearest_u8


def test_source_batch_refuses_cpu_tensors_whatever_else_is_wrong():
    for bad in (torch.zeros(4, 5, 3, dtype=torch.uint8), torch.zeros(4, 5, 3), np.zeros((4, 5, 3), np.uint8)):
        for layout_error in (_lib.MindposeHipError, ValueError):  # the class of the layout errors does not change this one
            with pytest.raises(_lib.MindposeHipError):
                source_batch([bad], layout_error=layout_error)
    with pytest.raises(_lib.MindposeHipError):
        source_batch([torch.zeros(4, 5, dtype=torch.uint8)], pixel=())


@pytest.fixture
def on_device(monkeypatch):
    """Host tensors that claim to live on the device: the layout checks and the tables behind the device check run here."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)


@pytest.mark.parametrize("layout_error", [_lib.MindposeHipError, ValueError])  # the two launchers / bottomup_augment_batch
def test_source_batch_refuses_dtype_view_and_channels(on_device, layout_error):
    good = torch.zeros(6, 8, 3, dtype=torch.uint8)
    source_batch([good], layout_error=layout_error)
    for bad in (torch.zeros(6, 8, 3, dtype=torch.float32), torch.zeros(6, 8, 3, dtype=torch.int8), good[:, ::2], good.permute(1, 0, 2),
                torch.zeros(6, 8, 4, dtype=torch.uint8), torch.zeros(6, 8, dtype=torch.uint8), torch.zeros(2, 6, 8, 3, dtype=torch.uint8)):
        with pytest.raises(layout_error):
            source_batch([good, bad], layout_error=layout_error)
    # the [H, W] variant, of the masks
    mask = torch.zeros(6, 8, dtype=torch.uint8)
    source_batch([mask], pixel=())
    for bad in (good, mask.bool(), mask[:, ::2], torch.zeros(8, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            source_batch([mask, bad], pixel=(), layout_error=ValueError)


def test_source_batch_tables(on_device):
    buf = torch.zeros(13 * 9 * 3 + 7 * 11 * 3, dtype=torch.uint8)
    a, b = buf[:13 * 9 * 3].view(13, 9, 3), buf[13 * 9 * 3:].view(7, 11, 3)
    for images in ([a, b], [b, a]):  # the base is the lowest address, wherever it stands in the list
        base, offs, hw, dev = source_batch(images)
        assert base == buf.data_ptr() and dev == buf.device
        assert offs.dtype == torch.int64 and offs.tolist() == [im.data_ptr() - base for im in images]
        assert hw.dtype == torch.int32 and hw.tolist() == [list(im.shape[:2]) for im in images]
    base, offs, hw, _ = source_batch([a, b], index=[1, 1, 0])
    assert base == buf.data_ptr() and offs.tolist() == [13 * 9 * 3, 13 * 9 * 3, 0] and hw.tolist() == [[7, 11], [7, 11], [13, 9]]
    other = torch.zeros(5, 4, 3, dtype=torch.uint8)  # a separate allocation: offsets are signed
    base, offs, _, _ = source_batch([a, other], index=[1])
    assert base == min(a.data_ptr(), other.data_ptr()) and base + offs.item() == other.data_ptr()


def test_norm255_is_the_float32_of_the_product():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.255)
    m3, s3 = norm255(mean, std)
    assert len(m3) == len(s3) == 3
    for got, vals in ((m3, mean), (s3, std)):
        for g, v in zip(got, vals):
            assert np.float32(g) == np.float32(v * 255) and g == float(np.float32(v * 255))


# What warp_affine_linear_u8 / warp_affine_nearest_u8 returned for these inputs before _warp_coords existed (each warp built its
# grids itself), output 5 x 4.  The mask's value is its flat source index + 1, so the nearest result IS the coordinate grid.
_IMAGE = (np.arange(7 * 9, dtype=np.int64) * 37 % 251).astype(np.uint8).reshape(7, 9, 1)
_MASK = (np.arange(7 * 9) + 1).astype(np.uint8).reshape(7, 9)
_CASES = [
    (np.array([[1.14, -0.62, 1.75], [0.62, 1.14, -2.25]]),  # rotation + scale, inside the source
     [[116, 160, 155, 150, 143], [233, 147, 199, 213, 146], [126, 47, 96, 124, 33], [120, 117, 111, 106, 100]],
     [[19, 19, 11, 12, 12], [28, 20, 20, 21, 13], [37, 29, 30, 21, 22], [38, 38, 30, 31, 31]]),
    (np.array([[0.6, 0.2, -1.5], [-0.1, 0.7, 2.5]]),  # shear + translation, partly outside
     [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [64, 137, 193, 50, 3], [163, 179, 67, 147, 96]],
     [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [4, 5, 7, 8, 0], [12, 14, 15, 26, 0]]),
]


@pytest.mark.parametrize("trans,linear,nearest", _CASES)
def test_warp_coords_reproduces_both_host_warps(trans, linear, nearest):
    assert np.array_equal(warp_affine_linear_u8(_IMAGE, trans, (5, 4))[..., 0], np.array(linear, np.uint8))
    assert np.array_equal(warp_affine_nearest_u8(_MASK, trans, (5, 4)), np.array(nearest, np.uint8))
    # the nearest grid straight from the function
    x, y = _warp_coords(trans, (5, 4), 512, 10)
    assert x.shape == y.shape == (4, 5) and x.dtype == y.dtype == np.int64
    inside = (x >= 0) & (x < 9) & (y >= 0) & (y < 7)
    assert np.array_equal(np.where(inside, y * 9 + x + 1, 0), np.array(nearest))
    # both grids are one 1 / 1024 coordinate under their own round delta and shift
    tx, ty = _warp_coords(trans, (5, 4), 0, 0)
    bx, by = _warp_coords(trans, (5, 4), 16, 5)
    assert np.array_equal(x, (tx + 512) >> 10) and np.array_equal(y, (ty + 512) >> 10)
    assert np.array_equal(bx, (tx + 16) >> 5) and np.array_equal(by, (ty + 16) >> 5)
