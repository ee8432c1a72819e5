"""CPU-side checks of the bottom-up train-time augmentations (mindpose/data/transform/bottomup_transform.py:88-140, :304-460):
registry names and constructor defaults as the reference declares them, the host ``transform`` s against what the reference's own
classes did under fixed seeds (tests/golden/bottomup_augment.npz: matrices, key points, masks, the generator's next draw),
``warp_affine_nearest_u8`` on answers that follow from its formula, and the argument validation of ``mp_bottomup_train_augment``
(it runs before any HIP call)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import mindpose_amd as mp
from mindpose_amd import _lib
from mindpose_amd.data.transform.bottomup_transform import warp_affine_nearest_u8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bottomup_augment.npz")


def _params(fn):
    return [(k, v.default) for k, v in list(inspect.signature(fn).parameters.items())[1:]]


def _cfg(image_size=(64, 48), heatmap_sizes=((16, 12), (32, 24)), flip_pairs=((1, 2), (3, 4))):
    return dict(image_size=[int(v) for v in image_size], max_image_size=[int(v) for v in image_size],
                heatmap_sizes=[[int(v) for v in s] for s in heatmap_sizes], flip_pairs=[list(p) for p in flip_pairs], pixel_std=200.0,
                tag_per_joint=True)


def test_registry_names_exports_and_defaults():
    for name, cls in (("BottomUpRandomAffine", mp.BottomUpRandomAffine), ("bottomup_random_affine", mp.BottomUpRandomAffine),
                      ("BottomUpHorizontalRandomFlip", mp.BottomUpHorizontalRandomFlip),
                      ("bottomup_horizontal_random_flip", mp.BottomUpHorizontalRandomFlip)):
        assert mp.entrypoint("transform", name) is cls, name
        assert issubclass(cls, mp.BottomUpTransform)
    assert callable(mp.bottomup_augment_batch)
    assert _params(mp.BottomUpRandomAffine.__init__) == [("is_train", True), ("config", None), ("rot_factor", 30.0),
                                                         ("scale_factor", (0.75, 1.5)), ("scale_type", "short"), ("trans_factor", 40.0)]
    assert _params(mp.BottomUpHorizontalRandomFlip.__init__) == [("is_train", True), ("config", None), ("flip_prob", 0.5)]
    t = mp.BottomUpRandomAffine(config=_cfg())
    assert (t.max_rotation, t.min_scale, t.max_scale, t.scale_type, t.trans_factor) == (30.0, 0.75, 1.5, "short", 40.0)
    with pytest.raises(KeyError):  # the required config keys are the base class's
        mp.BottomUpRandomAffine(config=dict(image_size=[64, 48]))
    with pytest.raises(KeyError):
        mp.BottomUpHorizontalRandomFlip(config=dict(image_size=[64, 48]))


def _cases():
    z = np.load(GOLDEN)
    for i in range(int(z["num_cases"])):
        yield i, {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"c{i}/")}


def _transforms(g):
    cfg = _cfg(g["image_size"], g["heatmap_sizes"])
    affine = mp.BottomUpRandomAffine(is_train=True, config=cfg, rot_factor=float(g["rot_factor"]), scale_factor=tuple(g["scale_factor"].tolist()),
                                     scale_type=str(g["scale_type"]), trans_factor=float(g["trans_factor"]))
    return affine, mp.BottomUpHorizontalRandomFlip(is_train=True, config=cfg, flip_prob=float(g["flip_prob"]))


def test_fixture_covers_the_listed_cases():
    cases = [g for _, g in _cases()]
    sources = {tuple(g["source_wh"].tolist()) for g in cases}
    assert any(w > h for w, h in sources) and any(w < h for w, h in sources) and any(w % 2 and h % 2 for w, h in sources)
    assert {str(g["scale_type"]) for g in cases} == {"short", "long"}
    assert {float(g["trans_factor"]) for g in cases} == {0.0, 40.0}
    assert {0.0, 1.0} <= {float(g["flip_prob"]) for g in cases}
    assert {bool(g["flipped"]) for g in cases} == {True, False}
    assert any(g["keypoints_in"].shape[0] == 0 for g in cases) and any(g["keypoints_in"].shape[0] > 1 for g in cases)
    assert all(g["mask_in"].shape[0] <= 64 and g["mask_in"].shape[1] <= 64 and g["mask_in"].size <= 64 * 48 for g in cases)
    assert all(g["warp_flags"].tolist() == [0] * (len(g["warp_flags"]) - 1) + [1] for g in cases)  # INTER_NEAREST per stage, then INTER_LINEAR
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_host_transforms_equal_the_reference_on_every_fixture_case():
    rng = np.random.RandomState(3)
    for i, g in _cases():
        affine, flip = _transforms(g)
        seed, (w, h), s = int(g["seed"]), g["source_wh"].tolist(), len(g["heatmap_sizes"])
        # the draw on its own, then the matrices: what the reference handed to warpAffine, in its order (stages, then the image)
        np.random.seed(seed)
        mats = affine.matrices(affine.draw(w, h))
        assert mats.dtype == np.float64 and mats.shape == (s + 1, 2, 3)
        assert np.array_equal(mats, g["matrices"]), (i, np.abs(mats - g["matrices"]).max())
        sizes = [[int(v) for v in size] for size in g["heatmap_sizes"]] + [[int(v) for v in g["image_size"]]]
        assert g["warp_sizes"].tolist() == sizes
        # the two transforms as the pipeline would chain them
        np.random.seed(seed)
        image = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        state = dict(image=image, mask=np.repeat(g["mask_in"][None], s, axis=0), keypoints=np.repeat(g["keypoints_in"][None], s, axis=0))
        state.update(affine.transform(state))
        assert state["keypoints"].dtype == np.float32 and np.array_equal(state["keypoints"], g["keypoints_affine"]), i
        assert state["mask"].dtype == np.uint8 and np.array_equal(state["mask"], g["mask_affine"]), i
        assert state["image"].shape == tuple(g["image_shape"]) and state["image"].dtype == np.uint8
        warped = state["image"].copy()
        state.update(flip.transform(state))
        assert np.array_equal(state["keypoints"], g["keypoints"]), i
        assert np.array_equal(state["mask"], g["mask"]), i
        assert np.array_equal(state["image"], warped[:, ::-1] if g["flipped"] else warped), i
        assert np.random.rand() == float(g["next_draw"]), i  # the generator was consumed exactly as the reference consumes it


def test_draw_order_and_translation_switch():
    """uniform(scale), uniform(rot), then randint dx, dy only with a positive trans_factor - replayed by hand."""
    for trans in (0.0, 40.0):
        t = mp.BottomUpRandomAffine(config=_cfg(), trans_factor=trans)
        np.random.seed(5)
        d = t.draw(61, 33)
        np.random.seed(5)
        scale = np.array([61, 33], np.float32)
        scale *= np.random.uniform(0.75, 1.5)
        rot = np.random.uniform(-30.0, 30.0)
        center = np.array((61 / 2, 33 / 2))
        if trans > 0:
            center[0] += np.random.randint(-trans * scale[0] / 200.0, trans * scale[0] / 200.0)
            center[1] += np.random.randint(-trans * scale[1] / 200.0, trans * scale[1] / 200.0)
        assert d["img_scale"].dtype == np.float32 and np.array_equal(d["img_scale"], scale)
        assert d["rot"] == rot and np.array_equal(d["center"], center)
        assert sorted(d) == ["center", "img_scale", "rot"]


def test_unknown_scale_type_raises():
    t = mp.BottomUpRandomAffine(config=_cfg(), scale_type="diag")
    state = dict(image=np.zeros((20, 30, 3), np.uint8), mask=np.ones((2, 20, 30), np.uint8), keypoints=np.zeros((2, 1, 5, 3), np.float32))
    with pytest.raises(ValueError, match="Unknown scale type"):
        t.transform(state)
    with pytest.raises(ValueError, match="Unknown scale type"):
        t._get_scale((30.0, 20.0), (16, 12))
    for scale_type, want in (("short", [26.666666, 20.0]), ("long", [30.0, 22.5])):  # 30 / 16 > 20 / 12: "short" fits the height (a crop), "long" the width
        got = mp.BottomUpRandomAffine(config=_cfg(), scale_type=scale_type)._get_scale((30.0, 20.0), (16, 12))
        assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-6)


# ---- warp_affine_nearest_u8 on answers that follow from the formula ----------------------------------------------------------------

def _mask(h, w, seed=0):
    return np.random.RandomState(seed).randint(1, 256, (h, w)).astype(np.uint8)  # no zero: the border shows


def test_nearest_warp_identity_translation_rotation_outside():
    m = _mask(7, 11)
    eye = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert np.array_equal(warp_affine_nearest_u8(m, eye, (11, 7)), m)
    # identity into a larger output: the copy in the corner, zero beyond the source
    big = warp_affine_nearest_u8(m, eye, (13, 9))
    assert np.array_equal(big[:7, :11], m) and not big[7:].any() and not big[:, 11:].any()
    # integer translation: dst(x, y) = src(x - 3, y + 2), zero where that leaves the source
    shifted = warp_affine_nearest_u8(m, np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0]]), (11, 7))
    want = np.zeros_like(m)
    want[:5, 3:] = m[2:, :8]
    assert np.array_equal(shifted, want)
    # exact quarter turn of a non-square mask: forward (x, y) -> (H - 1 - y, x), so dst[y', x'] = src[H - 1 - x', y'] - a permutation
    rot = warp_affine_nearest_u8(m, np.array([[0.0, -1.0, 6.0], [1.0, 0.0, 0.0]]), (7, 11))
    assert rot.shape == (11, 7) and np.array_equal(rot, m[::-1].T)
    assert sorted(rot.reshape(-1).tolist()) == sorted(m.reshape(-1).tolist())
    # everything maps outside: all zero (a far translation, and a source coordinate that saturates int16)
    assert not warp_affine_nearest_u8(m, np.array([[1.0, 0.0, 500.0], [0.0, 1.0, 0.0]]), (11, 7)).any()
    assert not warp_affine_nearest_u8(m, np.array([[1.0, 0.0, -1e6], [0.0, 1.0, 0.0]]), (11, 7)).any()
    assert not warp_affine_nearest_u8(m, np.array([[1.0, 0.0, 1e6], [0.0, 1.0, 1e6]]), (11, 7)).any()
    # a halving: X = (x * 2048 + 512) >> 10 = 2 x exactly
    assert np.array_equal(warp_affine_nearest_u8(m, np.array([[0.5, 0.0, 0.0], [0.0, 0.5, 0.0]]), (5, 3)), m[0:6:2, 0:10:2])
    with pytest.raises(ValueError):
        warp_affine_nearest_u8(m.astype(np.float32), eye, (11, 7))


def test_nearest_warp_rounds_half_up_in_fixed_point():
    """The + 512 before the >> 10 is a round-half-up of the 1 / 1024 coordinate: a shift of 0.5 pixel takes the NEXT source pixel,
    one of 0.5 - 1 / 1024 still this one."""
    m = _mask(1, 9)
    half = warp_affine_nearest_u8(m, np.array([[1.0, 0.0, -0.5], [0.0, 1.0, 0.0]]), (9, 1))  # source x = x' + 0.5
    assert np.array_equal(half[0, :8], m[0, 1:]) and half[0, 8] == 0
    below = warp_affine_nearest_u8(m, np.array([[1.0, 0.0, -0.5 + 1.0 / 1024], [0.0, 1.0, 0.0]]), (9, 1))
    assert np.array_equal(below, m)


def test_flip_leaves_the_mask_padding_untouched():
    cfg = _cfg(image_size=(48, 48), heatmap_sizes=((24, 8), (12, 20)))
    flip = mp.BottomUpHorizontalRandomFlip(config=cfg, flip_prob=1.0)
    rng = np.random.RandomState(1)
    mask = rng.randint(0, 256, (2, 20, 24)).astype(np.uint8)  # the padding holds marks that must not move
    before = mask.copy()
    kp = np.concatenate([rng.uniform(0, 12, (2, 2, 5, 2)), np.ones((2, 2, 5, 1))], axis=3).astype(np.float32)
    kp_before = kp.copy()
    image = rng.randint(0, 256, (48, 48, 3)).astype(np.uint8)
    out = flip.transform(dict(image=image, mask=mask, keypoints=kp))
    assert out["mask"] is mask and out["keypoints"] is kp  # in place, as the reference
    assert np.array_equal(mask[0, :8, :24], before[0, :8, ::-1]) and np.array_equal(mask[0, 8:], before[0, 8:])
    assert np.array_equal(mask[1, :20, :12], before[1, :20, 11::-1]) and np.array_equal(mask[1, :, 12:], before[1, :, 12:])
    assert np.array_equal(out["image"], image[:, ::-1])
    index = [0, 2, 1, 4, 3]
    for i, width in enumerate((24, 12)):
        assert np.array_equal(kp[i, ..., 0], np.float32(width - 1) - kp_before[i][:, index, 0])
        assert np.array_equal(kp[i, ..., 1:], kp_before[i][:, index, 1:])
    # flip_prob 0 draws and changes nothing
    np.random.seed(2)
    same = mp.BottomUpHorizontalRandomFlip(config=cfg, flip_prob=0.0).transform(dict(image=image, mask=mask, keypoints=kp))
    assert same["image"] is image
    np.random.seed(2)
    np.random.rand()
    nxt = np.random.rand()
    np.random.seed(2)
    assert mp.BottomUpHorizontalRandomFlip(config=cfg, flip_prob=0.0).draw() is False and np.random.rand() == nxt


def test_batch_function_refuses_cpu_tensors():
    cfg = _cfg()
    affine, flip = mp.BottomUpRandomAffine(config=cfg), mp.BottomUpHorizontalRandomFlip(config=cfg)
    with pytest.raises(_lib.MindposeHipError):
        mp.bottomup_augment_batch(affine, flip, [torch.zeros(20, 30, 3, dtype=torch.uint8)], [torch.ones(20, 30, dtype=torch.uint8)],
                                  [np.zeros((1, 5, 3), np.float32)])
    with pytest.raises(ValueError):
        mp.bottomup_augment_batch(affine, flip, [], [], [])


def test_entry_point_validates_before_any_hip_call():
    lib = _lib.load()
    P = 4096  # a non-null address: validation must answer before anything dereferences or launches
    wh = (ctypes.c_int * 4)(16, 12, 32, 24)
    m3, s3 = (ctypes.c_float * 3)(120.0, 110.0, 100.0), (ctypes.c_float * 3)(58.0, 57.0, 65.0)

    def call(src=P, offs=P, hw=P, msrc=P, moffs=P, trans=P, flip=None, sizes=wh, image=P, mask=P, n=2, s=2, out_h=48, out_w=64, hmax=24,
             wmax=32, mean=m3, std=s3):
        return lib.mp_bottomup_train_augment(src, offs, hw, msrc, moffs, trans, flip, sizes, image, mask, n, s, out_h, out_w, hmax, wmax,
                                             mean, std, None)

    for kw in (dict(src=None), dict(offs=None), dict(hw=None), dict(msrc=None), dict(moffs=None), dict(trans=None), dict(sizes=None),
               dict(image=None), dict(mask=None), dict(mean=None), dict(std=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(s=0), dict(s=9), dict(s=-1)):
        assert call(**kw) == _lib.MP_ERR_UNSUPPORTED, kw
    for kw in (dict(wmax=31), dict(hmax=23), dict(sizes=(ctypes.c_int * 4)(16, 12, 33, 24)), dict(sizes=(ctypes.c_int * 4)(16, 0, 32, 24)),
               dict(sizes=(ctypes.c_int * 4)(-16, 12, 32, 24)), dict(n=0), dict(n=65536), dict(out_h=0), dict(out_w=-4), dict(hmax=0),
               dict(wmax=0), dict(std=(ctypes.c_float * 3)(58.0, 0.0, 65.0))):
        assert call(**kw) == -2, kw
    assert "mp_bottomup_train_augment" in _lib.EXPORTED_SYMBOLS
