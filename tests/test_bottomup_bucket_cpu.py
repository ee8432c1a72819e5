"""Batched bottom-up evaluation, host side: the bucket key against the host transform chain, the grouping order, the datasets'
``image_size`` and the refusals of ``create_pipeline(bucket_by_shape=True)`` - none of which opens a device."""
import json
import os

import numpy as np
import pytest

import mindpose_amd as mp
from mindpose_amd.data.data_factory import bottomup_input_size, bottomup_mode, bucket_indices

CFG = dict(image_size=[512, 512], max_image_size=[832, 512], heatmap_sizes=[[128, 128], [256, 256]], pixel_std=200.0, tag_per_joint=True,
           flip_pairs=[[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]])
# (width, height): both orientations, the square, and the two one-pixel-off-square sources on either side of the pad's swap
SIZES = [(640, 480), (480, 640), (640, 640), (639, 640), (1279, 1280), (1280, 1279), (500, 375), (333, 500), (1000, 400), (64, 48)]


@pytest.mark.parametrize("w,h", SIZES)
def test_rescale_pad_key_is_the_shape_the_host_chain_returns(w, h):
    transforms = [mp.BottomUpRescale(is_train=False, config=CFG), mp.BottomUpPad(is_train=False, config=CFG)]
    assert bottomup_mode(transforms) == "rescale_pad"
    state = dict(image=np.zeros((h, w, 3), np.uint8))
    for t in transforms:  # the expectation: the host transforms' own pixels
        state.update(t.transform(state))
    assert bottomup_input_size(transforms, "rescale_pad", w, h) == (state["image"].shape[1], state["image"].shape[0])
    assert state["mask"].shape == state["image"].shape[:2]


def test_rescale_pad_key_is_no_orientation_test():
    """By hand, max (832, 512).  1279 x 1280 is portrait: the limits swap to (512, 832), 0.9992 > 0.615 -> w = 512,
    h = round(1280 * 512 / 1279) = round(512.4) = 512: a square, which pads to the LANDSCAPE shape.  639 x 640: h =
    round(640 * 512 / 639) = round(512.8) = 513 -> 512 x 513, portrait."""
    transforms = [mp.BottomUpRescale(is_train=False, config=CFG), mp.BottomUpPad(is_train=False, config=CFG)]
    assert bottomup_input_size(transforms, "rescale_pad", 1279, 1280) == (832, 512)
    assert bottomup_input_size(transforms, "rescale_pad", 639, 640) == (512, 832)
    assert bottomup_input_size(transforms, "rescale_pad", 640, 480) == (832, 512)
    assert bottomup_input_size(transforms, "rescale_pad", 480, 640) == (512, 832)


@pytest.mark.parametrize("w,h", SIZES)
def test_resize_key_is_the_shape_the_host_transform_returns(w, h):
    t = mp.BottomUpResize(is_train=False, config=CFG, size=128, base_length=32)  # (a small target: the host warp is a numpy loop)
    assert bottomup_mode([t]) == "resize"
    image = t.transform(dict(image=np.zeros((h, w, 3), np.uint8)))["image"]
    assert bottomup_input_size([t], "resize", w, h) == (image.shape[1], image.shape[0])


def test_mode_of_other_lists_is_host():
    rescale, pad = mp.BottomUpRescale(is_train=False, config=CFG), mp.BottomUpPad(is_train=False, config=CFG)
    assert bottomup_mode([rescale]) == "host" and bottomup_mode([pad, rescale]) == "host" and bottomup_mode([]) == "host"
    assert bottomup_mode([rescale, pad], normalize=False) == "host" and bottomup_mode([rescale, pad], hwc_to_chw=False) == "host"
    with pytest.raises(ValueError):
        bottomup_input_size([rescale], "host", 640, 480)


# ---- the grouping ---------------------------------------------------------------------------------------------------------------
#        index: 0    1    2    3    4    5    6    7    8    9    10
_KEYS = ["L", "P", "L", "L", "P", "L", "L", "P", "L", "P", "P"]


def _group(order, batch_size, keys=_KEYS):
    return list(bucket_indices(order, lambda i: (i, 0), lambda w, h: keys[w], batch_size))


def test_grouping_emits_full_lists_as_they_fill_and_partials_in_first_pending_order():
    # walk 0..10, batch 3: L fills at 3 -> [0, 2, 3]; P fills at 7 -> [1, 4, 7]; L fills at 8 -> [5, 6, 8]; left: P [9, 10]
    assert _group(range(11), 3) == [[0, 2, 3], [1, 4, 7], [5, 6, 8], [9, 10]]
    # batch 4: L fills at 5 -> [0, 2, 3, 5]; P fills at 9 -> [1, 4, 7, 9]; the partials: L's first pending index 6 came before P's 10
    assert _group(range(11), 4) == [[0, 2, 3, 5], [1, 4, 7, 9], [6, 8], [10]]
    # a hand-written order: P [10, 9, 7] fills first; the partials L [0, 8] (pending since position 3) before P [4] (position 5)
    assert _group([10, 9, 7, 0, 8, 4], 3) == [[10, 9, 7], [0, 8], [4]]
    # after a key was emitted its NEXT pending list is younger than the other key's: P [1] (position 1) before L [5] (position 4)
    assert _group([0, 1, 2, 3, 5], 3) == [[0, 2, 3], [1], [5]]


@pytest.mark.parametrize("batch_size", [1, 2, 3, 4, 16])
def test_grouping_keeps_every_index_once_and_is_deterministic(batch_size):
    order = np.random.RandomState(batch_size).permutation(11)
    groups = _group(order, batch_size)
    assert sorted(i for g in groups for i in g) == list(range(11))
    assert all(1 <= len(g) <= batch_size and len({_KEYS[i] for i in g}) == 1 for g in groups)
    assert all(isinstance(i, int) for g in groups for i in g)
    assert groups == _group(order, batch_size)  # a second call: the same lists
    assert sum(len(g) < batch_size for g in groups) <= 2  # at most one partial list per key
    if batch_size == 1:
        assert groups == [[int(i)] for i in order]  # the input order
    with pytest.raises(ValueError):
        _group(order, 0)


# ---- datasets -------------------------------------------------------------------------------------------------------------------
_IMAGES = [dict(id=7, file_name="b.png", width=64, height=48), dict(id=3, file_name="a.png", width=48, height=64),
           dict(id=9, file_name="c.png", width=50, height=37), dict(id=4, file_name="d.png", width=63, height=64),
           dict(id=5, file_name="e.png", width=40, height=40)]


def _write_folder(tmp_path, images=_IMAGES):
    from PIL import Image
    for im in images:
        Image.fromarray(np.zeros((im["height"], im["width"], 3), np.uint8)).save(os.path.join(tmp_path, im["file_name"]))
    ann = os.path.join(tmp_path, "ann.json")
    with open(ann, "w") as f:
        json.dump(dict(images=images, annotations=[], categories=[dict(id=1, name="person")]), f)
    return ann


def test_coco_image_size_comes_from_the_annotation_file(tmp_path):
    # the json alone answers: declared sizes that no file on disk has
    images = [dict(im, width=im["width"] * 10, height=im["height"] * 10) for im in _IMAGES]
    ann = _write_folder(tmp_path)
    with open(ann, "w") as f:
        json.dump(dict(images=images, annotations=[], categories=[]), f)
    ds = mp.COCOBottomUpDataset(str(tmp_path), ann, is_train=False)
    want = [(im["width"], im["height"]) for im in images]
    assert [ds.image_size(i) for i in range(len(ds))] == want and all(isinstance(v, int) for v in ds.image_size(0))
    ds.lazy_image = True
    assert [ds.image_size(i) for i in range(len(ds))] == want


def test_imagefolder_image_size_comes_from_the_file_header(tmp_path):
    _write_folder(tmp_path)
    with open(os.path.join(tmp_path, "n.jpg"), "wb") as f:  # a .npy payload, which the codec accepts as well
        np.save(f, np.zeros((30, 70, 3), np.uint8))
    sizes = {im["file_name"]: (im["width"], im["height"]) for im in _IMAGES}
    sizes["n.jpg"] = (70, 30)
    ds = mp.ImageFolderBottomUpDataset(str(tmp_path))
    assert len(ds) == 6

    def answers():
        return {os.path.basename(ds[i][4]): ds.image_size(i) for i in range(len(ds))}

    assert answers() == sizes
    ds.lazy_image = True
    assert answers() == sizes
    # cached per index: the files are not opened again
    for name in sizes:
        os.remove(os.path.join(tmp_path, name))
    assert [ds.image_size(i) for i in range(len(ds))] == [sizes[os.path.basename(ds._dataset[i]["image_file"])] for i in range(len(ds))]
    with pytest.raises(NotImplementedError):
        mp.BottomUpDataset.image_size(ds, 0)


def test_each_shard_groups_its_own_indices(tmp_path):
    ann = _write_folder(tmp_path)
    transforms = [mp.BottomUpRescale(is_train=False, config=CFG), mp.BottomUpPad(is_train=False, config=CFG)]

    def key_of(w, h):
        return bottomup_input_size(transforms, "rescale_pad", w, h)

    # by the transforms: b 64x48 L, a 48x64 P, c 50x37 L, d 63x64 -> 512 x 520 P, e 40x40 L
    whole = mp.create_dataset(str(tmp_path), ann, dataset_format="coco_bottomup", is_train=False)
    assert list(bucket_indices(whole.indices(), whole.source.image_size, key_of, 2)) == [[0, 2], [1, 3], [4]]
    shards = [mp.create_dataset(str(tmp_path), ann, dataset_format="coco_bottomup", is_train=False, device_num=2, rank_id=r) for r in (0, 1)]
    assert [s.indices().tolist() for s in shards] == [[0, 2, 4], [1, 3, 0]]  # (the second shard wraps to the head of the order)
    got = [list(bucket_indices(s.indices(), s.source.image_size, key_of, 2)) for s in shards]
    assert got == [[[0, 2], [4]], [[1, 3], [0]]]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_device_call(tmp_path, monkeypatch):
    import torch

    def no_device(*args, **kwargs):
        raise AssertionError("a device call before the refusal")

    for name in ("current_device", "is_available", "init", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, no_device)
    ann = _write_folder(tmp_path)
    ds = mp.create_dataset(str(tmp_path), ann, dataset_format="coco_bottomup", is_train=False)
    recipe = ["bottomup_rescale", "bottomup_pad"]
    with pytest.raises(ValueError, match="bottom-up training data is not implemented"):
        mp.create_pipeline(ds, recipe, method="bottomup", is_train=True, config=CFG, bucket_by_shape=True)
    for method in ("topdown",):
        with pytest.raises(ValueError, match="bucket_by_shape"):
            mp.create_pipeline(ds, ["topdown_affine"], method=method, is_train=False, config=CFG, bucket_by_shape=True)
    for transforms, kwargs in ((["bottomup_rescale"], {}), (["bottomup_pad", "bottomup_rescale"], {}), ([], {}),
                               (recipe, dict(normalize=False)), (recipe, dict(hwc_to_chw=False)),
                               ([{"bottomup_resize": dict(size=128)}], dict(normalize=False))):
        for method in ("bottomup", "imagefolder_bottomup"):
            with pytest.raises(ValueError, match="bucket_by_shape"):
                mp.create_pipeline(ds, transforms, method=method, batch_size=4, is_train=False, config=CFG, bucket_by_shape=True, **kwargs)
