"""Bottom-up evaluation, host side: columns and registry, the geometry of the rescale / resize / pad transforms, the fixed-point
resize restatement on known answers (cv2 is not installed: every expected value below is derived from the formula), the COCO
bottom-up dataset on a synthetic annotation file and ``BottomUpEvaluator`` on hand-built records."""
import inspect
import json
import os

import numpy as np
import pytest

import mindpose_amd as mp
from mindpose_amd.data.column_names import COLUMN_MAP, FINAL_COLUMN_MAP
from mindpose_amd.data.transform.bottomup_transform import resize_linear_u8
from mindpose_amd.register import entrypoint

CFG = dict(image_size=[512, 512], max_image_size=[832, 512], heatmap_sizes=[[128, 128], [256, 256]], pixel_std=200.0, tag_per_joint=True,
           flip_pairs=[[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]])
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.255)


def _defaults(cls):
    return {k: v.default for k, v in inspect.signature(cls.__init__).parameters.items() if k != "self"}


def test_registry_columns_and_constructor_defaults():
    val = ["image", "mask", "center", "scale", "image_file", "image_shape"]
    for key in ("coco_bottomup", "bottomup", "imagefolder_bottomup"):
        assert COLUMN_MAP[key]["val"] == val
    for key in ("bottomup", "imagefolder_bottomup"):
        assert FINAL_COLUMN_MAP[key]["val"] == val
    assert "train" not in COLUMN_MAP["imagefolder_bottomup"]
    assert entrypoint("transform", "bottomup_rescale") is mp.BottomUpRescale
    assert entrypoint("transform", "bottomup_resize") is mp.BottomUpResize
    assert entrypoint("transform", "bottomup_pad") is mp.BottomUpPad
    assert entrypoint("dataset", "coco_bottomup") is mp.COCOBottomUpDataset
    assert entrypoint("dataset", "imagefolder_bottomup") is mp.ImageFolderBottomUpDataset
    assert entrypoint("evaluator", "bottomup") is mp.BottomUpEvaluator
    # the reference's constructor defaults (bottomup_transform.py, dataset/bottomup.py:34-41, bottomup_evaluator.py:36-44)
    assert _defaults(mp.BottomUpRescale) == dict(is_train=True, config=None)
    assert _defaults(mp.BottomUpPad) == dict(is_train=True, config=None)
    assert _defaults(mp.BottomUpResize) == dict(is_train=True, config=None, size=512, base_length=64)
    assert _defaults(mp.COCOBottomUpDataset) == dict(image_root=inspect.Parameter.empty, annotation_file=None, is_train=False,
                                                      num_joints=17, config=None)
    assert _defaults(mp.BottomUpEvaluator) == dict(annotation_file=inspect.Parameter.empty, metric="AP", num_joints=17, config=None,
                                                    remove_result_file=True, result_path="./result_keypoints.json")
    with pytest.raises(KeyError):
        mp.BottomUpRescale(is_train=False, config=dict(image_size=[512, 512]))  # the config keys are required, as in the reference


def test_rescale_geometry_known_answers():
    """_get_new_size by hand from bottomup_transform.py:152-168 with max (832, 512):
      (640, 480): landscape, 640/480 = 1.333 <= 832/512 = 1.625 -> h = 512, w = round(640 * 512 / 480) = round(682.67) = 683
      (480, 640): portrait, the limits swap to (512, 832); 0.75 > 512/832 = 0.615 -> w = 512, h = round(640 * 512 / 480) = 683
      (1000, 400): 2.5 > 1.625 -> w = 832, h = round(400 * 832 / 1000) = round(332.8) = 333
      (500, 500): not w < h; 1.0 <= 1.625 -> h = 512, w = round(500 * 512 / 500) = 512"""
    t = mp.BottomUpRescale(is_train=False, config=CFG)
    for (w, h), want in (((640, 480), (683, 512)), ((480, 640), (512, 683)), ((1000, 400), (832, 333)), ((500, 500), (512, 512))):
        got = t._get_new_size((w, h), (832, 512))
        assert got == want and all(isinstance(v, int) for v in got)
    out = t.transform(dict(image=np.zeros((375, 501, 3), np.uint8)))
    assert set(out) == {"image", "center", "scale", "image_shape"}
    # center = [round(w / 2), round(h / 2)] with Python's round (half to even): 250.5 -> 250, 187.5 -> 188
    assert out["center"].tolist() == [250, 188]
    assert out["scale"].tolist() == [501 / 200.0, 375 / 200.0]
    assert out["image_shape"] == (684, 512) and out["image"].shape == (512, 684, 3)  # round(501 * 512 / 375) = round(684.03)


def test_resize_geometry_known_answers():
    """bottomup_transform.py:238-263 with size 512, base_length 64: min_size = 512;
      (640, 480): h = 512, w = ceil(512 / 480 * 640 / 64) * 64 = ceil(10.67) * 64 = 704; scale = (704 / 512 * 480 / 200, 480 / 200)
      (480, 640): w = 512, h = ceil(512 / 480 * 640 / 64) * 64 = 704; scale = (480 / 200, 704 / 512 * 480 / 200)"""
    t = mp.BottomUpResize(is_train=False, config=CFG, size=512, base_length=64)
    size, center, scale = t._get_new_size((640, 480), 512, base_length=64, pixel_std=200.0)
    assert size == (704, 512) and center.tolist() == [320, 240] and scale.tolist() == [704 / 512 * 480 / 200, 480 / 200]
    size, center, scale = t._get_new_size((480, 640), 512, base_length=64, pixel_std=200.0)
    assert size == (512, 704) and center.tolist() == [240, 320] and scale.tolist() == [480 / 200, 704 / 512 * 480 / 200]
    out = t.transform(dict(image=np.full((48, 64, 3), 200, np.uint8)))
    assert set(out) == {"image", "mask", "center", "scale", "image_shape"}
    assert out["image_shape"] == (704, 512) and out["image"].shape == (512, 704, 3) and out["mask"].shape == (512, 704)
    assert out["mask"].dtype == np.uint8 and out["mask"].all()
    assert (out["image"][100:400, 100:600] == 200).all()  # the interior of a constant image stays constant under the warp


def test_host_resize_known_answers():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (24, 36, 3)).astype(np.uint8)
    # same size: f = (float)((d + 0.5) * 1 - 0.5) = d exactly -> s = d, f = 0 -> coefficients (2048, 0) on both axes:
    # r = 2048 * S; (2048 * ((2048 * S) >> 4)) >> 16 = (2048 * 128 * S) >> 16 = 4 * S; (4 * S + 0 + 2) >> 2 = S
    assert np.array_equal(resize_linear_u8(img, (36, 24)), img)
    # constant image c where every f lies on the 2^-11 grid, so that a0 + a1 = b0 + b1 = 2048 (dyadic scales 2, 1/2, 1/4, 4 below):
    # r = 2048 * c, r >> 4 = 128 * c; ((b0 * 128 * c) >> 16) + ((b1 * 128 * c) >> 16) lies in (4c - 2, 4c], and (that + 2) >> 2 = c
    const = np.full((16, 16, 3), 77, np.uint8)
    for size in ((8, 8), (32, 32), (64, 4)):
        assert (resize_linear_u8(const, size) == 77).all()
    # exact 2x down-scale: f = (float)((d + 0.5) * 2 - 0.5) = 2d + 0.5 -> s = 2d, f = 0.5 -> coefficients (1024, 1024);
    # r0 = 1024 * (a + b), r0 >> 4 = 64 * (a + b), (1024 * 64 * (a + b)) >> 16 = a + b exactly, likewise c + d:
    # out = (a + b + c + d + 2) >> 2
    half = resize_linear_u8(img, (18, 12))
    blocks = img.astype(np.int32).reshape(12, 2, 18, 2, 3)
    assert np.array_equal(half, ((blocks.sum(axis=(1, 3)) + 2) >> 2).astype(np.uint8))
    # up-scale: the first column has f = 0.5 * (src / dst) - 0.5 < 0 -> s = -1 -> (0, 0): source column 0 alone; the last column has
    # f = (dst - 0.5) * src / dst - 0.5 = src - 1 + 0.5 * (1 - src / dst) >= src - 1 -> (src - 1, 0): source column src - 1 alone.
    # With the row count unchanged (coefficients (2048, 0) vertically) those two columns are the source's own
    wide = resize_linear_u8(img, (90, 24))
    assert np.array_equal(wide[:, 0], img[:, 0]) and np.array_equal(wide[:, -1], img[:, -1])
    with pytest.raises(ValueError):
        resize_linear_u8(img.astype(np.float32), (4, 4))


def test_pad_shape_mask_and_normalised_pad_value():
    from oracle.loader import normalize_chw
    t = mp.BottomUpPad(is_train=False, config=CFG)
    land = t.transform(dict(image=np.full((333, 832, 3), 9, np.uint8)))
    assert land["image"].shape == (512, 832, 3) and land["mask"].shape == (512, 832) and land["mask"].dtype == np.uint8
    assert land["mask"][:333].all() and not land["mask"][333:].any() and not land["image"][333:].any()
    port = t.transform(dict(image=np.full((683, 512, 3), 9, np.uint8)))  # portrait: padded to (512, 832) as (w, h)
    assert port["image"].shape == (832, 512, 3) and port["mask"][:683].all() and not port["mask"][683:].any()
    with pytest.raises(AssertionError):
        t.transform(dict(image=np.zeros((600, 832, 3), np.uint8)))
    # the pad is on the uint8 image, before Normalize: a padded pixel is (0 - mean * 255) / (std * 255), not 0
    mean, std = [m * 255.0 for m in MEAN], [s * 255.0 for s in STD]
    chw = normalize_chw(land["image"], mean, std)
    for c in range(3):
        want = (np.float32(0) - np.float32(mean[c])) / np.float32(std[c])
        assert (chw[c, 333:] == want).all() and want != 0


def _kp(x0, y0, size=120.0, seed=0):
    rng = np.random.RandomState(seed)
    kp = np.zeros((17, 3))
    kp[:, 0], kp[:, 1], kp[:, 2] = x0 + rng.uniform(0, 1, 17) * size, y0 + rng.uniform(0, 1, 17) * size, 2
    return kp


def _write_coco(tmp_path):
    """Three images in file order 7, 3, 9; image 9 has no annotation."""
    images = [dict(id=7, file_name="b.jpg", width=640, height=480), dict(id=3, file_name="a.jpg", width=480, height=640),
              dict(id=9, file_name="c.jpg", width=500, height=375)]
    anns = []
    for ann_id, (image_id, x0, y0) in enumerate(((7, 50, 60), (7, 300, 200), (3, 100, 300)), start=1):
        kp = _kp(x0, y0, seed=ann_id)
        anns.append(dict(id=ann_id, image_id=image_id, category_id=1, iscrowd=0, num_keypoints=17, keypoints=kp.reshape(-1).tolist(),
                         area=120.0 * 120.0, bbox=[x0, y0, 120.0, 120.0]))
    path = os.path.join(tmp_path, "ann.json")
    with open(path, "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=1, name="person")]), f)
    return path, anns


def test_coco_bottomup_dataset(tmp_path):
    ann, _ = _write_coco(tmp_path)
    for name in ("a.jpg", "b.jpg", "c.jpg"):
        with open(os.path.join(tmp_path, name), "wb") as f:
            f.write(b"\xff\xd8payload-" + name.encode())
    ds = mp.COCOBottomUpDataset(str(tmp_path), ann, is_train=False)
    assert len(ds) == 3  # the image without annotations is a record too
    assert ds.name2id == {"b.jpg": 7, "a.jpg": 3, "c.jpg": 9} and ds.id2name[9] == "c.jpg"
    image, mask, center, scale, image_file, image_shape = ds[2]
    assert image.dtype == np.uint8 and image.tobytes() == b"\xff\xd8payload-c.jpg" and image_file.endswith("c.jpg")
    assert (mask.dtype, center.dtype, scale.dtype, image_shape.dtype) == (np.uint8, np.float32, np.float32, np.int32)
    assert [os.path.basename(ds[i][4]) for i in range(3)] == ["b.jpg", "a.jpg", "c.jpg"]  # file order
    ds.lazy_image = True  # the codec workers read the file themselves: only the path travels
    assert isinstance(ds[0][0], str) and ds[0][0].endswith("b.jpg")
    with pytest.raises(ValueError, match="bottom-up training data is not implemented"):
        mp.COCOBottomUpDataset(str(tmp_path), ann, is_train=True)
    sharded = mp.create_dataset(str(tmp_path), ann, dataset_format="coco_bottomup", is_train=False)
    assert len(sharded) == 3 and sharded.column_names == ["image", "mask", "center", "scale", "image_file", "image_shape"]
    assert sharded.indices().tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        mp.create_dataset(str(tmp_path), ann, dataset_format="coco_bottomup", is_train=True)
    with pytest.raises(ValueError, match="bottom-up training data is not implemented"):
        mp.create_pipeline(sharded, ["bottomup_rescale", "bottomup_pad"], method="bottomup", is_train=True, config=CFG)
    folder = mp.ImageFolderBottomUpDataset(str(tmp_path))
    assert sorted(os.path.basename(folder[i][4]) for i in range(len(folder))) == ["a.jpg", "b.jpg", "c.jpg"]  # ann.json is no image


EVAL_CFG = dict(oks_thr=0.9, use_nms=False, soft_nms=False, sigmas=(np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62,
                                                                              0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89]) / 10.0).tolist())


def _records(anns, names, drop_images=()):
    """Inference records that repeat the ground truth: pred [P, K, 3 + L] (one tag column), score [P]."""
    by_image = {}
    for a in anns:
        by_image.setdefault(a["image_id"], []).append(np.concatenate([np.array(a["keypoints"]).reshape(17, 3), np.zeros((17, 1))], axis=1))
    records = []
    for image_id, people in by_image.items():
        if image_id in drop_images:
            people = []
        records.append(dict(pred=np.array(people).reshape(-1, 17, 4), score=[0.9 - 0.1 * i for i in range(len(people))],
                            image_path=os.path.join("/somewhere", names[image_id])))
    return records


def test_bottomup_evaluator_on_hand_built_records(tmp_path):
    ann, anns = _write_coco(tmp_path)
    names = {7: "b.jpg", 3: "a.jpg", 9: "c.jpg"}
    result = os.path.join(tmp_path, "res.json")
    ev = mp.create_evaluator(ann, name="bottomup", metric="AP", config=EVAL_CFG, result_path=result)
    assert isinstance(ev, mp.BottomUpEvaluator)
    stats = ev(_records(anns, names))
    assert stats["AP"] == 1.0 and stats["AR"] == 1.0 and not os.path.exists(result)  # the predictions are the ground truth
    # every person of image 3 dropped: 2 of the 3 ground-truth persons are still matched at every OKS threshold -> AR = 2 / 3;
    # precision stays 1 up to that recall: AP = the share of the 101 recall points <= 2 / 3 = 67 / 101
    stats = ev(_records(anns, names, drop_images=(3,)))
    assert abs(stats["AR"] - 2 / 3) < 1e-12 and abs(stats["AP"] - 67 / 101) < 1e-12
    # an exact duplicate of a person: OKS 1 > oks_thr, removed by the NMS; kept without it
    dup = _records(anns, names)
    dup[0]["pred"] = np.concatenate([dup[0]["pred"], dup[0]["pred"][:1]])
    dup[0]["score"] = dup[0]["score"] + [0.3]
    for use_nms, want in ((False, 4), (True, 3)):
        e = mp.BottomUpEvaluator(ann, config=dict(EVAL_CFG, use_nms=use_nms), remove_result_file=False, result_path=result)
        e.eval(dup)
        with open(result) as f:
            entries = json.load(f)
        assert len(entries) == want and {x["image_id"] for x in entries} == {7, 3}
        # the area of a person is the extent of its key points (bottomup_evaluator.py:81-83); center / scale are not known: -1
        assert entries[0]["center"] == -1 and entries[0]["scale"] == -1 and len(entries[0]["keypoints"]) == 51
        os.remove(result)

    class Wider(mp.BottomUpEvaluator):
        SUPPORT_METRICS = {"AP", "PCK"}

    with pytest.raises(ValueError, match="PCK"):
        Wider(ann, metric="PCK", config=EVAL_CFG, result_path=result).eval(_records(anns, names))
    with pytest.raises(KeyError):
        mp.BottomUpEvaluator(ann, metric="PCK", config=EVAL_CFG)
    with pytest.raises(KeyError):
        mp.BottomUpEvaluator(ann, config=dict(oks_thr=0.9))  # the evaluation keys are required
