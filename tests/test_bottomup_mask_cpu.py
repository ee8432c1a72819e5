"""The bottom-up training mask and record parts, host side.  pycocotools and cv2 are not installed: the polygon answers are the
determinate cases of the restated ``rleFrPoly``, the erosion is checked against ``scipy.ndimage.binary_erosion`` with the disc built
from ``disc_half_widths``, and ``_get_keypoints`` / ``_get_boxes`` against what the reference's own methods returned
(tests/golden/bottomup_records.npz)."""
import ctypes
import os

import numpy as np
import pytest
from scipy import ndimage

import mindpose_amd as mp
from mindpose_amd import _lib
from mindpose_amd.data.transform import bottomup_mask as bm
from tests import bottomup_mask_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bottomup_records.npz")


def test_polygon_known_answers():
    h, w = 8, 10
    counts = bm.rle_from_polygon([2, 1, 2, 5, 7, 5, 7, 1], h, w)
    assert counts.dtype == np.uint32 and counts.tolist() == [17, 4, 4, 4, 4, 4, 4, 4, 4, 4, 27]
    want = np.zeros((h, w), np.uint8)
    want[1:5, 2:7] = 1
    assert np.array_equal(bm.decode_region(counts, h, w), want)
    full = bm.rle_from_polygon([0, 0, 0, h, w, h, w, 0], h, w)
    assert full.tolist() == [0, 80] and bm.decode_region(full, h, w).all()
    triangle = bm.rle_from_polygon([1, 1, 6, 2, 3, 6], h, w)
    xs, ys = np.array([1, 6, 3.0]), np.array([1, 2, 6.0])
    assert abs(np.dot(xs, np.roll(ys, -1)) - np.dot(ys, np.roll(xs, -1))) / 2 == 11.5  # the shoelace area
    assert int(bm.decode_region(triangle, h, w).sum()) == 12
    with pytest.raises(ValueError):
        bm.rle_from_polygon([1, 2, 3], h, w)


@pytest.mark.parametrize("h, w", cases.SHAPES)
def test_region_decode_equals_a_plain_numpy_decode(h, w):
    for layout in cases.LAYOUTS:
        for counts in cases.regions(layout, h, w):
            assert int(counts.sum()) == h * w
            got = bm.decode_region(counts, h, w)
            assert got.dtype == np.uint8 and got.shape == (h, w)
            assert np.array_equal(got, cases.numpy_decode(counts, h, w)), layout
            assert np.array_equal(cases.encode(got), counts), layout  # and back
    with pytest.raises(ValueError):
        bm.decode_region(np.array([1, 2], np.uint32), h, w + 1)


def _disc(r):
    half = bm.disc_half_widths(r)
    return np.abs(np.arange(-r, r + 1))[None, :] <= half[:, None]


@pytest.mark.parametrize("r", [0, 1, 2, 3, 6, 12, 24, 48, 127])
def test_disc_properties(r):
    half = bm.disc_half_widths(r)
    assert half.shape == (2 * r + 1,) and np.array_equal(half, half[::-1]) and half[r] == r
    assert (np.diff(half[r:]) <= 0).all() and half.min() >= 0
    dy = np.arange(-r, r + 1)
    assert (np.abs(half - np.sqrt(r * r - dy * dy)) <= 1).all()
    disc = _disc(r)
    assert disc.shape == (2 * r + 1, 2 * r + 1) and disc[r, 0] and disc[r, -1] and disc[0, r] and disc[-1, r]


def test_stage_radii():
    assert bm.stage_radii(2.0, 2) == [24, 12]
    assert bm.stage_radii(2, 1) == [12] and bm.stage_radii(1.5, 3) == [36, 18, 9]


@pytest.mark.parametrize("h, w", cases.SHAPES)
def test_erosion_equals_scipy(h, w):
    radii = [24, 12, 6, 0]
    eroded_somewhere = False
    for layout in cases.LAYOUTS:
        info = cases.mask_info(layout, h, w, radii)
        got = bm.decode_mask_info(info)
        assert got.dtype == np.uint8 and got.shape == (4, h, w) and got.max() <= 1
        invalid = np.zeros((h, w), bool)
        for counts in info["regions"]:
            invalid |= cases.numpy_decode(counts, h, w).astype(bool)
        valid = ~invalid
        for i, r in enumerate(radii):
            want = ndimage.binary_erosion(valid, structure=_disc(r), border_value=1)
            assert np.array_equal(got[i].astype(bool), want), (layout, r, int((got[i].astype(bool) != want).sum()))
        assert np.array_equal(got[3].astype(bool), valid)  # radius 0 is the un-eroded plane
        eroded_somewhere |= bool((got[0] != got[3]).any())
        if layout == "none":
            assert got.all()
        if layout == "pixel_interior" and h > 1:  # one invalid pixel prints the disc itself, clipped by the image
            cy, cx = h // 2, w // 2
            disc = _disc(6)
            printed = np.ones((h + 12, w + 12), bool)
            printed[cy:cy + 13, cx:cx + 13] &= ~disc
            assert np.array_equal(got[2].astype(bool), printed[6:6 + h, 6:6 + w])
    assert eroded_somewhere


def _dataset(tmp_path, **cfg):
    return mp.COCOBottomUpDataset(str(tmp_path), cases.write_records_json(tmp_path), is_train=False, num_joints=cases.K,
                                  config=dict(cases.RECORD_CFG, **cfg))


def test_record_parts(tmp_path):
    ds = _dataset(tmp_path)
    assert len(ds) == 3 and ds.img_ids == [5, 2, 8] and ds._dataset[0] == {"image_file": os.path.join(str(tmp_path), "a.jpg")}  # as before
    anns = {a["id"]: a for a in cases.record_annotations()}
    rec = ds._load_coco_keypoint_annotations_per_img(5)
    assert sorted(rec) == ["boxes", "image_file", "keypoints", "mask_info"] and rec["image_file"].endswith("a.jpg")
    kept = [40, 30, 20, 50]  # file order; the crowd without key points (10) is filtered, the crowd with key points (50) stays
    assert rec["keypoints"].shape == (2, 4, cases.K, 3) and rec["keypoints"].dtype == np.int64
    for level in range(2):
        for m, ann_id in enumerate(kept):
            assert rec["keypoints"][level, m].reshape(-1).tolist() == anns[ann_id]["keypoints"]
    assert rec["boxes"].shape == (4, 2, 2) and rec["boxes"].dtype == np.float64
    for m, ann_id in enumerate(kept):
        x, y, bw, bh = anns[ann_id]["bbox"]
        assert rec["boxes"][m].tolist() == [[x, y], [x + bw, y + bh]]
    # mask_info: made from ALL annotations - the crowd's counts as they stand, two polygons, the crowd with key points; no person
    info = rec["mask_info"]
    assert sorted(info) == ["radii", "regions", "shape"] and info["shape"] == (2, 53, 70) and info["radii"] == [24, 12]
    assert len(info["regions"]) == 4 and all(r.dtype == np.uint32 and int(r.sum()) == 53 * 70 for r in info["regions"])
    assert info["regions"][0].tolist() == anns[10]["segmentation"]["counts"]
    for region, poly in zip(info["regions"][1:3], anns[30]["segmentation"]):
        assert np.array_equal(region, bm.rle_from_polygon(poly, 53, 70))
    assert info["regions"][3].tolist() == anns[50]["segmentation"]["counts"]
    mask = bm.decode_mask_info(info)
    assert mask.shape == (2, 53, 70) and 0 < mask[0].sum() < mask[1].sum() < 53 * 70
    assert mask[1, 5, 30] == 1  # inside person 40's polygon, far from every region: a person's segmentation is no part of the mask
    assert _dataset(tmp_path, expand_mask=False)._load_coco_keypoint_annotations_per_img(5)["mask_info"]["radii"] == [0, 0]
    # an image without annotations: the reference's untiled zeros, no region
    empty = ds._load_coco_keypoint_annotations_per_img(2)
    assert empty["keypoints"].shape == (1, cases.K, 3) and empty["keypoints"].dtype == np.float64 and not empty["keypoints"].any()
    assert empty["boxes"].shape == (1, 2, 2) and empty["boxes"].dtype == np.float64 and not empty["boxes"].any()
    assert empty["mask_info"] == dict(regions=[], shape=(2, 40, 37), radii=[24, 12])
    assert bm.decode_mask_info(empty["mask_info"]).all()
    # the two refusals name the annotation
    with pytest.raises(ValueError, match="annotation 60.*compressed"):
        ds._load_coco_keypoint_annotations_per_img(8)
    for seg in (dict(size=[53, 70], counts=[10, 20]), dict(size=[70, 53], counts=anns[10]["segmentation"]["counts"])):
        with pytest.raises(ValueError, match="annotation 10"):
            ds._get_encoded_mask([dict(anns[10], segmentation=seg)], 5)
    # the switches stay refusals
    with pytest.raises(ValueError, match="bottom-up training data is not implemented"):
        mp.COCOBottomUpDataset(str(tmp_path), cases.write_records_json(tmp_path), is_train=True, config=cases.RECORD_CFG)


def test_keypoints_and_boxes_equal_the_reference(tmp_path):
    golden = np.load(GOLDEN)
    ds = _dataset(tmp_path)
    anns = cases.record_annotations()
    for image in cases.IMAGES:
        of_image = [a for a in anns if a["image_id"] == image["id"]]
        kept = [a for a in of_image if a["iscrowd"] == 0 or a["num_keypoints"] > 0]
        for key, got in (("keypoints", ds._get_keypoints(kept)), ("boxes", ds._get_boxes(kept))):
            want = golden[f"i{image['id']}/{key}"]
            assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (image["id"], key)
    rec = ds._load_coco_keypoint_annotations_per_img(5)  # the filter and the order, through the record
    assert np.array_equal(rec["keypoints"], golden["i5/keypoints"]) and np.array_equal(rec["boxes"], golden["i5/boxes"])


def test_entry_point_validates_before_any_hip_call():
    lib = _lib.load()
    P = 4096  # a non-null address: validation must answer before anything dereferences or launches
    h, w = 6, 5

    def call(prefix=(3, 10, 30), region_ptr=(0, 3), tab=(h, w, 0, 1), offs=(0, 0), radii=(2, 1), n=1, s=2, out_bytes=2 * h * w,
             ws_bytes=h * w, null=None):
        arrays = dict(prefix=(ctypes.c_uint32 * len(prefix))(*prefix), region_ptr=(ctypes.c_int * len(region_ptr))(*region_ptr),
                      tab=(ctypes.c_int * len(tab))(*tab), offs=(ctypes.c_longlong * len(offs))(*offs),
                      radii=(ctypes.c_int * len(radii))(*radii), half=(ctypes.c_uint8 * (8 * 128))())
        dev = dict(dprefix=P, dregion=P, dtab=P, doffs=P, out=P, ws=P)
        for key in (null or ()):
            (arrays if key in arrays else dev)[key] = None
        return lib.mp_bottomup_train_masks(arrays["prefix"], arrays["region_ptr"], arrays["tab"], arrays["offs"], dev["dprefix"],
                                           dev["dregion"], dev["dtab"], dev["doffs"], arrays["radii"], arrays["half"], dev["out"], out_bytes,
                                           dev["ws"], ws_bytes, n, s, None)

    for key in ("prefix", "region_ptr", "tab", "offs", "radii", "half", "dprefix", "dregion", "dtab", "doffs", "out", "ws"):
        assert call(null=[key]) == -1, key
    for kw in (dict(s=0), dict(s=9), dict(radii=(128, 1)), dict(radii=(2, -1))):
        assert call(**kw) == _lib.MP_ERR_UNSUPPORTED, kw
    for kw in (dict(n=0), dict(n=65536), dict(tab=(0, w, 0, 1)), dict(tab=(h, -1, 0, 1)), dict(tab=(16385, w, 0, 1)),
               dict(prefix=(3, 10, 29)), dict(prefix=(3, 10, 31)), dict(prefix=(12, 10, 30)),  # wrong sums, a descending table
               dict(tab=(h, w, 1, 1)), dict(tab=(h, w, 0, -1)), dict(region_ptr=(0, 0)),
               dict(out_bytes=2 * h * w - 1), dict(offs=(1, 0)), dict(ws_bytes=h * w - 1), dict(offs=(0, 1)), dict(offs=(-4, 0))):
        assert call(**kw) == -2, kw
    assert {"mp_bottomup_train_masks", "mp_bottomup_train_augment_stages"} <= set(_lib.EXPORTED_SYMBOLS)


def test_batch_functions_refuse_the_host():
    import torch
    info = cases.mask_info("whole", 6, 5, [1])
    with pytest.raises(_lib.MindposeHipError):
        mp.bottomup_masks_batch([info], "cpu")
    with pytest.raises(_lib.MindposeHipError):
        bm.launch_bottomup_masks([info], torch.zeros(30, dtype=torch.uint8), [0])
    with pytest.raises(ValueError):
        mp.bottomup_masks_batch([], "cuda:0")
