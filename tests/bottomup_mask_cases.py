"""Shared inputs of tests/test_bottomup_mask_cpu.py, tests/test_gpu_bottomup_mask.py and tests/golden/gen_bottomup_records_golden.py:
the shapes and region layouts the training mask is checked on, and the annotation file of the record tests."""
import functools
import json
import os

import numpy as np

SHAPES = [(53, 70), (40, 37), (64, 128), (1, 9)]  # (h, w): odd extents, the 49-row disc taller than the image, dword rows, one row
LAYOUTS = ["none", "pixel_interior", "pixel_corner", "borders", "wrap", "starts_with_0", "whole", "overlap", "crowd300"]
K = 5  # joints of the record tests


def encode(mask):
    """The run-length counts of a binary [h, w] plane: column-major, zeros first."""
    flat = np.asarray(mask, dtype=np.uint8).T.reshape(-1)
    cuts = np.flatnonzero(np.diff(flat)) + 1
    counts = np.diff(np.concatenate([[0], cuts, [flat.size]]))
    if flat[0]:
        counts = np.concatenate([[0], counts])
    return counts.astype(np.uint32)


def numpy_decode(counts, h, w):
    """The ten-line decode the module's own is checked against: walk the runs, paint the odd ones."""
    flat = np.zeros(h * w, np.uint8)
    pos = 0
    for j, c in enumerate(counts):
        if j % 2:
            flat[pos:pos + int(c)] = 1
        pos += int(c)
    assert pos == h * w
    return flat.reshape(w, h).T


@functools.lru_cache(maxsize=None)
def regions(layout, h, w):
    """The regions (a tuple of uint32 count arrays) of one layout on an h x w image."""
    n = h * w
    plane = np.zeros((h, w), np.uint8)
    if layout == "none":
        return ()
    if layout == "pixel_interior":  # prints the disc itself
        plane[h // 2, w // 2] = 1
    elif layout == "pixel_corner":
        plane[h - 1, w - 1] = 1
    elif layout == "borders":  # one row and one column: touches all four borders
        plane[h // 3, :] = 1
        plane[:, (2 * w) // 3] = 1
    elif layout == "wrap":  # ONE run that wraps over several columns
        length = max(2, (5 * h) // 2)
        start = min(n - length - 1, h + max(0, h - 2))
        return (np.array([start, length, n - start - length], np.uint32),)
    elif layout == "starts_with_0":  # ones from the first pixel on
        return (np.array([0, min(n - 1, h + 3), n - min(n - 1, h + 3)], np.uint32),)
    elif layout == "whole":
        return (np.array([0, n], np.uint32),)
    elif layout == "overlap":
        other = np.zeros((h, w), np.uint8)
        plane[h // 4:h // 4 + max(1, h // 3), w // 4:w // 4 + max(1, w // 3)] = 1
        other[h // 3:h // 3 + max(1, h // 3), w // 3:w // 3 + max(1, w // 3)] = 1
        return (encode(plane), encode(other))
    elif layout == "crowd300":  # 300 random runs (as many as the image holds)
        rng = np.random.RandomState(h * 1000 + w)
        cuts = np.sort(rng.choice(np.arange(1, n), size=min(299, n - 1), replace=False))
        return (np.diff(np.concatenate([[0], cuts, [n]])).astype(np.uint32),)
    else:
        raise KeyError(layout)
    return (encode(plane),)


def mask_info(layout, h, w, radii):
    return dict(regions=list(regions(layout, h, w)), shape=(len(radii), h, w), radii=list(radii))


# ---- the record tests' annotation file: six annotations, NOT in id order; image 5 holds five of them
RECORD_CFG = dict(sigma=2.0, heatmap_sizes=[[16, 12], [32, 24]], expand_mask=True)
IMAGES = [dict(id=5, file_name="a.jpg", height=53, width=70), dict(id=2, file_name="b.jpg", height=40, width=37),
          dict(id=8, file_name="c.jpg", height=64, width=128)]


def _person(rng, w, h, visible):
    kp = np.concatenate([rng.randint(0, w, (K, 1)), rng.randint(0, h, (K, 1)), np.full((K, 1), 2)], axis=1)
    kp[visible:] = 0
    return [int(v) for v in kp.reshape(-1)]


def record_annotations():
    rng = np.random.RandomState(3)
    h, w = 53, 70
    crowd = np.zeros((h, w), np.uint8)
    crowd[30:45, 50:66] = 1
    crowd[33, 55] = 0
    return [
        dict(id=40, image_id=5, category_id=1, iscrowd=0, num_keypoints=4, bbox=[10.5, 8.0, 20.25, 30.0], keypoints=_person(rng, w, h, 4),
             segmentation=[[10, 8, 30, 8, 30, 38, 10, 38]]),  # an ordinary person: its segmentation is no part of the mask
        dict(id=10, image_id=5, category_id=1, iscrowd=1, num_keypoints=0, bbox=[50.0, 30.0, 16.0, 15.0], keypoints=[0] * (3 * K),
             segmentation=dict(size=[h, w], counts=[int(c) for c in encode(crowd)])),  # a crowd region with list counts
        dict(id=30, image_id=5, category_id=1, iscrowd=0, num_keypoints=0, bbox=[2.0, 40.0, 14.0, 11.0], keypoints=[0] * (3 * K),
             segmentation=[[2, 40, 9, 40, 9, 51, 2, 51], [11.5, 42.0, 16.0, 44.5, 12.0, 50.0]]),  # no key points: two polygons
        dict(id=20, image_id=5, category_id=1, iscrowd=0, num_keypoints=5, bbox=[35.0, 5.5, 18.0, 40.5], keypoints=_person(rng, w, h, 5),
             segmentation=[[35, 5, 53, 5, 53, 46, 35, 46]]),
        dict(id=50, image_id=5, category_id=1, iscrowd=1, num_keypoints=2, bbox=[0.0, 0.0, 12.0, 9.0], keypoints=_person(rng, w, h, 2),
             segmentation=dict(size=[h, w], counts=[int(c) for c in regions("starts_with_0", h, w)[0]])),  # a crowd WITH key points
        dict(id=60, image_id=8, category_id=1, iscrowd=1, num_keypoints=0, bbox=[1.0, 1.0, 5.0, 5.0], keypoints=[0] * (3 * K),
             segmentation=dict(size=[64, 128], counts="Xd02k1")),  # compressed string counts: refused
    ]


def write_records_json(directory):
    path = os.path.join(str(directory), "records.json")
    with open(path, "w") as f:
        json.dump(dict(images=IMAGES, annotations=record_annotations(), categories=[dict(id=1, name="person")]), f)
    return path
