"""Generate tests/golden/bottomup_records.npz: what the REFERENCE's own ``COCOBottomUpDataset`` (mindpose/data/dataset/coco_bottomup.py)
returns as ``keypoints`` and ``boxes`` for the annotation file of tests/bottomup_mask_cases.py.

Run ONLY where a checkout of the reference is present:  python tests/golden/gen_bottomup_records_golden.py <reference root>

The class is loaded by file path, as gen_bottomup_augment_golden.py loads the transforms: ``mindpose/__init__.py`` (which imports
MindSpore) is bypassed, and empty stand-ins are registered for ``mindspore``, ``cv2`` and ``pycocotools`` - none is installed.
``pycocotools.coco.COCO`` is an in-script index of the json with the three calls the reference makes (``getAnnIds(imgIds=...)``,
``loadAnns``, ``loadImgs``), annotations in file order as pycocotools keeps them.  The reference's own
``_load_coco_keypoint_annotations_per_img`` runs per image - its annotation filter, ``_get_keypoints`` and ``_get_boxes`` - with
``_get_encoded_mask`` replaced by a stub: the mask needs pycocotools' rasteriser and cv2's erosion and CANNOT be pinned this way, so the
fixture holds none.  No reference source or bytecode is written anywhere: only the returned arrays.

Per image id ``i<id>/``: keypoints, boxes.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = os.path.join(sys.argv[1], "mindpose")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import bottomup_mask_cases as cases  # noqa: E402


class COCO:
    def __init__(self, annotation_file):
        with open(annotation_file) as f:
            data = json.load(f)
        self.imgs = {img["id"]: img for img in data["images"]}
        self.anns = {a["id"]: a for a in data["annotations"]}
        self._order = [a["id"] for a in data["annotations"]]

    def getImgIds(self):
        return list(self.imgs)

    def getAnnIds(self, imgIds):
        return [i for i in self._order if self.anns[i]["image_id"] == imgIds]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def loadImgs(self, idx):
        return [self.imgs[idx]]


def load_reference_class():
    for name in ["mindpose", "mindpose.data", "mindpose.data.dataset", "mindspore", "cv2", "pycocotools", "pycocotools.mask", "pycocotools.coco"]:
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["pycocotools.coco"].COCO = COCO
    sys.modules["pycocotools"].mask = sys.modules["pycocotools.mask"]

    def load(modname, path):
        spec = importlib.util.spec_from_file_location(modname, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    load("mindpose.register", REF + "/register.py")
    load("mindpose.data.dataset.bottomup", REF + "/data/dataset/bottomup.py")
    return load("mindpose.data.dataset.coco_bottomup", REF + "/data/dataset/coco_bottomup.py").COCOBottomUpDataset


def main():
    cls = load_reference_class()
    cls._get_encoded_mask = lambda self, annos, idx: None  # the mask is not pinned (see above)
    with tempfile.TemporaryDirectory() as tmp:
        dataset = cls(tmp, cases.write_records_json(tmp), is_train=False, num_joints=cases.K, config=cases.RECORD_CFG)
    out = dict(source="reference:mindpose/data/dataset/coco_bottomup.py COCOBottomUpDataset (numpy %s)" % np.__version__)
    for image in cases.IMAGES:
        rec = dataset._load_coco_keypoint_annotations_per_img(image["id"])
        out[f"i{image['id']}/keypoints"], out[f"i{image['id']}/boxes"] = rec["keypoints"], rec["boxes"]
        print(image["id"], rec["keypoints"].shape, rec["keypoints"].dtype, rec["boxes"].shape, rec["boxes"].dtype)
    path = os.path.join(HERE, "bottomup_records.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
