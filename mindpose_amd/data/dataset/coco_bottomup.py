"""COCO-format bottom-up records, without pycocotools (reference: mindpose/data/dataset/coco_bottomup.py:15-189).

Evaluation: one record per image id of the annotation file, in file order - images without annotations included, as the reference's
evaluation branch keeps them (:71-84).  ``load_dataset`` builds these and nothing else.

Training record PARTS, under the reference's method names and callable on a dataset built with ``is_train=False`` (the
``is_train=True`` switch itself stays a refusal): ``_load_coco_keypoint_annotations_per_img`` (:86-105), ``_get_keypoints`` (:120-132),
``_get_boxes`` (:134-144) and ``_get_encoded_mask`` (:146-189).  ``mask_info`` is NOT the reference's packed bits of the finished
mask - only the reference dataset's own ``__getitem__`` ever read those - but what the mask is made from,
``dict(regions=[uint32 run-length arrays], shape=(S, H, W), radii=[r_0 .. r_{S-1}])`` (``data/transform/bottomup_mask.py``):
``bottomup_masks_batch`` makes the masks of a batch on the device, ``decode_mask_info`` on the host.  The keys ``sigma`` /
``heatmap_sizes`` / ``expand_mask`` they read are taken from the config when present."""
import os
from typing import Any, Dict, List, Tuple

import numpy as np

from ...register import register
from ..transform.bottomup_mask import regions_of_annotation, stage_radii
from .bottomup import BottomUpDataset
from .coco_topdown import _CocoIndex


@register("dataset", extra_name="coco_bottomup")
class COCOBottomUpDataset(BottomUpDataset):
    def load_dataset_cfg(self) -> Dict[str, Any]:
        return {key: self.config[key] for key in ("sigma", "heatmap_sizes", "expand_mask") if key in self.config}

    def load_dataset(self) -> List[Dict[str, Any]]:
        self.coco = _CocoIndex(self.annotation_file)
        self.id2name, self.name2id = self._get_mapping_id_name(self.coco.imgs)
        self.img_ids = self.coco.get_img_ids()
        return [{"image_file": os.path.join(self.image_root, self.id2name[img_id])} for img_id in self.img_ids]

    def image_size(self, idx: int) -> Tuple[int, int]:
        """The annotation file's ``width`` / ``height`` of record ``idx`` (the pipeline checks the decoded image against them)."""
        info = self.coco.load_img(self.img_ids[idx])
        return int(info["width"]), int(info["height"])

    @staticmethod
    def _get_mapping_id_name(imgs: Dict[int, Dict[str, Any]]) -> Tuple[Dict[int, str], Dict[str, int]]:
        id2name = {image_id: image["file_name"] for image_id, image in imgs.items()}
        name2id = {image["file_name"]: image_id for image_id, image in imgs.items()}
        return id2name, name2id

    def _load_coco_keypoint_annotations_per_img(self, img_id: int) -> Dict[str, Any]:
        """One training record: ``image_file``, ``keypoints`` [S, M, K, 3], ``boxes`` [M, 2, 2], ``mask_info``.  The annotations stay
        in file order; ``mask_info`` is made from ALL of them, before the filter ``iscrowd == 0 or num_keypoints > 0``."""
        annos = list(self.coco.img_to_anns.get(img_id, []))
        mask_info = self._get_encoded_mask(annos, img_id)
        annos = [obj for obj in annos if obj["iscrowd"] == 0 or obj["num_keypoints"] > 0]
        return {"image_file": os.path.join(self.image_root, self.id2name[img_id]), "keypoints": self._get_keypoints(annos),
                "boxes": self._get_boxes(annos), "mask_info": mask_info}

    def _get_keypoints(self, annos: List[Dict[str, Any]]) -> np.ndarray:
        """[S, M, K, 3]: the image's stack tiled over the levels.  Without an annotation ``zeros((1, K, 3))`` - the untiled shape
        is the reference's own."""
        if len(annos) == 0:
            return np.zeros((1, self.num_joints, 3))
        keypoints = np.stack([np.array(x["keypoints"]).reshape((-1, 3)) for x in annos], axis=0)
        return np.tile(keypoints[None, ...], (len(self._dataset_cfg["heatmap_sizes"]), 1, 1, 1))

    def _get_boxes(self, annos: List[Dict[str, Any]]) -> np.ndarray:
        """[M, 2, 2]: (x0, y0), (x1, y1) from COCO's xywh.  Without an annotation ``zeros((1, 2, 2))``."""
        if len(annos) == 0:
            return np.zeros((1, 2, 2))
        boxes = np.stack([np.array(x["bbox"]) for x in annos], axis=0)
        boxes[..., 2] += boxes[..., 0]
        boxes[..., 3] += boxes[..., 1]
        return boxes.reshape((-1, 2, 2))

    def _get_encoded_mask(self, annos: List[Dict[str, Any]], idx: int) -> Dict[str, Any]:
        """What the training mask of image ``idx`` is made from: the regions of every crowd annotation and of every non-crowd
        annotation without key points, the [S, H, W] shape and the erosion radius per level (zero without ``expand_mask``)."""
        img_info = self.coco.load_img(idx)
        height, width = int(img_info["height"]), int(img_info["width"])
        regions: List[np.ndarray] = []
        for obj in annos:
            if "segmentation" in obj and (obj["iscrowd"] or obj["num_keypoints"] == 0):
                regions.extend(regions_of_annotation(obj, height, width))
        num_levels = len(self._dataset_cfg["heatmap_sizes"])
        radii = stage_radii(float(self._dataset_cfg["sigma"]), num_levels) if self._dataset_cfg["expand_mask"] else [0] * num_levels
        return {"regions": regions, "shape": (num_levels, height, width), "radii": radii}
