"""COCO-format bottom-up records for evaluation, without pycocotools (reference: mindpose/data/dataset/coco_bottomup.py:15-118).

One record per image id of the annotation file, in file order - images without annotations included, as the reference's
evaluation branch keeps them (:71-84).  The key points, boxes and the crowd mask of a record feed training only and are not
loaded; the keys ``sigma`` / ``heatmap_sizes`` / ``expand_mask`` the reference reads for that mask are taken when present."""
import os
from typing import Any, Dict, List, Tuple

from ...register import register
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

    @staticmethod
    def _get_mapping_id_name(imgs: Dict[int, Dict[str, Any]]) -> Tuple[Dict[int, str], Dict[str, int]]:
        id2name = {image_id: image["file_name"] for image_id, image in imgs.items()}
        name2id = {image["file_name"]: image_id for image_id, image in imgs.items()}
        return id2name, name2id
