"""Bottom-up evaluator: per-person area, optional OKS NMS, COCO key-point AP (reference:
mindpose/engine/evaluator/bottomup_evaluator.py:12-122), host Python like the reference.  Consumes the records of
``BottomUpHeatMapAEInferencer``: ``{pred [P, K, 3 + L], score [P], image_path}`` per image."""
import os
from collections import defaultdict
from typing import Any, Dict, List

import numpy as np

from ...register import register
from ...utils.nms import oks_nms, soft_oks_nms
from .evaluator import Evaluator


@register("evaluator", extra_name="bottomup")
class BottomUpEvaluator(Evaluator):
    SUPPORT_METRICS = {"AP"}

    def load_evaluation_cfg(self) -> Dict[str, Any]:
        cfg = dict()
        cfg["oks_thr"] = self.config["oks_thr"]
        cfg["use_nms"] = self.config["use_nms"]
        cfg["soft_nms"] = self.config["soft_nms"]
        cfg["sigmas"] = np.array(self.config["sigmas"])
        return cfg

    def eval(self, inference_result: List[Dict[str, Any]]) -> Dict[str, Any]:
        """records -> per-image person lists (area = the extent of the key points, :81-83) -> (soft) OKS NMS per image -> result
        file -> the ten COCO statistics."""
        people: Dict[int, List[Dict[str, Any]]] = defaultdict(list)
        for record in inference_result:
            image_id = self.name2id[os.path.basename(record["image_path"])]
            for kpt, score in zip(record["pred"], record["score"]):
                area = (np.max(kpt[:, 0]) - np.min(kpt[:, 0])) * (np.max(kpt[:, 1]) - np.min(kpt[:, 1]))
                people[image_id].append({"keypoints": kpt[:, :3], "score": score, "image_id": image_id, "area": area})
        cfg = self._evaluation_cfg
        survivors = []
        for persons in people.values():
            if cfg["use_nms"]:
                keep = (soft_oks_nms if cfg["soft_nms"] else oks_nms)(persons, cfg["oks_thr"], sigmas=np.asarray(cfg["sigmas"]))
                persons = [persons[k] for k in keep]
            survivors.append(persons)
        return self._report(survivors)
