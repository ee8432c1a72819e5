"""Top-down evaluator: rescoring + OKS NMS + COCO key-point AP, host Python like the reference.

Mirror of ``TopDownEvaluator`` (mindpose/engine/evaluator/topdown_evaluator.py:12-148) and its base
(engine/evaluator/evaluator.py:15-180): same constructor, config keys, record format, result file, and the same ten
``(name, value)`` statistics - with the COCO annotation file read by ``json`` and the OKS-AP computed by
``coco_eval.coco_keypoint_eval`` instead of pycocotools.
"""
import os
from collections import defaultdict
from typing import Any, Dict, List

import numpy as np

from ...register import register
from ...utils.nms import oks_nms, soft_oks_nms
from .evaluator import Evaluator


@register("evaluator", extra_name="topdown")
class TopDownEvaluator(Evaluator):
    SUPPORT_METRICS = {"AP"}

    def load_evaluation_cfg(self) -> Dict[str, Any]:
        cfg = dict()
        cfg["vis_thr"] = self.config["vis_thr"]
        cfg["oks_thr"] = self.config["oks_thr"]
        cfg["use_nms"] = self.config["use_nms"]
        cfg["soft_nms"] = self.config["soft_nms"]
        cfg["sigmas"] = np.array(self.config["sigmas"])
        return cfg

    def eval(self, inference_result: List[Dict[str, Any]]) -> Dict[str, Any]:
        """records -> per-image person lists -> rescoring -> (soft) OKS NMS -> result file -> the ten COCO statistics."""
        people = self._group_by_image(inference_result)
        survivors = [self._suppress(self._rescore(persons)) for persons in people.values()]
        return self._report(survivors)

    def _group_by_image(self, records) -> Dict[int, List[Dict[str, Any]]]:
        """One list per image id, sorted by bbox_id with repeated boxes removed (:77-94, :134-148)."""
        people: Dict[int, List[Dict[str, Any]]] = defaultdict(list)
        for rec in records:
            image_id = self.name2id[os.path.basename(rec["image_path"])]
            box = rec["box"]
            people[image_id].append(dict(keypoints=rec["pred"], center=box[0:2], scale=box[2:4], area=box[4], score=box[5],
                                         image_id=image_id, bbox_id=rec["bbox_id"]))
        for image_id, persons in people.items():
            persons = sorted(persons, key=lambda person: person["bbox_id"])
            people[image_id] = [q for k, q in enumerate(persons) if k == 0 or q["bbox_id"] != persons[k - 1]["bbox_id"]]
        return people

    def _rescore(self, persons: List[Dict[str, Any]]) -> List[Dict[str, Any]]:
        """score = box score x mean confidence of the key points above ``vis_thr`` (:101-113); a python-float running sum in
        joint order, as the reference accumulates it."""
        vis_thr = self._evaluation_cfg["vis_thr"]
        for person in persons:
            total, count = 0, 0
            for joint in range(self.num_joints):
                conf = person["keypoints"][joint][2]
                if conf > vis_thr:
                    total, count = total + conf, count + 1
            person["score"] = (total / count if count else total) * person["score"]
        return persons

    def _suppress(self, persons: List[Dict[str, Any]]) -> List[Dict[str, Any]]:
        cfg = self._evaluation_cfg
        if not cfg["use_nms"]:
            return persons
        pick = (soft_oks_nms if cfg["soft_nms"] else oks_nms)(persons, cfg["oks_thr"], sigmas=np.asarray(cfg["sigmas"]))
        return [persons[k] for k in pick]
