"""What the COCO key-point evaluators share (reference: mindpose/engine/evaluator/evaluator.py:15-180): the constructor's
annotation index, the metric set, the result file and the call into the OKS-AP metric.  The annotation file is read with ``json``
and the metric is ``coco_eval.coco_keypoint_eval`` instead of pycocotools."""
import json
import os
from typing import Any, Dict, List, Optional, Set, Union

import numpy as np

from .coco_eval import STATS_NAMES, coco_keypoint_eval


class Evaluator:
    """A method's evaluator implements ``load_evaluation_cfg() -> dict`` and ``eval(records) -> {name: value}``; ``eval`` hands its
    per-image person lists to ``_report``."""

    SUPPORT_METRICS: Set[str] = set()

    def __init__(self, annotation_file: str, metric: Union[str, List[str]] = "AP", num_joints: int = 17,
                 config: Optional[Dict[str, Any]] = None, remove_result_file: bool = True,
                 result_path: str = "./result_keypoints.json") -> None:
        self.annotation_file = annotation_file
        self.num_joints = num_joints
        self.config = config if config else dict()
        self._metrics = set(metric) if isinstance(metric, list) else set([metric])
        for single_metric in self._metrics:
            if single_metric not in self.SUPPORT_METRICS:
                raise KeyError(f"metric {single_metric} is not supported")
        self._evaluation_cfg = self.load_evaluation_cfg()
        with open(annotation_file) as f:
            self.coco = json.load(f)
        self.id2name = {im["id"]: im["file_name"] for im in self.coco["images"]}
        self.name2id = {im["file_name"]: im["id"] for im in self.coco["images"]}
        cats = sorted(self.coco["categories"], key=lambda c: c["id"])
        self.classes = ["__background__"] + [c["name"] for c in cats]
        self._class_to_coco_ind = {c["name"]: c["id"] for c in cats}
        self.remove_result_file = remove_result_file
        self.result_path = result_path

    @property
    def metrics(self) -> Set[str]:
        return self._metrics

    def load_evaluation_cfg(self) -> Dict[str, Any]:
        raise NotImplementedError("Child class must implement this method.")

    def eval(self, inference_result: List[Dict[str, Any]]) -> Dict[str, Any]:
        raise NotImplementedError("Child class must implement this method.")

    def __call__(self, inference_result) -> Dict[str, Any]:
        return self.eval(inference_result)

    def _report(self, keypoints: List[List[Dict[str, Any]]]) -> Dict[str, Any]:
        """per-image person lists -> result file -> the ten COCO statistics; every requested metric must be among them."""
        results = self._dump_results(keypoints, self.result_path)
        stats = dict(self._do_python_keypoint_eval(results))
        missing = [m for m in self.metrics if m not in stats]
        if missing:
            raise ValueError(f"`{missing[0]}` is not in the returned result `{stats.keys()}`")
        if self.remove_result_file:
            os.remove(self.result_path)
        return stats

    def _dump_results(self, keypoints, res_file: str) -> List[Dict[str, Any]]:
        """COCO result entries of the (single) person category, written like evaluator.py:89-131 does."""
        cat_id = self._class_to_coco_ind[self.classes[1]]
        entries: List[Dict[str, Any]] = []
        for persons in keypoints:
            if not persons:
                continue
            flat = np.array([person["keypoints"] for person in persons]).reshape(-1, self.num_joints * 3)
            for person, row in zip(persons, flat):
                entries.append({"image_id": person["image_id"], "category_id": cat_id, "keypoints": row.tolist(),
                                "score": float(person["score"]), "center": np.asarray(person.get("center", -1)).tolist(),
                                "scale": np.asarray(person.get("scale", -1)).tolist()})
        with open(res_file, "w") as f:
            json.dump(entries, f, sort_keys=True, indent=4)
        return entries

    def _do_python_keypoint_eval(self, results):
        cat_id = self._class_to_coco_ind[self.classes[1]]
        gts = [a for a in self.coco["annotations"] if a.get("category_id", cat_id) == cat_id]
        stats = coco_keypoint_eval(gts, results, image_ids=sorted(self.id2name))
        return list(zip(STATS_NAMES, stats))
