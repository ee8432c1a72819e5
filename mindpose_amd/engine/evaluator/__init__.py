from .bottomup_evaluator import BottomUpEvaluator  # noqa: F401
from .coco_eval import coco_keypoint_eval  # noqa: F401
from .evaluator import Evaluator  # noqa: F401
from .topdown_evaluator import TopDownEvaluator  # noqa: F401

__all__ = ["Evaluator", "TopDownEvaluator", "BottomUpEvaluator", "coco_keypoint_eval"]
