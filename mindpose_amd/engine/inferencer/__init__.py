from .bottomup_inferencer import BottomUpHeatMapAEInferencer  # noqa: F401
from .topdown_inferencer import TopDownHeatMapInferencer  # noqa: F401

__all__ = ["BottomUpHeatMapAEInferencer", "TopDownHeatMapInferencer"]
