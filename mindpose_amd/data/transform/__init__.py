from .bottomup_transform import (BottomUpGenerateTarget, BottomUpHorizontalRandomFlip, BottomUpPad, BottomUpRandomAffine,  # noqa: F401
                                 BottomUpRescale, BottomUpResize, BottomUpTransform, bottomup_augment_batch)
from .topdown_transform import (TopDownAffine, TopDownBoxToCenterScale, TopDownGenerateTarget,  # noqa: F401
                                TopDownHalfBodyTransform, TopDownHorizontalRandomFlip, TopDownRandomScaleRotation,
                                fliplr_joints, get_affine_transform, get_warp_matrix)

__all__ = ["TopDownGenerateTarget", "TopDownBoxToCenterScale", "TopDownAffine", "TopDownHorizontalRandomFlip",
           "TopDownHalfBodyTransform", "TopDownRandomScaleRotation", "fliplr_joints", "get_affine_transform", "get_warp_matrix",
           "BottomUpTransform", "BottomUpRescale", "BottomUpResize", "BottomUpPad", "BottomUpGenerateTarget",
           "BottomUpRandomAffine", "BottomUpHorizontalRandomFlip", "bottomup_augment_batch"]
