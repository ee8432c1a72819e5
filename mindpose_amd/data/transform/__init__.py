from .bottomup_mask import (bottomup_masks_batch, decode_mask_info, disc_half_widths, rle_from_polygon,  # noqa: F401
                            stage_radii)
from .bottomup_transform import (BottomUpGenerateTarget, BottomUpHorizontalRandomFlip, BottomUpPad, BottomUpRandomAffine,  # noqa: F401
                                 BottomUpRescale, BottomUpResize, BottomUpTransform, bottomup_augment_batch)
from .topdown_transform import (TopDownAffine, TopDownBoxToCenterScale, TopDownGenerateTarget,  # noqa: F401
                                TopDownHalfBodyTransform, TopDownHorizontalRandomFlip, TopDownRandomScaleRotation,
                                fliplr_joints, get_affine_transform, get_warp_matrix)

__all__ = ["TopDownGenerateTarget", "TopDownBoxToCenterScale", "TopDownAffine", "TopDownHorizontalRandomFlip",
           "TopDownHalfBodyTransform", "TopDownRandomScaleRotation", "fliplr_joints", "get_affine_transform", "get_warp_matrix",
           "BottomUpTransform", "BottomUpRescale", "BottomUpResize", "BottomUpPad", "BottomUpGenerateTarget",
           "BottomUpRandomAffine", "BottomUpHorizontalRandomFlip", "bottomup_augment_batch",
           "bottomup_masks_batch", "decode_mask_info", "disc_half_widths", "rle_from_polygon", "stage_radii"]
