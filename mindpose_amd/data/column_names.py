"""Columns of the datasets and pipelines (reference: mindpose/data/column_names.py).  The bottom-up ``train`` lists are declared as
the reference has them, but only the ``val`` lists are used: bottom-up training data is not implemented."""

_TOPDOWN_TRAIN_COLUMN_NAMES = ["image", "center", "scale", "boxes", "keypoints", "rotation", "target", "target_weight"]
_TOPDOWN_TRAIN_FINAL_COLUMN_NAMES = ["image", "target", "target_weight"]
_TOPDOWN_VAL_COLUMN_NAMES = ["image", "center", "scale", "rotation", "image_file", "boxes", "bbox_ids", "bbox_scores"]
_TOPDOWN_VAL_FINAL_COLUMN_NAMES = ["image", "image_file", "boxes", "bbox_ids", "center", "scale", "bbox_scores"]

_BOTTOMUP_TRAIN_COLUMN_NAMES = ["image", "boxes", "keypoints", "target", "mask", "tag_ind"]
_BOTTOMUP_TRAIN_FINAL_COLUMN_NAMES = ["image", "target", "mask", "tag_ind"]
_BOTTOMUP_VAL_COLUMN_NAMES = ["image", "mask", "center", "scale", "image_file", "image_shape"]
_BOTTOMUP_VAL_FINAL_COLUMN_NAMES = ["image", "mask", "center", "scale", "image_file", "image_shape"]

COLUMN_MAP = dict(
    coco_topdown=dict(train=_TOPDOWN_TRAIN_COLUMN_NAMES, val=_TOPDOWN_VAL_COLUMN_NAMES),
    topdown=dict(train=_TOPDOWN_TRAIN_COLUMN_NAMES, val=_TOPDOWN_VAL_COLUMN_NAMES),
    coco_bottomup=dict(train=_BOTTOMUP_TRAIN_COLUMN_NAMES, val=_BOTTOMUP_VAL_COLUMN_NAMES),
    bottomup=dict(train=_BOTTOMUP_TRAIN_COLUMN_NAMES, val=_BOTTOMUP_VAL_COLUMN_NAMES),
    imagefolder_bottomup=dict(val=_BOTTOMUP_VAL_COLUMN_NAMES),
)
FINAL_COLUMN_MAP = dict(
    topdown=dict(train=_TOPDOWN_TRAIN_FINAL_COLUMN_NAMES, val=_TOPDOWN_VAL_FINAL_COLUMN_NAMES),
    bottomup=dict(train=_BOTTOMUP_TRAIN_FINAL_COLUMN_NAMES, val=_BOTTOMUP_VAL_FINAL_COLUMN_NAMES),
    imagefolder_bottomup=dict(val=_BOTTOMUP_VAL_FINAL_COLUMN_NAMES),
)
