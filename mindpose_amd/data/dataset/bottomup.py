"""Bottom-up record store, evaluation side (reference: mindpose/data/dataset/bottomup.py:7-102).

Contract kept: the constructor, the two hooks of a format class (``load_dataset_cfg`` / ``load_dataset``) and the evaluation tuple
``(image, mask, center, scale, image_file, image_shape)`` with its typed placeholders.  The training tuple (key points, boxes, the
crowd mask) is not built: ``is_train=True`` raises ``ValueError``.  The ``image`` column follows the lazy-path convention of
``dataset/topdown.py``: a pipeline whose codec runs in worker processes sets ``lazy_image`` and only the path travels."""
import logging
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

from ..column_names import COLUMN_MAP
from .topdown import ImagePath

_PLACEHOLDERS = dict(mask=np.uint8(0), center=np.float32(0), scale=np.float32(0), image_shape=np.int32(0))  # bottomup.py:95-102


class BottomUpDataset:
    """Args (bottomup.py:34-49): image_root, annotation_file, is_train, num_joints, config.

    Items (evaluation): (image, mask, center, scale, image_file, image_shape) - ``image`` the encoded file, ``mask`` / ``center`` /
    ``scale`` / ``image_shape`` placeholders the transforms fill.  A format class implements ``load_dataset_cfg() -> dict`` and
    ``load_dataset() -> list of records`` with the key ``image_file``."""

    def __init__(self, image_root: str, annotation_file: Optional[str] = None, is_train: bool = False, num_joints: int = 17,
                 config: Optional[Dict[str, Any]] = None) -> None:
        if is_train:
            raise ValueError("bottom-up training data is not implemented")
        self.image_root = image_root
        self.annotation_file = annotation_file
        self.is_train = is_train
        self.num_joints = num_joints
        self.config = config if config else dict()
        self._dataset_cfg = self.load_dataset_cfg()
        self._dataset = self.load_dataset()
        self._columns = COLUMN_MAP["bottomup"]["val"]
        logging.info(f"Number of records in dataset: {len(self._dataset)}")

    def load_dataset_cfg(self) -> Dict[str, Any]:
        raise NotImplementedError("Child class must implement this method.")

    def load_dataset(self) -> List[Dict[str, Any]]:
        raise NotImplementedError("Child class must implement this method.")

    def __len__(self) -> int:
        return len(self._dataset)

    def image_size(self, idx: int) -> Tuple[int, int]:
        """(width, height) of record ``idx`` WITHOUT decoding its pixels: what a pipeline that buckets its batches by network input
        shape (``create_pipeline(bucket_by_shape=True)``) asks before any image exists.  A format class answers from what it
        holds - the annotation file, the file's header."""
        raise NotImplementedError("Child class must implement this method.")

    def _column_sources(self, idx: int) -> Dict[str, Callable[[], Any]]:
        image_file = self._dataset[idx]["image_file"]
        lazy = getattr(self, "lazy_image", False)
        return {"image": (lambda: ImagePath(image_file)) if lazy else (lambda: np.fromfile(image_file, dtype=np.uint8)),
                "image_file": lambda: image_file}

    def __getitem__(self, idx: int) -> tuple:
        produce = self._column_sources(idx)
        return tuple(produce[name]() if name in produce else _PLACEHOLDERS[name] for name in self._columns)
