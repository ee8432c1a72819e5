"""Every image of a folder as a bottom-up evaluation record, for demos (reference:
mindpose/data/dataset/imagefolder_bottomup.py:9-56)."""
import os
from typing import Any, Dict, List, Tuple

import numpy as np

from ...register import register
from .bottomup import BottomUpDataset


@register("dataset", extra_name="imagefolder_bottomup")
class ImageFolderBottomUpDataset(BottomUpDataset):
    SUPPORTED_EXTS = {".bmp", ".png", ".jpg", ".jpeg", ".tiff"}

    def load_dataset_cfg(self) -> Dict[str, Any]:
        return dict()

    def load_dataset(self) -> List[Dict[str, Any]]:
        self._sizes: Dict[int, Tuple[int, int]] = {}
        return [{"image_file": image_file} for image_file in self._search_images(self.image_root)]

    def _search_images(self, image_root: str) -> List[str]:
        files = [x for x in os.listdir(image_root) if os.path.splitext(x)[1].lower() in self.SUPPORTED_EXTS]
        return [os.path.join(image_root, x) for x in files]

    def image_size(self, idx: int) -> Tuple[int, int]:
        """From the file's header, read once per record: PIL's ``Image.open(path).size`` parses the header and decodes nothing; a
        ``.npy`` payload (which the codec accepts as well) answers from its own header."""
        if idx not in self._sizes:
            path = self._dataset[idx]["image_file"]
            with open(path, "rb") as f:
                magic = f.read(6)
            if magic == b"\x93NUMPY":
                height, width = np.load(path, mmap_mode="r", allow_pickle=False).shape[:2]
            else:
                from PIL import Image  # the image codec is host plumbing
                with Image.open(path) as im:
                    width, height = im.size
            self._sizes[idx] = (int(width), int(height))
        return self._sizes[idx]
