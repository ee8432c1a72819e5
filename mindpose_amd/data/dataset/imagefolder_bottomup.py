"""Every image of a folder as a bottom-up evaluation record, for demos (reference:
mindpose/data/dataset/imagefolder_bottomup.py:9-56)."""
import os
from typing import Any, Dict, List

from ...register import register
from .bottomup import BottomUpDataset


@register("dataset", extra_name="imagefolder_bottomup")
class ImageFolderBottomUpDataset(BottomUpDataset):
    SUPPORTED_EXTS = {".bmp", ".png", ".jpg", ".jpeg", ".tiff"}

    def load_dataset_cfg(self) -> Dict[str, Any]:
        return dict()

    def load_dataset(self) -> List[Dict[str, Any]]:
        return [{"image_file": image_file} for image_file in self._search_images(self.image_root)]

    def _search_images(self, image_root: str) -> List[str]:
        files = [x for x in os.listdir(image_root) if os.path.splitext(x)[1].lower() in self.SUPPORTED_EXTS]
        return [os.path.join(image_root, x) for x in files]
