#!/usr/bin/env python3
"""python tools/train.py --config RECIPE.yaml [--outdir DIR] [--ckpt FILE] [--cfg-options K=V ...]  (mindpose_amd.cli.train)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mindpose_amd.cli.train import main  # noqa: E402

if __name__ == "__main__":
    main()
