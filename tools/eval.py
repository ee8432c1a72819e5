#!/usr/bin/env python3
"""python tools/eval.py --config RECIPE.yaml --ckpt MODEL.ckpt [--outdir DIR] [--cfg-options K=V ...]  (mindpose_amd.cli.eval)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mindpose_amd.cli.eval import main  # noqa: E402

if __name__ == "__main__":
    main()
