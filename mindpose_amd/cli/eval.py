"""Evaluate a checkpoint from a recipe: ``python -m mindpose_amd.cli.eval --config RECIPE.yaml --ckpt MODEL.ckpt`` (or
``python tools/eval.py ...``).  Serves top-down and bottom-up recipes; writes ``<outdir>/result.json`` and returns the result.

``--cfg-options ema=True`` evaluates the exponential moving average of the weights that a checkpoint holds under ``ema.<name>``
beside the live weights (the names ``weights.clone(prefix="ema")`` gives in MindSpore, what a mindcv-style run with ``ema: True``
saves) in place of the live ones; a file without such entries is refused.  BatchNorm moving statistics have no averaged twin: both
sets of weights share them."""
import json
import logging
import os
from argparse import Namespace
from typing import Any, Dict

import torch

from ..models import auto_mixed_precision
from ..utils import load_checkpoint, load_param_into_net
from .config import parse_args
from .train import evaluation, network, val_pipeline

_logger = logging.getLogger(__name__)


def use_ema(args: Namespace) -> bool:
    """The recipe key ``ema`` (bool, default False; the key of the sibling mindcv recipes, no recipe of the reference has it)."""
    ema = getattr(args, "ema", False)
    if not isinstance(ema, bool):
        raise ValueError(f"`ema` is True or False, got {ema!r}")
    return ema


def load_weights(net, ckpt: str, ema: bool):
    """The checkpoint into the network: with ``ema`` its ``ema.<name>`` entries in place of ``<name>`` - a file without them is
    refused - else the live weights (``ema.*`` are then names the network does not know, and ignored)."""
    return load_param_into_net(net, load_checkpoint(ckpt), strict_load=False, prefer_ema=ema)


def eval(args: Namespace) -> Dict[str, Any]:  # noqa: A001 - the reference's name
    ema = use_ema(args)  # refused before anything is opened
    dev = torch.device("cuda", torch.cuda.current_device())
    dataset = val_pipeline(args)
    try:
        net = network(args, pretrained=False).to(dev)
        missing = load_weights(net, args.ckpt, ema)
        if missing:
            _logger.warning(f"{len(missing)} parameter(s) of the network are not in {args.ckpt}: {missing[:5]} ...")
        if getattr(args, "amp_level", "O0") != "O0":
            auto_mixed_precision(net, args.amp_level)
        os.makedirs(args.outdir, exist_ok=True)
        inferencer, evaluator = evaluation(args, net, dev, os.path.join(args.outdir, "result_keypoint.json"), progress_bar=True)
        result = evaluator(inferencer(dataset))
    finally:
        dataset.close()
    result_path = os.path.join(args.outdir, "result.json")
    with open(result_path, "w") as f:
        json.dump(result, f, indent=4)
    _logger.info(result)
    _logger.info(f"Result is saved at `{result_path}`.")
    return result


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s - %(message)s")
    eval(parse_args(argv, description="Evaluation script", need_ckpt=True))


if __name__ == "__main__":
    main()
