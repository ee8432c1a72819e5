"""Command line and recipe files of the runner: ``--config recipe.yaml [--outdir DIR] [--ckpt FILE] [--cfg-options K=V ...]``.

A recipe is a YAML mapping (the files under ``configs/`` of a mindpose checkout); every top-level key becomes an attribute of the
returned namespace.  ``--cfg-options`` overrides single settings after the file is read: ``K=V`` or ``K:V``, ``K`` a dotted path
into nested settings (``dataset_setting.det_bbox_thr=0.5``), ``V`` a Python literal where it parses as one and a string otherwise.
"""
import argparse
import ast
import logging
from typing import Any, Dict, List, Optional, Tuple

import yaml

__all__ = ["parse_args", "parse_option", "apply_option", "load_recipe"]

_logger = logging.getLogger(__name__)


def parse_option(pair: str) -> Tuple[str, Any]:
    """``"K=V"`` / ``"K:V"`` -> (K, value); the first ``=`` splits, else the first ``:``."""
    for sep in "=:":
        if sep in pair:
            key, text = pair.split(sep, 1)
            break
    else:
        raise ValueError(f"`{pair}`: --cfg-options takes `KEY=VALUE` or `KEY:VALUE` pairs")
    try:
        value = ast.literal_eval(text)
    except (ValueError, SyntaxError, TypeError, MemoryError, RecursionError):
        value = text  # not a literal: the text itself
    return key, value


def apply_option(args: argparse.Namespace, key: str, value: Any) -> None:
    """Set the setting at dotted path ``key``: the first part names an attribute of ``args``, the rest keys of nested dicts
    (created where the recipe has none)."""
    head, *rest = key.split(".")
    if not rest:
        setattr(args, head, value)
        return
    node = getattr(args, head, None)
    if not isinstance(node, dict):
        node = {}
        setattr(args, head, node)
    for part in rest[:-1]:
        if not isinstance(node.get(part), dict):
            node[part] = {}
        node = node[part]
    node[rest[-1]] = value


def load_recipe(path: str) -> Dict[str, Any]:
    with open(path, "r") as f:
        recipe = yaml.safe_load(f)
    if not isinstance(recipe, dict):
        raise ValueError(f"{path}: a recipe is a YAML mapping, got {type(recipe).__name__}")
    return recipe


class _Options(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, dict(parse_option(v) for v in values))


def parse_args(argv: Optional[List[str]] = None, description: str = "", need_ckpt: bool = False) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument("--config", required=True, help="recipe file (YAML)")
    parser.add_argument("--outdir", default="output", help="output directory")
    parser.add_argument("--ckpt", required=need_ckpt, help="checkpoint to load")
    parser.add_argument("--cfg-options", nargs="+", action=_Options, default={}, metavar="KEY=VALUE",
                        help="override settings of the recipe; dotted keys reach nested settings")
    args = parser.parse_args(argv)
    for key, value in load_recipe(args.config).items():
        setattr(args, key, value)
    for key, value in args.cfg_options.items():
        apply_option(args, key, value)
    _logger.info(args)
    return args
