"""The recipe runner's command line (mindpose_amd/cli/config.py) and rank resolution (cli/train.py), on the recipe files of the
reference kept unchanged under tests/golden/recipes/."""
import glob
import os

import pytest

from mindpose_amd.cli.config import parse_args, parse_option
from mindpose_amd.cli.train import resolve_ranks

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recipes")
W32 = os.path.join(RECIPES, "hrnet_w32_ascend.yaml")
ALL = sorted(glob.glob(os.path.join(RECIPES, "*.yaml")))


def test_the_eleven_fixture_files_are_there():
    names = [os.path.basename(p) for p in ALL]
    assert len(names) == 11 and "higher_hrnet_w32_ascend.yaml" in names and "hrnet_w32_ascend.yaml" in names, names


@pytest.mark.parametrize("path", ALL, ids=[os.path.basename(p) for p in ALL])
def test_every_recipe_parses(path):
    args = parse_args(["--config", path])
    assert args.config == path and args.outdir == "output" and args.ckpt is None and args.cfg_options == {}
    for key in ("dataset_format", "pipeline_method", "batch_size", "backbone_name", "head_name", "decoder_name", "loss", "amp_level",
                "scheduler", "num_epochs", "lr", "optimizer", "inference_method", "eval_method", "val_transforms", "train_transforms"):
        assert hasattr(args, key), key
    assert isinstance(args.dataset_setting, dict) and isinstance(args.eval_setting, dict)


def test_hrnet_w32_values():
    args = parse_args(["--config", W32])
    assert args.batch_size == 128
    assert args.lr_scheduler_setting == {"milestones": [170, 200]}
    assert args.normalize_std[2] == 0.255


def test_options_land_at_their_dotted_paths():
    args = parse_args(["--config", W32, "--outdir", "o", "--cfg-options", "batch_size=4", "dataset_setting.det_bbox_thr=0.5",
                       "eval_setting.hflip_tta:True", "val_root=/x"])
    assert args.batch_size == 4 and isinstance(args.batch_size, int)
    assert args.dataset_setting["det_bbox_thr"] == 0.5
    assert args.dataset_setting["image_size"] == [192, 256]  # the siblings stay
    assert args.eval_setting["hflip_tta"] is True
    assert args.val_root == "/x" and args.outdir == "o"


def test_option_values():
    assert parse_option("lr_scheduler_setting.milestones=[2]") == ("lr_scheduler_setting.milestones", [2])
    assert parse_option("backbone_pretrained=False") == ("backbone_pretrained", False)
    assert parse_option("a=b=c") == ("a", "b=c")
    assert parse_option("url=https://host/x.ckpt") == ("url", "https://host/x.ckpt")  # `=` splits before `:`
    # not a literal: stays a string
    args = parse_args(["--config", W32, "--cfg-options", "optimizer=sgd", "dataset_setting.new.deep=some text"])
    assert args.optimizer == "sgd" and args.dataset_setting["new"] == {"deep": "some text"}


def test_pair_without_separator_is_a_value_error():
    with pytest.raises(ValueError):
        parse_args(["--config", W32, "--cfg-options", "batch_size"])


def test_need_ckpt_exits_without_one():
    with pytest.raises(SystemExit):
        parse_args(["--config", W32], need_ckpt=True)
    assert parse_args(["--config", W32, "--ckpt", "m.ckpt"], need_ckpt=True).ckpt == "m.ckpt"


def test_rank_resolution_opens_no_group():
    import torch.distributed as dist
    assert resolve_ranks(True, environ={})[:2] == (None, None)
    assert resolve_ranks(False, environ={"WORLD_SIZE": "2", "RANK": "1", "LOCAL_RANK": "1"})[:2] == (None, None)
    assert resolve_ranks(True, environ={"WORLD_SIZE": "2", "RANK": "1", "LOCAL_RANK": "1"}) == (2, 1, 1)
    assert not (dist.is_available() and dist.is_initialized())
