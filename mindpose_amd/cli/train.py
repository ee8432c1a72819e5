"""Train a model from a recipe: ``python -m mindpose_amd.cli.train --config configs/hrnet/hrnet_w32_ascend.yaml`` (or
``python tools/train.py ...``; ``torchrun --nproc_per_node=8 tools/train.py ...`` for several ranks).

The recipe's keys are the ones of the YAML files of a mindpose checkout; ``mode`` and ``enable_graph_kernel`` (MindSpore context
settings) are ignored.  Top-down recipes only: ``pipeline_method: bottomup`` is refused by ``create_pipeline``.
"""
import logging
import math
import os
import random
from argparse import Namespace
from typing import Optional, Tuple

import numpy as np
import torch

from ..callbacks import EvalCallback
from ..data import create_dataset, create_pipeline
from ..engine import Trainer, create_evaluator, create_inferencer
from ..models.layers import Conv2d, Conv2dTranspose
from ..models import (NetWithLoss, PoseAccuracy, auto_mixed_precision, create_decoder, create_eval_network, create_loss,
                      create_network, create_network_with_loss)
from ..utils import DynamicLossScaleManager, create_lr_scheduler, create_optimizer, load_checkpoint, load_param_into_net
from ..utils.adamw import check_clip_norm
from .config import parse_args

_logger = logging.getLogger(__name__)


def resolve_ranks(distribute: bool, environ=None) -> Tuple[Optional[int], Optional[int], int]:
    """(device_num, rank_id, local_rank) of this process.  ``distribute`` with ``WORLD_SIZE`` set (a torchrun launch): the triple
    the launcher gave; otherwise one process: (None, None, 0)."""
    environ = os.environ if environ is None else environ
    if distribute and "WORLD_SIZE" in environ:
        return int(environ["WORLD_SIZE"]), int(environ.get("RANK", 0)), int(environ.get("LOCAL_RANK", 0))
    if distribute:
        _logger.info("`distribute` is set but WORLD_SIZE is not: running as one process")
    return None, None, 0


def init_distributed(distribute: bool) -> Tuple[Optional[int], Optional[int], torch.device]:
    """Open the process group when the launch has several ranks; returns device_num, rank_id (from the group) and this rank's
    device."""
    device_num, rank_id, local_rank = resolve_ranks(distribute)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    if device_num is not None:
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group("nccl")
        device_num, rank_id = dist.get_world_size(), dist.get_rank()
    return device_num, rank_id, dev


def val_pipeline(args: Namespace):
    """The validation dataset and pipeline of a recipe (also what evaluation runs on)."""
    dataset = create_dataset(args.val_root, args.val_label, dataset_format=args.dataset_format, is_train=False,
                             num_joints=args.num_joints, use_gt_bbox_for_val=args.val_use_gt_bbox,
                             detection_file=args.val_detection_result, num_workers=args.num_parallel_workers,
                             config=args.dataset_setting)
    return create_pipeline(dataset, transforms=args.val_transforms, method=args.pipeline_method, batch_size=args.batch_size,
                           is_train=False, normalize_mean=args.normalize_mean, normalize_std=args.normalize_std,
                           num_workers=args.num_parallel_workers, config=args.dataset_setting)


def init_weights(net: torch.nn.Module, skip: Optional[torch.nn.Module] = None) -> None:
    """What constructing the cells does in MindSpore: conv / deconv weights ~ HeUniform(sqrt(5)), i.e. U(-b, b) with
    b = 1 / sqrt(fan_in) (BatchNorm starts at gamma 1, beta 0 already).  The layers of this package are parameter HOLDERS - their
    conv weights are uninitialised memory until something is loaded - so a run that trains from scratch, and every head above a
    pretrained backbone, starts here.  Drawn from torch's global generator (``train`` seeds it); ``skip``: a sub-module whose
    weights were loaded."""
    skipped = {id(m) for m in skip.modules()} if skip is not None else set()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (Conv2d, Conv2dTranspose)) and id(m) not in skipped:
                torch.nn.init.kaiming_uniform_(m.weight, a=math.sqrt(5))
    if hasattr(net, "invalidate_plans"):
        net.invalidate_plans()


def network(args: Namespace, pretrained: bool, initialize: bool = False):
    net = create_network(args.backbone_name, args.head_name, neck_name=args.neck_name, backbone_pretrained=pretrained,
                         backbone_ckpt_url=args.backbone_ckpt_url, in_channels=args.in_channels,
                         neck_out_channels=args.neck_out_channels, num_joints=args.num_joints, backbone_args=args.backbone_setting,
                         neck_args=args.neck_setting, head_args=args.head_setting)
    if initialize:
        init_weights(net, skip=net.backbone if pretrained else None)
    return net


def evaluation(args: Namespace, net, dev, result_path: str, progress_bar: bool = False):
    """decoder -> eval network -> inferencer, and the evaluator that writes its key points to ``result_path``."""
    decoder = create_decoder(args.decoder_name, **(args.decoder_setting or {})).to(dev)
    eval_net = create_eval_network(net, decoder)
    inferencer = create_inferencer(net=eval_net, name=args.inference_method, config=args.eval_setting,
                                   dataset_config=args.dataset_setting, decoder=decoder, progress_bar=progress_bar)
    evaluator = create_evaluator(annotation_file=args.val_label, name=args.eval_method, metric=args.eval_metric,
                                 config=args.eval_setting, dataset_config=args.dataset_setting, result_path=result_path)
    return inferencer, evaluator


def train_metric(args: Namespace) -> Optional[PoseAccuracy]:
    """The training-time accuracy metric of a run: ``train_accuracy`` (``--cfg-options train_accuracy=True``; no recipe of the
    reference has the key) asks for the PCK of the output heat maps against the target heat maps, logged per epoch.  It compares
    one heat map per joint with its label, which is what the top-down pipeline trains on."""
    if not getattr(args, "train_accuracy", False):
        return None
    method = getattr(args, "pipeline_method", None)
    if method != "topdown":
        raise ValueError(f"`train_accuracy` needs `pipeline_method: topdown` (one target heat map per output heat map), the recipe "
                         f"has `{method}`")
    return PoseAccuracy()


def grad_clip_norm(args: Namespace) -> Optional[float]:
    """The optimizer's ``clip_norm`` of a run: ``clip_grad`` (bool, default False) switches clipping of the gradient by its global
    norm on, ``clip_value`` (default 15.0) is the norm - the two keys of the sibling mindcv recipes; no recipe of the reference has
    them, ``--cfg-options clip_grad=True clip_value=1.0`` sets them.  ``clip_value=inf`` measures and logs the norm and clips
    nothing.  A value that is not a positive number is refused, also with ``clip_grad`` off."""
    clip_grad = getattr(args, "clip_grad", False)
    if not isinstance(clip_grad, bool):
        raise ValueError(f"`clip_grad` is True or False, got {clip_grad!r}")
    value = getattr(args, "clip_value", 15.0)
    if isinstance(value, str) and value.strip().lower() in ("inf", "+inf", "infinity"):
        value = math.inf  # (not a Python literal: --cfg-options hands the text on)
    try:
        value = check_clip_norm(value)
    except ValueError as e:
        raise ValueError(f"`clip_value`: {e}") from None
    if value is None:
        raise ValueError("`clip_value` must be a positive number or inf, got None")
    return value if clip_grad else None


def train(args: Namespace) -> None:
    metric = train_metric(args)  # refused before anything is opened
    clip_norm = grad_clip_norm(args)  # likewise
    if getattr(args, "ema", False):  # (cli/eval takes the key; a run that silently kept no average would mislead)
        raise ValueError("`ema`: keeping an exponential moving average of the weights while training is not built yet")
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)
    device_num, rank_id, dev = init_distributed(bool(getattr(args, "distribute", False)))

    train_dataset = create_dataset(args.train_root, args.train_label, dataset_format=args.dataset_format, is_train=True,
                                   num_joints=args.num_joints, device_num=device_num, rank_id=rank_id,
                                   num_workers=args.num_parallel_workers, config=args.dataset_setting)
    train_pipeline = create_pipeline(train_dataset, transforms=args.train_transforms, method=args.pipeline_method,
                                     batch_size=args.batch_size, is_train=True, normalize_mean=args.normalize_mean,
                                     normalize_std=args.normalize_std, num_workers=args.num_parallel_workers,
                                     config=args.dataset_setting)
    val_dataset = val_pipeline(args) if args.val_while_train else None
    try:
        net = network(args, pretrained=args.backbone_pretrained, initialize=True).to(dev)
        _logger.info(f"Model param: {sum(p.numel() for p in net.parameters())}")
        if args.amp_level != "O0":
            auto_mixed_precision(net, args.amp_level)  # before the optimizer: the arenas are built over the network as it trains
        loss = create_loss(args.loss, **(args.loss_setting or {}))
        if metric is None:
            net_with_loss = create_network_with_loss(net, loss, has_extra_inputs=args.loss_with_extra_input).to(dev)
        else:  # (the factory keeps the reference's signature)
            net_with_loss = NetWithLoss(net, loss, has_extra_inputs=args.loss_with_extra_input, metric=metric).to(dev)
        lr_scheduler = create_lr_scheduler(name=args.scheduler, lr=args.lr, total_epochs=args.num_epochs,
                                           steps_per_epoch=train_pipeline.get_dataset_size(), warmup=args.warmup,
                                           **(args.lr_scheduler_setting or {}))
        optimizer = create_optimizer(net, name=args.optimizer, learning_rate=lr_scheduler, filter_bias_and_bn=args.filter_bias_and_bn,
                                     weight_decay=args.weight_decay, overlap=False, clip_norm=clip_norm,
                                     **(args.optimizer_setting or {}))
        if args.ckpt:
            _logger.info(f"Loading the checkpoint from {args.ckpt}")
            load_param_into_net(net, load_checkpoint(args.ckpt))  # (the arena's parameters are views: loaded in place)
        loss_scale_manager = DynamicLossScaleManager() if args.amp_level != "O0" else None

        inferencer, evaluator = None, None
        if args.val_while_train:
            os.makedirs(args.outdir, exist_ok=True)
            inferencer, evaluator = evaluation(args, net, dev, os.path.join(args.outdir, "result_keypoint.json"))

        model_outdir = os.path.join(args.outdir, "saved_model")
        os.makedirs(model_outdir, exist_ok=True)
        model_name = os.path.splitext(os.path.basename(args.config))[0]
        callback = EvalCallback(inferencer, evaluator, val_dataset, interval=args.val_interval, max_epoch=args.num_epochs,
                                save_best=args.save_best, save_last=args.save_last,
                                best_ckpt_path=os.path.join(model_outdir, f"{model_name}_best.ckpt"),
                                last_ckpt_path=os.path.join(model_outdir, f"{model_name}_last.ckpt"),
                                summary_dir=os.path.join(args.outdir, "summary"), rank_id=rank_id, device_num=device_num)
        try:
            with callback:
                Trainer(net_with_loss, optimizer, loss_scale_manager).train(args.num_epochs, train_pipeline, callbacks=[callback])
        finally:
            optimizer.close()
    finally:
        train_pipeline.close()
        if val_dataset is not None:
            val_dataset.close()


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s - %(message)s")
    train(parse_args(argv, description="Training script"))


if __name__ == "__main__":
    main()
