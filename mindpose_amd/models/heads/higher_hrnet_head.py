"""HigherHRNet head (reference: mindpose/models/heads/higher_hrnet_head.py:72-229).

``final_layers[0]`` (1x1 conv with bias) makes the low-resolution heat maps + tags; each deconvolution layer then takes the
channel concatenation of its input and that output, runs Conv2dTranspose(4, 2, 1) + BN + ReLU and ``num_basic_blocks``
BasicBlocks, and ``final_layers[i + 1]`` makes the next, doubled, resolution.  The network output is the list of those maps,
lowest resolution first.

Under amp O2 the whole head runs on the fp16 kernels in the channel-blocked layout; a layer wider than a kernel stages (the
256 - 416 columns after the deconvolution at the bottom-up eval sizes) is recorded by the plan as output-column bands.
"""
from typing import List

import torch.nn as nn

from ...register import register
from ..backbones.hrnet import BasicBlock
from ..act_c8 import ActC8
from ..layers import BatchNorm2d, Conv2d, Conv2dTranspose, Plan
from .head import Head


@register("head", extra_name="higher_hrnet_head")
class HigherHRNetHead(Head):
    """Parameter names follow the reference's cells so that a mindpose checkpoint maps name for name:
    ``final_layers.{i}.weight / bias``, ``deconv_layers.{i}.0.0.weight`` ([Cin, Cout, 4, 4]), ``deconv_layers.{i}.0.1.*`` (its
    BatchNorm) and ``deconv_layers.{i}.{1..num_basic_blocks}.conv1 / bn1 / conv2 / bn2.*``."""

    def __init__(self, in_channels: int = 32, num_joints: int = 17, with_ae_loss: List[bool] = [True, False],
                 tag_per_joint: bool = True, final_conv_kernel_size: int = 1, num_deconv_layers: int = 1,
                 num_deconv_filters: List[int] = [32], num_deconv_kernels: List[int] = [4], cat_outputs: List[bool] = [True],
                 num_basic_blocks: int = 4) -> None:
        super().__init__()
        self.in_channels, self.num_joints = in_channels, num_joints
        self.with_ae_loss, self.tag_per_joint = list(with_ae_loss), tag_per_joint
        self.final_conv_kernel_size, self.num_deconv_layers = final_conv_kernel_size, num_deconv_layers
        self.num_deconv_filters, self.num_deconv_kernels = list(num_deconv_filters), list(num_deconv_kernels)
        self.cat_outputs, self.num_basic_blocks = list(cat_outputs), num_basic_blocks
        for kernel in self.num_deconv_kernels[:num_deconv_layers]:
            if kernel == 2:
                raise NotImplementedError("num_deconv_kernels = 2 (Conv2dTranspose(2, 2, 0)) is not implemented on the HIP path")
            if kernel != 4:
                raise ValueError("Invalid deconv_kernel.")
        if final_conv_kernel_size not in (1, 3):
            raise ValueError("final_conv_kernel_size must be 1 or 3")

        widths = [self._out_width(i) for i in range(num_deconv_layers + 1)]
        k, pad = final_conv_kernel_size, 1 if final_conv_kernel_size == 3 else 0
        finals, deconvs, width = [Conv2d(in_channels, widths[0], k, padding=pad, has_bias=True)], [], in_channels
        for i in range(num_deconv_layers):
            if self.cat_outputs[i]:
                width += widths[i]
            planes = self.num_deconv_filters[i]
            cells = [nn.Sequential(Conv2dTranspose(width, planes, 4), BatchNorm2d(planes), nn.ReLU())]
            cells += [BasicBlock(planes, planes) for _ in range(num_basic_blocks)]
            deconvs.append(nn.Sequential(*cells))
            finals.append(Conv2d(planes, widths[i + 1], k, padding=pad, has_bias=True))
            width = planes
        self.deconv_layers = nn.ModuleList(deconvs)
        self.final_layers = nn.ModuleList(finals)

    def _out_width(self, i: int) -> int:
        """channels of output i: heat maps, plus tags when that resolution has the associative-embedding output"""
        return self.num_joints + ((self.num_joints if self.tag_per_joint else 1) if self.with_ae_loss[i] else 0)

    @staticmethod
    def _fp32(plan: Plan, x):
        return plan.from_c8(x) if isinstance(x, ActC8) else x

    def emit(self, plan: Plan, x) -> List:
        y = plan.conv(x, self.final_layers[0])
        outputs = [y]
        for i in range(self.num_deconv_layers):
            if self.cat_outputs[i]:
                if isinstance(x, ActC8) != isinstance(y, ActC8) or (isinstance(x, ActC8) and x.shape[1] % 8):
                    x, y = self._fp32(plan, x), self._fp32(plan, y)
                x = plan.concat(x, y)
            seq = list(self.deconv_layers[i])
            x = plan.deconv4x4s2(x, seq[0][0], seq[0][1], relu=True)
            for blk in seq[1:]:
                x = blk.emit(plan, x)
            y = plan.conv(x, self.final_layers[i + 1])
            outputs.append(y)
        return outputs
