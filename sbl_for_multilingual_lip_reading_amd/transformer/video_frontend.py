# coding: utf-8
"""The visual frontend with the class surface and state-dict keys of the reference's transformer/video_frontend.py:
Conv3d stem + ResNet-18 trunk.

The torch.nn conv / batch-norm modules below are parameter containers only (so state-dict keys, shapes, .to(),
pickling and the seeded initialisation behave like the reference's); their own forward is never called.
Activations flow channels-last: (N*T, h, w, C)."""
import math

import torch
import torch.nn as nn

from ._env import config, ops


def conv3x3(in_planes, out_planes, stride=1):
    """Bias-free 3x3 convolution, padding 1."""
    return nn.Conv2d(in_planes, out_planes, 3, stride, 1, bias=False)


def _he_init(modules):
    """Conv kernels ~ N(0, 2 / (out_channels * kernel volume)) with zero biases, BatchNorm affines (1, 0); applied in
    the iteration order of `modules`, which fixes the RNG draws."""
    for m in modules:
        if isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Conv3d)):
            nn.init.normal_(m.weight, 0.0, math.sqrt(2.0 / (m.out_channels * math.prod(m.kernel_size))))
            if isinstance(m.bias, torch.Tensor):
                nn.init.zeros_(m.bias)
        elif isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)


def _params(conv, bn):
    """The parameters, BatchNorm buffers and settings of a conv -> BatchNorm2d pair, as the block's tape node takes them."""
    return ops.ConvBN(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                      conv.stride[0], bn.momentum, bn.eps)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super(BasicBlock, self).__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        # video_frontend.py:28-41 on NHWC activations; BN side effects like nn.BatchNorm2d
        ds = self.downsample
        return ops.basic_block(x, _params(self.conv1, self.bn1), _params(self.conv2, self.bn2),
                               None if ds is None else _params(ds[0], ds[1]), self.training)


class ResNet(nn.Module):
    """layer1..layer4 of ResNet-18 (the stem lives in Lipreading), then global average pooling."""

    _STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))      # (planes, stride of the stage's first block)

    def __init__(self, block, layers):
        super(ResNet, self).__init__()
        self.inplanes = 64         # channels entering the next stage (the stem's 64)
        for i, ((planes, stride), n_blocks) in enumerate(zip(self._STAGES, layers)):
            setattr(self, "layer%d" % (i + 1), self._stage(block, planes, n_blocks, stride))
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        _he_init(self.modules())

    def _stage(self, block, planes, n_blocks, stride):
        """n_blocks blocks of `planes` channels; the first one strides and, when the shape changes, gets a 1x1 conv +
        BatchNorm projection shortcut, built before the block itself (the RNG order depends on it)."""
        width = planes * block.expansion
        shortcut = None
        if stride != 1 or self.inplanes != width:
            shortcut = nn.Sequential(nn.Conv2d(self.inplanes, width, 1, stride, bias=False), nn.BatchNorm2d(width))
        blocks = [block(self.inplanes, planes, stride, shortcut)]
        self.inplanes = width
        blocks += [block(width, planes) for _ in range(1, n_blocks)]
        return nn.Sequential(*blocks)

    def forward(self, x):
        """x: (N*T, h, w, 64) channels-last -> (N*T, 512)   (video_frontend.py:82-89)"""
        for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
            x = stage(x)
        return ops.AvgPoolFn.apply(x)


class Lipreading(nn.Module):
    """(N, 1, T, H, W) grayscale clips -> (N, T, 512) per-frame features: Conv3d 5x7x7 stem + BN + ReLU + 3x3 max-pool
    (one fused kernel), the ResNet-18 trunk per frame, then the reference's always-on dropout."""

    def __init__(self, hiddenDim=512, embedSize=256):
        super(Lipreading, self).__init__()
        self.inputDim, self.hiddenDim, self.embedSize, self.nLayers = 512, hiddenDim, embedSize, 3
        self.frontend3D = nn.Sequential(           # parameter containers of the fused stem kernel (ops.StemFn)
            nn.Conv3d(1, 64, (5, 7, 7), (1, 2, 2), (2, 3, 3), bias=False), nn.BatchNorm3d(64), nn.ReLU(True),
            nn.MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1)))
        self.resnet18 = ResNet(BasicBlock, [2, 2, 2, 2])
        # the reference's always-on F.dropout(p=0.5) (video_frontend.py:122); set to 0.0 for parity runs
        self.frontend_dropout_p = config.FRONTEND_DROPOUT_P
        _he_init(self.modules())      # again over the trunk too: its draws are overwritten but advance the RNG

    def _frontend_forward(self, x):
        """x: (N, 1, T, H, W) or (N, T, H, W) float clips, or an ops.RawClips (uint8 frames, fed to the stem as they are)
        -> (N*T, 512)"""
        if x.dim() == 5:
            x = x[:, 0]
        conv, bn = self.frontend3D[0], self.frontend3D[1]
        x = ops.StemFn.apply(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.training,
                             bn.momentum, bn.eps, bn.num_batches_tracked if self.training else None)
        return self.resnet18(x)

    def forward(self, x):
        frames = x.size(2) if x.dim() == 5 else x.size(1)
        feats = ops.dropout(self._frontend_forward(x), self.frontend_dropout_p, True)   # in eval too, like the reference
        return feats.view(-1, frames, self.inputDim)


device = config.device


def visual_frontend(pt=None):
    """A new Lipreading frontend.  With a checkpoint path: every state-dict entry of that file (tensors only) whose
    name and shape match one of the model's replaces it; everything else keeps its initial value."""
    model = Lipreading()
    if pt is None:
        return model
    own = model.state_dict()
    saved = torch.load(pt, map_location=device, weights_only=True)
    hits = {k: v for k, v in saved.items() if k in own and v.shape == own[k].shape}
    print("visual_frontend: %d of the model's %d entries loaded from %s (%d entries in the file)"
          % (len(hits), len(own), pt, len(saved)))
    model.load_state_dict({**own, **hits})
    return model
