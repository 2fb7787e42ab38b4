"""Test tooling for the BUILD CONTAINER only, beside d2_stub.py: a plain-torch stand-in for detectron2's bottleneck ResNet.

detectron2 is not in this image, and the reference's `build_fcos_resnet_fpn_backbone` (modeling/backbone/fpn.py:56-87) builds its
bottom-up with `detectron2.modeling.backbone.build_resnet_backbone`.  BasicStem, BottleneckBlock, ResNet and build_resnet_backbone
below are written from detectron2 ~0.5's public behaviour (module names and registration order, strides, the max-pool of the stem,
FrozenBN without conv bias), on d2_stub's Conv2d / FrozenBatchNorm2d / Backbone, like the FPN and DCN stand-ins: fixtures produced
through them stay "parity unpinned" against a real detectron2.  They are ordinary torch modules that compute with F.conv2d; nothing
here is shared with centermask2_amd/modeling/backbone/resnet.py, which only holds parameters and launches kernels.
"""
import torch.nn.functional as F
from torch import nn

import d2_stub
from d2_stub import Backbone, Conv2d, get_norm

_BLOCKS_PER_STAGE = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3], 152: [3, 8, 36, 3]}


class BasicStem(nn.Module):
    def __init__(self, in_channels=3, out_channels=64, norm="BN"):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, 4
        self.conv1 = Conv2d(in_channels, out_channels, kernel_size=7, stride=2, padding=3, bias=False, norm=get_norm(norm, out_channels))

    def forward(self, x):
        x = self.conv1(x)
        x = F.relu_(x)
        return F.max_pool2d(x, kernel_size=3, stride=2, padding=1)


class BottleneckBlock(nn.Module):
    def __init__(self, in_channels, out_channels, *, bottleneck_channels, stride=1, num_groups=1, norm="BN", stride_in_1x1=False, dilation=1):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        if in_channels != out_channels:
            self.shortcut = Conv2d(in_channels, out_channels, kernel_size=1, stride=stride, bias=False, norm=get_norm(norm, out_channels))
        else:
            self.shortcut = None
        stride_1x1, stride_3x3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = Conv2d(in_channels, bottleneck_channels, kernel_size=1, stride=stride_1x1, bias=False, norm=get_norm(norm, bottleneck_channels))
        self.conv2 = Conv2d(bottleneck_channels, bottleneck_channels, kernel_size=3, stride=stride_3x3, padding=1 * dilation, bias=False,
                            groups=num_groups, dilation=dilation, norm=get_norm(norm, bottleneck_channels))
        self.conv3 = Conv2d(bottleneck_channels, out_channels, kernel_size=1, bias=False, norm=get_norm(norm, out_channels))

    def forward(self, x):
        out = F.relu_(self.conv1(x))
        out = F.relu_(self.conv2(out))
        out = self.conv3(out)
        shortcut = self.shortcut(x) if self.shortcut is not None else x
        out += shortcut
        return F.relu_(out)


class ResNet(Backbone):
    def __init__(self, stem, stages, out_features):
        super().__init__()
        self.stem = stem
        self._out_feature_strides = {"stem": stem.stride}
        self._out_feature_channels = {"stem": stem.out_channels}
        self.stage_names, self.stages = [], []
        current_stride = stem.stride
        for i, blocks in enumerate(stages):
            name = "res" + str(i + 2)
            stage = nn.Sequential(*blocks)
            self.add_module(name, stage)
            self.stage_names.append(name)
            self.stages.append(stage)
            for b in blocks:
                current_stride *= b.stride
            self._out_feature_strides[name] = current_stride
            self._out_feature_channels[name] = blocks[-1].out_channels
        self._out_features = list(out_features)
        for f in self._out_features:
            assert f in self._out_feature_strides, f

    def forward(self, x):
        outputs = {}
        x = self.stem(x)
        if "stem" in self._out_features:
            outputs["stem"] = x
        for name, stage in zip(self.stage_names, self.stages):
            x = stage(x)
            if name in self._out_features:
                outputs[name] = x
        return outputs


def build_resnet_backbone(cfg, input_shape):
    r = cfg.MODEL.RESNETS
    norm = r.NORM
    stem = BasicStem(in_channels=input_shape.channels, out_channels=r.STEM_OUT_CHANNELS, norm=norm)
    out_features = r.OUT_FEATURES
    assert r.RES5_DILATION == 1 and not any(r.DEFORM_ON_PER_STAGE) and r.DEPTH in _BLOCKS_PER_STAGE
    bottleneck_channels = r.NUM_GROUPS * r.WIDTH_PER_GROUP
    in_channels, out_channels = r.STEM_OUT_CHANNELS, r.RES2_OUT_CHANNELS
    max_stage_idx = max({"res2": 2, "res3": 3, "res4": 4, "res5": 5}[f] for f in out_features if f != "stem")
    stages = []
    for idx, stage_idx in enumerate(range(2, max_stage_idx + 1)):
        first_stride = 1 if idx == 0 else 2
        blocks = []
        for i in range(_BLOCKS_PER_STAGE[r.DEPTH][idx]):
            blocks.append(BottleneckBlock(in_channels, out_channels, bottleneck_channels=bottleneck_channels, stride=first_stride if i == 0 else 1,
                                          num_groups=r.NUM_GROUPS, norm=norm, stride_in_1x1=r.STRIDE_IN_1X1))
            in_channels = out_channels
        stages.append(blocks)
        out_channels *= 2
        bottleneck_channels *= 2
    model = ResNet(stem, stages, out_features)
    for p in ([stem] if cfg.MODEL.BACKBONE.FREEZE_AT >= 1 else []) + [s for i, s in enumerate(model.stages, 2) if cfg.MODEL.BACKBONE.FREEZE_AT >= i]:
        for q in p.parameters():
            q.requires_grad = False
    return model


def build_resnet_fpn_backbone(cfg, input_shape):
    """detectron2's plain FPN builder: ResNet + FPN + LastLevelMaxPool."""
    bottom_up = build_resnet_backbone(cfg, input_shape)
    return d2_stub.FPN(bottom_up=bottom_up, in_features=cfg.MODEL.FPN.IN_FEATURES, out_channels=cfg.MODEL.FPN.OUT_CHANNELS, norm=cfg.MODEL.FPN.NORM,
                       top_block=d2_stub.LastLevelMaxPool(), fuse_type=cfg.MODEL.FPN.FUSE_TYPE)
