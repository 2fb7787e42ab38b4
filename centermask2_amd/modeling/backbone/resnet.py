"""ResNet-50 / 101 / 152 and ResNeXt backbones (detectron2's bottleneck ResNet) on HIP kernels, behind d2's and the reference's builder names.

centermask2/centermask/modeling/backbone/fpn.py:56-87 builds `build_fcos_resnet_fpn_backbone` on detectron2's `build_resnet_backbone`;
the module tree below reproduces d2's state-dict keys ('stem.conv1.weight', 'stem.conv1.norm.*', 'res{2..5}.{i}.conv{1,2,3}.*' and
'res{s}.0.shortcut.*' in the first block of a stage, the shortcut registered first as in d2), FrozenBN with eps 1e-5, no conv bias.

MI355X path, NHWC fp32:
  * the stem (7x7 stride-2 conv, FrozenBN, ReLU, max_pool2d(3, 2, 1)) is ONE launch, ops.stem7x7_bn_relu_maxpool (csrc/stem7_pool.hip):
    the (N, H/2, W/2, 64) conv map is never written;
  * a bottleneck is three launches of the ordinary conv kernels with the FrozenBN folded: relu(conv1), relu(conv2), and conv3 with the
    shortcut as the residual of its epilogue and the block's last ReLU behind the sum (res_mode 1, relu);
  * the pointwise kernels take no stride, so a down-sampling block first keeps every second pixel of its input (ops.maxpool1x1s2, one
    launch per down-sampling block, three per network) and feeds `shortcut` — and `conv1` under STRIDE_IN_1X1 — from that view.  With
    STRIDE_IN_1X1 False the stride sits on the 3x3 conv2, which the conv kernels take;
  * with MODEL.RESNETS.NUM_GROUPS > 1 (ResNeXt: X-50-32x4d, X-101-32x4d / 64x4d / 32x8d) conv2 is a grouped 3x3, one launch of
    ops.group_conv3x3 (csrc/conv_group3.hip) at stride 1 or 2 with the FrozenBN and the ReLU in its epilogue; every built stage must have
    Cg = WIDTH_PER_GROUP * 2^(stage-2) in {4, 8, 16, 32, 64}.
No memsets, no host syncs: the launch sequence is static and graph-capturable.
"""
import torch
from torch import nn

from ... import ops
from ...registry import BACKBONE_REGISTRY
from ...structures import ShapeSpec
from ..base import Backbone, FrozenBatchNorm2d, NormConv2d
from .fpn import FPN, LastLevelMaxPool, LastLevelP6, LastLevelP6P7
from .mobilenet import build_mnv2_backbone

__all__ = ["ResNet", "BasicStem", "BottleneckBlock", "build_resnet_backbone", "build_resnet_fpn_backbone", "build_fcos_resnet_fpn_backbone"]

_BLOCKS_PER_STAGE = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
_STAGES = ("res2", "res3", "res4", "res5")


def _conv_bn(cin, cout, k, stride=1, groups=1):
    return NormConv2d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=False, groups=groups, norm=FrozenBatchNorm2d(cout))


class BasicStem(nn.Module):
    """Parameter holder of d2's BasicStem: conv1 7x7 stride 2 (+ FrozenBN); ReLU and max_pool2d(3, 2, 1) have no parameters."""

    def __init__(self, in_channels=3, out_channels=64):
        super().__init__()
        self.conv1 = _conv_bn(in_channels, out_channels, 7, 2)


class BottleneckBlock(nn.Module):
    """Parameter holder of d2's BottleneckBlock: [shortcut 1x1,] conv1 1x1, conv2 3x3, conv3 1x1, each with a FrozenBN.  num_groups > 1
    (ResNeXt) makes conv2 a grouped conv with a (width, width / num_groups, 3, 3) weight."""

    def __init__(self, in_channels, out_channels, bottleneck_channels, stride, stride_in_1x1, num_groups=1):
        super().__init__()
        assert stride in (1, 2)
        self.stride, self.stride_in_1x1, self.num_groups = stride, stride_in_1x1, num_groups
        self.shortcut = _conv_bn(in_channels, out_channels, 1, stride) if in_channels != out_channels else None
        stride_1x1, stride_3x3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = _conv_bn(in_channels, bottleneck_channels, 1, stride_1x1)
        self.conv2 = _conv_bn(bottleneck_channels, bottleneck_channels, 3, stride_3x3, num_groups)
        self.conv3 = _conv_bn(bottleneck_channels, out_channels, 1)


def _packed_conv(conv, dev, stride=1):
    norm = conv.norm
    scale, shift = ops.fold_frozen_bn(norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.eps)
    return ops.PackedConv(conv.weight, scale, shift, dev, stride=stride)


def _packed_group_conv(conv, dev, groups, stride=1):
    norm = conv.norm
    scale, shift = ops.fold_frozen_bn(norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.eps)
    return ops.PackedGroupConv(conv.weight, scale, shift, dev, groups, stride=stride)


class ResNet(Backbone):
    def __init__(self, cfg, out_features):
        super().__init__()
        r = cfg.MODEL.RESNETS
        if r.DEPTH not in _BLOCKS_PER_STAGE:
            raise NotImplementedError("MODEL.RESNETS.DEPTH {}: the bottleneck depths 50, 101 and 152 are built (18 and 34 are basic-block networks)".format(r.DEPTH))
        if r.RES5_DILATION != 1:
            raise NotImplementedError("MODEL.RESNETS.RES5_DILATION {}: a dilated res5 is not built".format(r.RES5_DILATION))
        if any(r.DEFORM_ON_PER_STAGE):
            raise NotImplementedError("MODEL.RESNETS.DEFORM_ON_PER_STAGE {}: deformable ResNet stages are not built".format(list(r.DEFORM_ON_PER_STAGE)))
        if r.NORM != "FrozenBN":
            raise NotImplementedError("MODEL.RESNETS.NORM '{}': the ResNet body folds FrozenBN into its convs".format(r.NORM))
        if r.STEM_OUT_CHANNELS != 64:
            raise NotImplementedError("MODEL.RESNETS.STEM_OUT_CHANNELS {}: the fused stem kernel has 64 outputs".format(r.STEM_OUT_CHANNELS))
        width = r.NUM_GROUPS * r.WIDTH_PER_GROUP
        if width % 16 and r.NUM_GROUPS != 1:
            raise NotImplementedError("MODEL.RESNETS.NUM_GROUPS {} x WIDTH_PER_GROUP {} = {}: the conv kernels take channel counts that are multiples "
                                      "of 16".format(r.NUM_GROUPS, r.WIDTH_PER_GROUP, width))
        if width % 16:
            raise NotImplementedError("MODEL.RESNETS.WIDTH_PER_GROUP {}: the conv kernels take channel counts that are multiples of 16".format(r.WIDTH_PER_GROUP))
        if r.RES2_OUT_CHANNELS % 16:
            raise NotImplementedError("MODEL.RESNETS.RES2_OUT_CHANNELS {}: the conv kernels take channel counts that are multiples of 16".format(r.RES2_OUT_CHANNELS))
        out_features = list(out_features)
        unknown = [f for f in out_features if f != "stem" and f not in _STAGES]
        if unknown or not out_features:
            raise NotImplementedError("MODEL.RESNETS.OUT_FEATURES {}: a ResNet produces 'stem' and {}".format(out_features, list(_STAGES)))
        last = max([_STAGES.index(f) for f in out_features if f != "stem"] + [-1])     # d2 builds no stage past the last one asked for
        if r.NUM_GROUPS != 1:                                                         # ResNeXt: conv2 runs on the grouped 3x3 kernel
            for si in range(last + 1):
                if r.NUM_GROUPS < 2 or not ops.group_conv_supported(width << si, r.NUM_GROUPS):
                    raise NotImplementedError("MODEL.RESNETS.NUM_GROUPS {} with WIDTH_PER_GROUP {}: {} has Cg = {} channels per group; the grouped 3x3 "
                                              "kernel takes {}".format(r.NUM_GROUPS, r.WIDTH_PER_GROUP, _STAGES[si], r.WIDTH_PER_GROUP << si,
                                                                       list(ops.GROUP_CONV_CG)))
        self.stem = BasicStem(3, r.STEM_OUT_CHANNELS)
        self._out_feature_channels = {"stem": r.STEM_OUT_CHANNELS}
        self._out_feature_strides = {"stem": 4}
        self.stage_names = []
        cin, cout, stride = r.STEM_OUT_CHANNELS, r.RES2_OUT_CHANNELS, 4
        for si, name in enumerate(_STAGES[:last + 1]):
            blocks = []
            for i in range(_BLOCKS_PER_STAGE[r.DEPTH][si]):
                blocks.append(BottleneckBlock(cin, cout, width, 2 if (i == 0 and si > 0) else 1, bool(r.STRIDE_IN_1X1), r.NUM_GROUPS))
                cin = cout
            self.add_module(name, nn.Sequential(*blocks))
            self.stage_names.append(name)
            stride *= 2 if si > 0 else 1
            self._out_feature_channels[name], self._out_feature_strides[name] = cout, stride
            cout, width = cout * 2, width * 2
        self._out_features = out_features
        frozen = ([self.stem] if cfg.MODEL.BACKBONE.FREEZE_AT >= 1 else []) + \
                 [getattr(self, n) for i, n in enumerate(self.stage_names, 2) if cfg.MODEL.BACKBONE.FREEZE_AT >= i]
        for m in frozen:                                                              # FREEZE_AT only clears requires_grad
            for p in m.parameters():
                p.requires_grad = False

    def _build_packed(self, dev):
        conv = self.stem.conv1
        sc, sh = ops.fold_frozen_bn(conv.norm.weight, conv.norm.bias, conv.norm.running_mean, conv.norm.running_var, conv.norm.eps)
        P = {"stem": (ops.pack_stem7_weight(conv.weight).to(dev), sc.contiguous().to(dev), sh.contiguous().to(dev))}
        for name in self.stage_names:
            P[name] = []
            for blk in getattr(self, name):
                s2 = 1 if blk.stride_in_1x1 else blk.stride
                b = {"conv1": _packed_conv(blk.conv1, dev), "conv3": _packed_conv(blk.conv3, dev),
                     "conv2": _packed_group_conv(blk.conv2, dev, blk.num_groups, s2) if blk.num_groups > 1 else _packed_conv(blk.conv2, dev, stride=s2)}
                if blk.shortcut is not None:
                    b["shortcut"] = _packed_conv(blk.shortcut, dev)
                P[name].append(b)
        return P

    def forward_views(self, x: torch.Tensor):
        """x: (N,3,H,W) float32 on the GPU -> {name: View} for the requested features."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("ResNet expects (N,3,H,W), got {}".format(tuple(x.shape)))
        P = self.packed()
        w147, sc, sh = P["stem"]
        cur = ops.stem7x7_bn_relu_maxpool(x.float(), w147, sc, sh)
        outputs = {}
        if "stem" in self._out_features:
            outputs["stem"] = cur
        for name in self.stage_names:
            for blk, b in zip(getattr(self, name), P[name]):
                sub = ops.maxpool1x1s2(cur) if blk.stride == 2 else cur     # what a stride-2 1x1 conv reads
                h = ops.conv_out(sub if blk.stride_in_1x1 else cur, b["conv1"], relu=True)
                h = ops.group_conv3x3(h, b["conv2"], relu=True) if blk.num_groups > 1 else ops.conv_out(h, b["conv2"], relu=True)
                short = ops.conv_out(sub, b["shortcut"]) if blk.shortcut is not None else cur
                cur = ops.conv_out(h, b["conv3"], res=short, relu=True)    # relu(conv3 + shortcut)
            if name in self._out_features:
                outputs[name] = cur
        return {k: outputs[k] for k in self._out_features}

    def forward(self, x):
        return {k: v.nchw() for k, v in self.forward_views(x).items()}


@BACKBONE_REGISTRY.register()
def build_resnet_backbone(cfg, input_shape):
    """detectron2's builder: the bare body; MODEL.RESNETS.OUT_FEATURES names the returned features."""
    del input_shape
    return ResNet(cfg, cfg.MODEL.RESNETS.OUT_FEATURES)


@BACKBONE_REGISTRY.register()
def build_resnet_fpn_backbone(cfg, input_shape: ShapeSpec):
    """detectron2's builder: ResNet + FPN with LastLevelMaxPool on top (p2..p6 over res2..res5, the keypoint head's default levels)."""
    bottom_up = build_resnet_backbone(cfg, input_shape)
    return FPN(bottom_up=bottom_up, in_features=cfg.MODEL.FPN.IN_FEATURES, out_channels=cfg.MODEL.FPN.OUT_CHANNELS, norm=cfg.MODEL.FPN.NORM,
               top_block=LastLevelMaxPool(), fuse_type=cfg.MODEL.FPN.FUSE_TYPE)


@BACKBONE_REGISTRY.register()
def build_fcos_resnet_fpn_backbone(cfg, input_shape: ShapeSpec):
    """fpn.py:56-87: ResNet + FPN + P6/P7 (TOP_LEVELS 2), P6 (1) or nothing (0) from p5.  With MODEL.MOBILENET the reference's line 66
    calls `build_mnv2_backbone`, a name that module never imports; it means the MobileNetV2 body, which is what runs here."""
    bottom_up = build_mnv2_backbone(cfg, input_shape) if cfg.MODEL.MOBILENET else build_resnet_backbone(cfg, input_shape)
    out_channels = cfg.MODEL.FPN.OUT_CHANNELS
    top_levels = cfg.MODEL.FCOS.TOP_LEVELS
    if top_levels == 2:
        top_block = LastLevelP6P7(out_channels, out_channels, "p5")
    elif top_levels == 1:
        top_block = LastLevelP6(out_channels, out_channels, "p5")
    elif top_levels == 0:
        top_block = None
    else:
        raise ValueError("MODEL.FCOS.TOP_LEVELS must be 0, 1 or 2")
    return FPN(bottom_up=bottom_up, in_features=cfg.MODEL.FPN.IN_FEATURES, out_channels=out_channels, norm=cfg.MODEL.FPN.NORM,
               top_block=top_block, fuse_type=cfg.MODEL.FPN.FUSE_TYPE)
