"""MobileNetV2 backbone (the CenterMask-Lite body) on HIP kernels, behind the reference's builder names.

Mirrors centermask2/centermask/modeling/backbone/mobilenet.py: conv_bn stem :22-27, InvertedResidual :38-76, the (t, c, n, s) table
and the returned blocks 3 / 6 / 13 / 17 :79-130, builders :147-215.  The module tree reproduces the reference's state-dict keys
('features.0.0.weight', 'features.0.1.running_var', 'features.N.conv.{0,1,3,4,6,7}.*', 'conv.{0,1,3,4}' for the t = 1 block).

MI355X path, NHWC fp32, HBM-bound (thin convs, a 6x hidden tensor on either side of every depth-wise conv):
  * the stem and each expand 1x1 run on the ordinary conv kernels with their plain ReLU epilogue.  Their ReLU6 outputs are read by a
    depth-wise conv only, never returned, so the consumer applies min(., 6) while it loads: min(relu(v), 6) == relu6(v) bit for bit;
  * the depth-wise 3x3, its FrozenBN and its ReLU6 are ONE launch (ops.dwconv3x3_bn_act, csrc/dwconv_bn_act.hip);
  * the project 1x1 is linear (FrozenBN folded, no activation); the residual of a stride-1 block rides in its epilogue (res_mode 1);
  * the conv kernels take Cin % 16 == 0: the 24-channel maps (features[2], features[3] = res2) live in 32-channel buffers whose pad lanes
    the producing project conv writes as zeros (its filters, scale and shift zero-padded to 32 outputs; residual 0 + 0).  Consumers read
    the 32-wide view with zero-padded weights (PackedConv pads Cin).  No memset: the launch sequence is static and graph-capturable.
forward_views hands the (padded) views to FPN; forward slices back to the true channel counts.
"""
import torch
from torch import nn

from ... import ops
from ...ops import View
from ...registry import BACKBONE_REGISTRY
from ...structures import ShapeSpec
from ..base import Backbone, FrozenBatchNorm2d
from .fpn import FPN, LastLevelMaxPool, LastLevelP6, LastLevelP6P7

__all__ = ["MobileNetV2", "build_mnv2_backbone", "build_mobilenetv2_fpn_backbone", "build_fcos_mobilenetv2_fpn_backbone"]

# mobilenet.py:87-96: expansion t, output channels c, repeats n, stride s of the first repeat
_SETTING = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
_STEM_CH = 32
_RETURN = {3: "res2", 6: "res3", 13: "res4", 17: "res5"}            # mobilenet.py:101,130
_OUT_CHANNELS = {"res2": 24, "res3": 32, "res4": 96, "res5": 320}   # mobilenet.py:156-158
_OUT_STRIDES = {"res2": 4, "res3": 8, "res4": 16, "res5": 32}


def _pad16(c: int) -> int:
    return (c + 15) // 16 * 16


def _bias_free_conv(cin, cout, k, stride=1, groups=1):
    conv = nn.Conv2d(cin, cout, k, stride, k // 2, groups=groups, bias=False)
    nn.init.normal_(conv.weight, 0.0, (2.0 / (k * k * cout)) ** 0.5)         # mobilenet.py:135-136
    return conv


class InvertedResidual(nn.Module):
    """Parameter holder of mobilenet.py:38-76: `conv` = [expand 1x1, BN, ReLU6,] depth-wise 3x3, BN, ReLU6, project 1x1, BN."""

    def __init__(self, inp, oup, stride, expand_ratio):
        super().__init__()
        assert stride in (1, 2)
        self.inp, self.oup, self.stride = inp, oup, stride
        self.hidden = int(round(inp * expand_ratio))
        self.expand = expand_ratio != 1
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if self.expand:
            layers += [_bias_free_conv(inp, self.hidden, 1), FrozenBatchNorm2d(self.hidden), nn.ReLU6(inplace=True)]
        layers += [_bias_free_conv(self.hidden, self.hidden, 3, stride, groups=self.hidden), FrozenBatchNorm2d(self.hidden), nn.ReLU6(inplace=True),
                   _bias_free_conv(self.hidden, oup, 1), FrozenBatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)


def _folded(norm):
    return ops.fold_frozen_bn(norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.eps)


class MobileNetV2(Backbone):
    def __init__(self, cfg, n_class=1000, input_size=224, width_mult=1.0):
        super().__init__()
        del n_class                                    # the classifier of the original network is not part of the backbone
        if width_mult != 1.0:
            raise NotImplementedError("MobileNetV2 width_mult {} (the builders use 1.0; the channel padding is laid out for it)".format(width_mult))
        assert input_size % 32 == 0
        self.features = nn.ModuleList([nn.Sequential(_bias_free_conv(3, _STEM_CH, 3, 2), FrozenBatchNorm2d(_STEM_CH), nn.ReLU6(inplace=True))])
        cin = _STEM_CH
        for t, c, n, s in _SETTING:
            for i in range(n):
                self.features.append(InvertedResidual(cin, c, s if i == 0 else 1, t))
                cin = c
        for layer in self.features[:cfg.MODEL.BACKBONE.FREEZE_AT]:              # mobilenet.py:119-122
            for p in layer.parameters():
                p.requires_grad = False
        self._out_features = list(_RETURN.values())
        self._out_feature_channels = dict(_OUT_CHANNELS)
        self._out_feature_strides = dict(_OUT_STRIDES)

    # -- packed weights ------------------------------------------------------------------------------------------
    def _build_packed(self, dev):
        stem = self.features[0]
        sc, sh = _folded(stem[1])
        P = {"stem": (stem[0].weight.detach().float().cpu().permute(2, 3, 1, 0).reshape(27, -1).contiguous().to(dev), sc.to(dev), sh.to(dev)),
             "blocks": []}
        for blk in list(self.features)[1:]:
            seq = list(blk.conv)
            b = {}
            if blk.expand:
                sc, sh = _folded(seq[1])
                b["expand"] = ops.PackedConv(seq[0].weight, sc, sh, dev)       # Cin zero-padded to a multiple of 16 by the packer
                seq = seq[3:]
            sc, sh = _folded(seq[1])
            b["dw"] = (ops.pack_dw_weight(seq[0].weight).to(dev), sc.contiguous().to(dev), sh.contiguous().to(dev))
            # project conv: outputs zero-padded to the buffer width, so the pad lanes come out as 0 * 1 + 0 (+ a zero residual)
            w = seq[3].weight.detach().float().cpu()
            sc, sh = _folded(seq[4])
            cpad = _pad16(blk.oup)
            wp = torch.zeros((cpad, w.shape[1], 1, 1), dtype=torch.float32)
            wp[:blk.oup] = w
            scp, shp = torch.ones(cpad), torch.zeros(cpad)
            scp[:blk.oup], shp[:blk.oup] = sc.cpu(), sh.cpu()
            b["project"] = ops.PackedConv(wp, scp, shp, dev)
            P["blocks"].append(b)
        return P

    # -- forward ---------------------------------------------------------------------------------------------------
    def forward_views(self, x: torch.Tensor):
        """x: (N,3,H,W) float32 on the GPU -> {name: View} for the requested features (mobilenet.py:124-130).  A view is as wide as its
        buffer: res2 comes as 32 channels of which the last 8 are zeros (what FPN's zero-padded lateral weights expect)."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("MobileNetV2 expects (N,3,H,W), got {}".format(tuple(x.shape)))
        P = self.packed()
        w27, sc, sh = P["stem"]
        cur = ops.stem_conv(x.float(), w27, sc, sh)              # ReLU here; the first depth-wise conv finishes the ReLU6
        outputs = {}
        for idx, (blk, b) in enumerate(zip(list(self.features)[1:], P["blocks"]), 1):
            hid = ops.conv_out(cur, b["expand"], relu=True) if blk.expand else cur
            w9c, dsc, dsh = b["dw"]
            d = ops.dwconv3x3_bn_act(hid, w9c, dsc, dsh, stride=blk.stride, in_max=6.0, out_min=0.0, out_max=6.0)
            cur = ops.conv_out(d, b["project"], res=cur if blk.use_res_connect else None)
            name = _RETURN.get(idx)
            if name in self._out_features:
                outputs[name] = cur
        return outputs

    def forward(self, x):
        return {k: v.t[..., :self._out_feature_channels[k]].permute(0, 3, 1, 2) for k, v in self.forward_views(x).items()}


@BACKBONE_REGISTRY.register()
def build_mnv2_backbone(cfg, input_shape):
    """mobilenet.py:147-163: the bare body; the returned features are named by MODEL.RESNETS.OUT_FEATURES."""
    del input_shape
    model = MobileNetV2(cfg)
    out_features = list(cfg.MODEL.RESNETS.OUT_FEATURES)
    unknown = [f for f in out_features if f not in _OUT_CHANNELS]
    if unknown:
        raise ValueError("MODEL.RESNETS.OUT_FEATURES names {}; MobileNetV2 produces {}".format(unknown, sorted(_OUT_CHANNELS)))
    model._out_features = out_features
    return model


@BACKBONE_REGISTRY.register()
def build_mobilenetv2_fpn_backbone(cfg, input_shape: ShapeSpec):
    """mobilenet.py:166-185: MobileNetV2 + FPN with d2's LastLevelMaxPool on top."""
    bottom_up = build_mnv2_backbone(cfg, input_shape)
    return FPN(bottom_up=bottom_up, in_features=cfg.MODEL.FPN.IN_FEATURES, out_channels=cfg.MODEL.FPN.OUT_CHANNELS, norm=cfg.MODEL.FPN.NORM,
               top_block=LastLevelMaxPool(), fuse_type=cfg.MODEL.FPN.FUSE_TYPE)


@BACKBONE_REGISTRY.register()
def build_fcos_mobilenetv2_fpn_backbone(cfg, input_shape: ShapeSpec):
    """mobilenet.py:188-215: MobileNetV2 + FPN + P6/P7 (TOP_LEVELS 2), P6 (1) or nothing (0) from p5."""
    bottom_up = build_mnv2_backbone(cfg, input_shape)
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
