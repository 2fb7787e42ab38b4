"""Keypoint R-CNN head of CenterROIHeads (MODEL.KEYPOINT_ON) on HIP kernels.

Mirrors the inference half of centermask2/centermask/modeling/centermask/keypoint_head.py:
  :173-224  KRCNNConvDeconvUpsampleHead   conv_fcn1..N (3x3 + ReLU) -> MFMA convs; score_lowres, a ConvTranspose2d(k4, s2, p1), runs
                                          as ONE 3x3 conv with 4K outputs (its four output phases), see deconv4x4s2_as_conv3x3
  :219-224, :89-116  bilinear x2 + keypoint_rcnn_inference (d2 heatmaps_to_keypoints)   -> ops.keypoint_decode on the packed maps
State-dict keys equal the reference's: conv_fcn{i}.weight/bias, score_lowres.weight (Cin, K, 4, 4), score_lowres.bias.
"""
import torch
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...ops import View
from ...registry import ROI_KEYPOINT_HEAD_REGISTRY
from ...structures import ShapeSpec
from ..base import HipModule

__all__ = ["KRCNNConvDeconvUpsampleHead", "build_keypoint_head", "deconv4x4s2_as_conv3x3", "ROI_KEYPOINT_HEAD_REGISTRY"]

MAX_DECODE_S = 16          # cmk_keypoint_decode keeps the 4S x 4S map of one keypoint in LDS (cmk.h)


def deconv4x4s2_as_conv3x3(weight: torch.Tensor, bias: torch.Tensor):
    """ConvTranspose2d(Cin, K, 4, stride 2, padding 1) as a 3x3 conv (padding 1) with 4K outputs, one group of K per output phase:
    out[2a+py, 2b+px, k] = sum x[a+dy, b+dx, ci] W[ci, k, py+1-2dy, px+1-2dx] over the (dy, dx) in {-1,0,1}^2 whose kernel indices lie in
    [0, 4) — two per axis.  Returns (W3 (4K, Cin, 3, 3) with W3[(2py+px)K + k, ci, dy+1, dx+1] and zero elsewhere, the bias repeated four
    times): the channel order cmk_keypoint_decode reads.  Pure torch, any dtype / device."""
    cin, k, kh, kw = weight.shape
    assert (kh, kw) == (4, 4), "score_lowres is a 4x4 stride-2 deconvolution"
    w3 = weight.new_zeros((4 * k, cin, 3, 3))
    for py in range(2):
        for px in range(2):
            ph = (2 * py + px) * k
            for dy in (-1, 0, 1):
                ky = py + 1 - 2 * dy
                if not 0 <= ky < 4:
                    continue
                for dx in (-1, 0, 1):
                    kx = px + 1 - 2 * dx
                    if 0 <= kx < 4:
                        w3[ph:ph + k, :, dy + 1, dx + 1] = weight[:, :, ky, kx].t()
    return w3, bias.repeat(4)


@ROI_KEYPOINT_HEAD_REGISTRY.register()
class KRCNNConvDeconvUpsampleHead(HipModule):
    """keypoint_head.py:173-224 (BaseKeypointRCNNHead's loss settings are training-only and not read)."""

    def __init__(self, cfg, input_shape: ShapeSpec):
        super().__init__()
        conv_dims = tuple(cfg.MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS)
        self.num_keypoints = cfg.MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS
        self.up_scale = 2
        if self.num_keypoints < 1:
            raise ValueError("MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS must be >= 1, got {}".format(self.num_keypoints))
        s = input_shape.width
        if s is not None and not (1 <= s <= MAX_DECODE_S and s == input_shape.height):
            raise NotImplementedError("MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION {}: the keypoint decode kernel takes square RoI maps of side "
                                      "1..{} (14 in detectron2's recipe)".format(s, MAX_DECODE_S))
        in_channels = input_shape.channels
        self.num_conv = len(conv_dims)
        for idx, layer_channels in enumerate(conv_dims, 1):
            self.add_module("conv_fcn{}".format(idx), nn.Conv2d(in_channels, layer_channels, 3, stride=1, padding=1))
            in_channels = layer_channels
        self.score_lowres = nn.ConvTranspose2d(in_channels, self.num_keypoints, 4, stride=2, padding=1)
        for name, param in self.named_parameters():          # keypoint_head.py:211-217
            if "bias" in name:
                nn.init.constant_(param, 0)
            elif "weight" in name:
                nn.init.kaiming_normal_(param, mode="fan_out", nonlinearity="relu")

    def _build_packed(self, dev):
        P = {"convs": []}
        for k in range(self.num_conv):
            c = getattr(self, "conv_fcn{}".format(k + 1))
            P["convs"].append(ops.PackedConv(c.weight, None, c.bias, dev))
        w3, b3 = deconv4x4s2_as_conv3x3(self.score_lowres.weight.detach().float().cpu(), self.score_lowres.bias.detach().float().cpu())
        P["score_lowres"] = ops.PackedConv(w3, None, b3, dev)
        return P

    def features(self, x: View) -> View:
        """conv_fcn x N (ReLU) -> score_lowres in packed form: (R, S, S, 4K), channel (2py+px)K + k = logits[k, 2a+py, 2b+px]."""
        P = self.packed()
        for pc in P["convs"]:
            x = ops.conv_out(x, pc, relu=True)
        return ops.conv_out(x, P["score_lowres"])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Reference signature of `layers` (keypoint_head.py:219-224): (M, C, S, S) -> keypoint logits (M, K, 4S, 4S).  The model path
        does not come through here (it decodes the packed maps in one kernel); the depth-to-space and the bilinear x2 are torch ops."""
        k = self.num_keypoints
        m, s = x.shape[0], x.shape[2]
        if m == 0:
            return x.new_zeros((0, k, 4 * s, 4 * s))
        dec = self.features(ops.as_view(x)).t                                 # (M,S,S,4K)
        low = dec.reshape(m, s, s, 2, 2, k).permute(0, 5, 1, 3, 2, 4).reshape(m, k, 2 * s, 2 * s)
        return F.interpolate(low, scale_factor=self.up_scale, mode="bilinear", align_corners=False)


def build_keypoint_head(cfg, input_shape):
    return ROI_KEYPOINT_HEAD_REGISTRY.get(cfg.MODEL.ROI_KEYPOINT_HEAD.NAME)(cfg, input_shape)
