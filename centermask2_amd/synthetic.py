"""Seeded synthetic weights and inputs; data generation only, no compute path.

No checkpoint or dataset is reachable offline (the reference's weights are Dropbox URLs,
README.md:173,254), so parity and the benchmark run on random-init weights written under the
reference's state-dict key names and on uint8-valued BGR noise images preprocessed like
deploy_utils.py:76-83.  Every tensor is drawn from its own generator seeded by
crc32(key) ^ seed, so the values do not depend on the enumeration order or on who enumerates.
"""
import math
import zlib
from collections import OrderedDict
from typing import Dict, Iterable, Tuple

import torch

# vovnet.py:30-108
STAGE_SPECS = {
    "V-19-slim-dw-eSE": dict(stem=[64, 64, 64], stage_conv_ch=[64, 80, 96, 112], stage_out_ch=[112, 256, 384, 512],
                             layer_per_block=3, block_per_stage=[1, 1, 1, 1], dw=True),
    "V-19-dw-eSE": dict(stem=[64, 64, 64], stage_conv_ch=[128, 160, 192, 224], stage_out_ch=[256, 512, 768, 1024],
                        layer_per_block=3, block_per_stage=[1, 1, 1, 1], dw=True),
    "V-19-slim-eSE": dict(stem=[64, 64, 128], stage_conv_ch=[64, 80, 96, 112], stage_out_ch=[112, 256, 384, 512],
                          layer_per_block=3, block_per_stage=[1, 1, 1, 1]),
    "V-19-eSE": dict(stem=[64, 64, 128], stage_conv_ch=[128, 160, 192, 224], stage_out_ch=[256, 512, 768, 1024],
                     layer_per_block=3, block_per_stage=[1, 1, 1, 1]),
    "V-39-eSE": dict(stem=[64, 64, 128], stage_conv_ch=[128, 160, 192, 224], stage_out_ch=[256, 512, 768, 1024],
                     layer_per_block=5, block_per_stage=[1, 1, 2, 2]),
    "V-57-eSE": dict(stem=[64, 64, 128], stage_conv_ch=[128, 160, 192, 224], stage_out_ch=[256, 512, 768, 1024],
                     layer_per_block=5, block_per_stage=[1, 1, 4, 3]),
    "V-99-eSE": dict(stem=[64, 64, 128], stage_conv_ch=[128, 160, 192, 224], stage_out_ch=[256, 512, 768, 1024],
                     layer_per_block=5, block_per_stage=[1, 3, 9, 3]),
}

PIXEL_MEAN = (103.53, 116.28, 123.675)  # deploy_utils.py:81 (BGR), std 1

MOBILENETV2 = "MobileNetV2"             # conv_body name of the CenterMask-Lite body (mobilenet.py:79-130); it has no MODEL.VOVNET entry
# mobilenet.py:87-96 (t, c, n, s) and the channel counts of res2..res5 (:156-158)
MNV2_SETTING = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
MNV2_OUT_CHANNELS = {"res2": 24, "res3": 32, "res4": 96, "res5": 320}


def mobilenetv2_param_shapes(prefix: str = "") -> "OrderedDict[str, Tuple[int, ...]]":
    """State-dict entries of the bare MobileNetV2 body in the reference's key names and order (mobilenet.py:22-27, 38-70)."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def bn(key: str, c: int) -> None:
        for n in ("weight", "bias", "running_mean", "running_var"):
            s["{}.{}".format(key, n)] = (c,)

    s[prefix + "features.0.0.weight"] = (32, 3, 3, 3)
    bn(prefix + "features.0.1", 32)
    cin, idx = 32, 1
    for t, c, n, _ in MNV2_SETTING:
        for _ in range(n):
            p, hidden, i = prefix + "features.{}.conv.".format(idx), cin * t, 0
            if t != 1:
                s[p + "0.weight"] = (hidden, cin, 1, 1)
                bn(p + "1", hidden)
                i = 3
            s[p + "{}.weight".format(i)] = (hidden, 1, 3, 3)
            bn(p + str(i + 1), hidden)
            s[p + "{}.weight".format(i + 3)] = (c, hidden, 1, 1)
            bn(p + str(i + 4), c)
            cin, idx = c, idx + 1
    return s


RESNET_DEPTHS = {"R-50": 50, "R-101": 101, "R-152": 152}      # conv_body names of the detectron2 bottleneck ResNets (MODEL.RESNETS.DEPTH)
RESNET_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
# ResNeXt bodies: name -> (MODEL.RESNETS.DEPTH, NUM_GROUPS, WIDTH_PER_GROUP); conv2 of every bottleneck is a grouped 3x3
RESNEXT_BODIES = {"X-50-32x4d": (50, 32, 4), "X-101-32x4d": (101, 32, 4), "X-101-64x4d": (101, 64, 4), "X-101-32x8d": (101, 32, 8)}


def resnet_body(conv_body: str):
    """(depth, groups, width per group) of a ResNet / ResNeXt conv_body name, or None for any other body."""
    if conv_body in RESNET_DEPTHS:
        return RESNET_DEPTHS[conv_body], 1, 64
    return RESNEXT_BODIES.get(conv_body)


def resnet_param_shapes(depth: int = 50, prefix: str = "", last_stage: int = 5, res2_out: int = 256, width: int = 64,
                        groups: int = 1) -> "OrderedDict[str, Tuple[int, ...]]":
    """State-dict entries of detectron2's bottleneck ResNet up to res<last_stage>, in d2's key names and order (the shortcut of a stage's
    first block is registered before its conv1).  width: NUM_GROUPS * WIDTH_PER_GROUP; groups > 1 (ResNeXt) makes conv2 a grouped 3x3."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def conv_bn(key: str, cin: int, cout: int, k: int, g: int = 1) -> None:
        s[key + ".weight"] = (cout, cin // g, k, k)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s["{}.norm.{}".format(key, n)] = (cout,)

    conv_bn(prefix + "stem.conv1", 3, 64, 7)
    cin, cout = 64, res2_out
    for stage, blocks in zip(range(2, last_stage + 1), RESNET_BLOCKS[depth]):
        for i in range(blocks):
            p = "{}res{}.{}.".format(prefix, stage, i)
            if cin != cout:
                conv_bn(p + "shortcut", cin, cout, 1)
            conv_bn(p + "conv1", cin, width, 1)
            conv_bn(p + "conv2", width, width, 3, groups)
            conv_bn(p + "conv3", width, cout, 1)
            cin = cout
        cout, width = cout * 2, width * 2
    return s


def model_param_shapes(conv_body: str = "V-39-eSE", num_classes: int = 80, fpn_ch: int = 256,
                       mask_dim: int = 256, pooler_res: int = 14, stage_with_dcn=(False, False, False, False),
                       with_modulated_dcn: bool = False, deformable_groups: int = 1, keypoint_on: bool = False,
                       keypoint_conv_dims=(512,) * 8, num_keypoints: int = 17, fpn_in=("res3", "res4", "res5"), top_levels: int = 2,
                       num_tower_convs: int = 4, mask_num_conv: int = 4, maskiou_num_conv: int = 4) -> "OrderedDict[str, Tuple[int, ...]]":
    """Every state-dict entry of the full model in the reference's key names (SURVEY §5 'checkpoint').
    keypoint_on / keypoint_conv_dims / num_keypoints: MODEL.KEYPOINT_ON and MODEL.ROI_KEYPOINT_HEAD.{CONV_DIMS, NUM_KEYPOINTS}: the
    `roi_heads.keypoint_head.*` entries of KRCNNConvDeconvUpsampleHead (keypoint_head.py:198-208), after everything else.
    stage_with_dcn / with_modulated_dcn / deformable_groups: MODEL.VOVNET.STAGE_WITH_DCN etc.; the 3x3 layers of a flagged stage are
    DFConv3x3 (vovnet.py:132-201: '/conv_offset' with bias, '/conv', '/norm'), except in the depth-wise bodies (vovnet.py:292-298).
    conv_body "MobileNetV2": the CenterMask-Lite body behind build_fcos_mobilenetv2_fpn_backbone, FPN laterals over `fpn_in`
    (MODEL.FPN.IN_FEATURES) and `top_levels` (MODEL.FCOS.TOP_LEVELS) top convs.  conv_body "R-50" / "R-101" / "R-152": detectron2's
    bottleneck ResNet behind build_fcos_resnet_fpn_backbone at d2's default widths, with the same `fpn_in` / `top_levels`; the RESNEXT_BODIES names
    ("X-101-32x8d", ...) are its grouped (ResNeXt) members.  num_tower_convs / mask_num_conv / maskiou_num_conv:
    MODEL.FCOS.NUM_{CLS,BOX}_CONVS, MODEL.ROI_MASK_HEAD.NUM_CONV, MODEL.ROI_MASKIOU_HEAD.NUM_CONV; fpn_ch and mask_dim the widths."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    if conv_body == MOBILENETV2:
        s.update(mobilenetv2_param_shapes("backbone.bottom_up."))
        _fpn_shapes(s, [(int(f[3:]), MNV2_OUT_CHANNELS[f]) for f in fpn_in], fpn_ch, top_levels)
    elif resnet_body(conv_body) is not None:
        depth, groups, wpg = resnet_body(conv_body)
        s.update(resnet_param_shapes(depth, "backbone.bottom_up.", last_stage=max(int(f[3:]) for f in fpn_in), width=groups * wpg, groups=groups))
        _fpn_shapes(s, [(int(f[3:]), 2 ** (int(f[3:]) + 6)) for f in fpn_in], fpn_ch, top_levels)
    else:
        _vovnet_shapes(s, STAGE_SPECS[conv_body], stage_with_dcn, with_modulated_dcn, deformable_groups)
        _fpn_shapes(s, list(zip((3, 4, 5), STAGE_SPECS[conv_body]["stage_out_ch"][1:])), fpn_ch, 2)
    _head_shapes(s, num_classes, fpn_ch, mask_dim, pooler_res, num_tower_convs, mask_num_conv, maskiou_num_conv, keypoint_on,
                 keypoint_conv_dims, num_keypoints)
    return s


def _vovnet_shapes(s, spec, stage_with_dcn, with_modulated_dcn, deformable_groups) -> None:

    def conv_bn(prefix: str, cin: int, cout: int, k: int) -> None:
        s[prefix + "/conv.weight"] = (cout, cin, k, k)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[prefix + "/norm." + n] = (cout,)

    def dw_pw_bn(prefix: str, c: int) -> None:      # dw_conv3x3 vovnet.py:110-130
        s[prefix + "/dw_conv3x3.weight"] = (c, 1, 3, 3)
        s[prefix + "/pw_conv1x1.weight"] = (c, c, 1, 1)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[prefix + "/pw_norm." + n] = (c,)

    dw = spec.get("dw", False)
    bu = "backbone.bottom_up."
    stem = spec["stem"]
    conv_bn(bu + "stem.stem_1", 3, stem[0], 3)
    if dw:
        assert stem[0] == stem[1] == stem[2]
        dw_pw_bn(bu + "stem.stem_2", stem[1])
        dw_pw_bn(bu + "stem.stem_3", stem[2])
    else:
        conv_bn(bu + "stem.stem_2", stem[0], stem[1], 3)
        conv_bn(bu + "stem.stem_3", stem[1], stem[2], 3)
    in_ch = stem[2]
    for si in range(4):
        stage_ch, concat_ch = spec["stage_conv_ch"][si], spec["stage_out_ch"][si]
        for b in range(spec["block_per_stage"][si]):
            mod = "OSA{}_{}".format(si + 2, b + 1)
            p = bu + "stage{}.{}.".format(si + 2, mod)
            cin = in_ch
            if dw and in_ch != stage_ch:            # conv_reduction vovnet.py:284-288
                conv_bn(p + "conv_reduction.{}_reduction_0".format(mod), in_ch, stage_ch, 1)
            for i in range(spec["layer_per_block"]):
                if dw:
                    dw_pw_bn(p + "layers.{}.{}_{}".format(i, mod, i), stage_ch)
                elif stage_with_dcn[si]:
                    q = p + "layers.{}.{}_{}".format(i, mod, i)
                    s[q + "/conv_offset.weight"] = ((27 if with_modulated_dcn else 18) * deformable_groups, cin, 3, 3)
                    s[q + "/conv_offset.bias"] = ((27 if with_modulated_dcn else 18) * deformable_groups,)
                    conv_bn(q, cin, stage_ch, 3)
                else:
                    conv_bn(p + "layers.{}.{}_{}".format(i, mod, i), cin, stage_ch, 3)
                cin = stage_ch
            conv_bn(p + "concat.{}_concat".format(mod), in_ch + spec["layer_per_block"] * stage_ch, concat_ch, 1)
            s[p + "ese.fc.weight"] = (concat_ch, concat_ch, 1, 1)
            s[p + "ese.fc.bias"] = (concat_ch,)
            in_ch = concat_ch


def _fpn_shapes(s, levels, fpn_ch, top_levels) -> None:
    for lvl, cin in levels:
        s["backbone.fpn_lateral{}.weight".format(lvl)] = (fpn_ch, cin, 1, 1)
        s["backbone.fpn_lateral{}.bias".format(lvl)] = (fpn_ch,)
        s["backbone.fpn_output{}.weight".format(lvl)] = (fpn_ch, fpn_ch, 3, 3)
        s["backbone.fpn_output{}.bias".format(lvl)] = (fpn_ch,)
    for n in ("p6", "p7")[:top_levels]:
        s["backbone.top_block.{}.weight".format(n)] = (fpn_ch, fpn_ch, 3, 3)
        s["backbone.top_block.{}.bias".format(n)] = (fpn_ch,)


def _head_shapes(s, num_classes, fpn_ch, mask_dim, pooler_res, num_tower_convs, mask_num_conv, maskiou_num_conv, keypoint_on,
                 keypoint_conv_dims, num_keypoints) -> None:
    h = "proposal_generator.fcos_head."
    for tower in ("cls_tower", "bbox_tower"):
        for k in range(num_tower_convs):
            s[h + "{}.{}.weight".format(tower, 3 * k)] = (fpn_ch, fpn_ch, 3, 3)
            s[h + "{}.{}.bias".format(tower, 3 * k)] = (fpn_ch,)
            s[h + "{}.{}.weight".format(tower, 3 * k + 1)] = (fpn_ch,)
            s[h + "{}.{}.bias".format(tower, 3 * k + 1)] = (fpn_ch,)
    for n, c in (("cls_logits", num_classes), ("bbox_pred", 4), ("ctrness", 1)):
        s[h + n + ".weight"] = (c, fpn_ch, 3, 3)
        s[h + n + ".bias"] = (c,)
    for l in range(5):
        s[h + "scales.{}.scale".format(l)] = (1,)
    m = "roi_heads.mask_head."
    for k in range(mask_num_conv):
        s[m + "mask_fcn{}.weight".format(k + 1)] = (mask_dim, fpn_ch if k == 0 else mask_dim, 3, 3)
        s[m + "mask_fcn{}.bias".format(k + 1)] = (mask_dim,)
    s[m + "spatialAtt.conv.weight"] = (1, 2, 3, 3)
    s[m + "deconv.weight"] = (mask_dim, mask_dim, 2, 2)
    s[m + "deconv.bias"] = (mask_dim,)
    s[m + "predictor.weight"] = (num_classes, mask_dim, 1, 1)
    s[m + "predictor.bias"] = (num_classes,)
    q = "roi_heads.maskiou_head."
    for k in range(maskiou_num_conv):
        s[q + "maskiou_fcn{}.weight".format(k + 1)] = (mask_dim, fpn_ch + 1 if k == 0 else mask_dim, 3, 3)
        s[q + "maskiou_fcn{}.bias".format(k + 1)] = (mask_dim,)
    res = pooler_res // 2
    s[q + "maskiou_fc1.weight"] = (1024, mask_dim * res * res)
    s[q + "maskiou_fc1.bias"] = (1024,)
    s[q + "maskiou_fc2.weight"] = (1024, 1024)
    s[q + "maskiou_fc2.bias"] = (1024,)
    s[q + "maskiou.weight"] = (num_classes, 1024)
    s[q + "maskiou.bias"] = (num_classes,)
    if keypoint_on:
        kp, cin = "roi_heads.keypoint_head.", fpn_ch
        for i, c in enumerate(keypoint_conv_dims, 1):
            s[kp + "conv_fcn{}.weight".format(i)] = (c, cin, 3, 3)
            s[kp + "conv_fcn{}.bias".format(i)] = (c,)
            cin = c
        s[kp + "score_lowres.weight"] = (cin, num_keypoints, 4, 4)          # ConvTranspose2d: (Cin, Cout, kh, kw)
        s[kp + "score_lowres.bias"] = (num_keypoints,)


# Frozen fixture constants (chosen once with the oracle so that every fixture image yields a few
# thousand candidates > 0.05 and >= 50 post-NMS detections spread over the three ROI levels).
SYNTH = dict(cls_logits_std=0.035, cls_logits_bias=-5.6, bbox_pred_std=0.05, bbox_pred_bias=1.0,
             ctrness_std=0.03, predictor_std=0.5, maskiou_std=0.002, scale_lo=6.0, scale_hi=12.0)


def _gen(name: str, seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed((zlib.crc32(name.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
    return g


def synthetic_tensor(name: str, shape: Iterable[int], seed: int = 0) -> torch.Tensor:
    shape = tuple(shape)
    g = _gen(name, seed)
    randn = lambda std=1.0, mean=0.0: torch.randn(shape, generator=g) * std + mean
    rand = lambda lo, hi: torch.rand(shape, generator=g) * (hi - lo) + lo
    leaf = name.rsplit(".", 1)[-1]
    if "features." in name:                           # the MobileNetV2 body (mobilenet.py): 'features.N[.conv].K.<leaf>', BN and conv told apart by rank
        if name.endswith("features.0.1.running_var"):
            return rand(0.5, 1.5) * 400.0             # pixel-scale inputs, as stem_1 below
        if len(shape) == 1:
            return rand(0.5, 1.5) if leaf in ("weight", "running_var") else randn(0.1)
        fan_in = shape[1] * shape[2] * shape[3]
        project = ".conv." in name and shape[2] == 1 and int(name.split(".")[-2]) in (3, 6)      # the linear 1x1 that ends a block
        return randn(math.sqrt((1.0 if project else 2.0) / fan_in))                            # a ReLU6 follows every other conv
    if name.endswith("stem.conv1.norm.running_var"):
        return rand(0.5, 1.5) * 400.0                 # the ResNet stem reads pixels too
    if name.endswith("stem_1/norm.running_var"):
        return rand(0.5, 1.5) * 400.0                 # pixel-scale inputs (std ~20) are normalised by the first BN
    if name.endswith("norm.weight") or name.endswith("norm.running_var"):     # '/norm.' and the dw bodies' '/pw_norm.'
        return rand(0.5, 1.5)
    if name.endswith("norm.bias") or name.endswith("norm.running_mean"):
        return randn(0.1)
    if name.endswith("/dw_conv3x3.weight"):
        return randn(1.0 / 3.0)                       # no ReLU between the dw and pw convs: unit gain
    if "/conv_offset." in name:                       # DFConv3x3 offsets (and mask logits): a few pixels, mostly fractional
        return randn(1.5 / math.sqrt(shape[1] * 9)) if leaf == "weight" else randn(0.5)
    if ".scales." in name:
        return rand(SYNTH["scale_lo"], SYNTH["scale_hi"])
    if "ese.fc.weight" in name:
        return randn(1.0 / math.sqrt(shape[1]))
    if "ese.fc.bias" in name:
        return randn(1.0)
    if "cls_logits" in name:
        if leaf == "weight":                          # zero-mean per class: the post-ReLU tower output has a
            w = randn(SYNTH["cls_logits_std"])        # positive mean that would otherwise favour one class
            return w - w.mean(dim=(1, 2, 3), keepdim=True)
        return randn(0.02, SYNTH["cls_logits_bias"])
    if "bbox_pred" in name:
        return randn(SYNTH["bbox_pred_std"]) if leaf == "weight" else randn(0.2, SYNTH["bbox_pred_bias"])
    if "ctrness" in name:
        return randn(SYNTH["ctrness_std"]) if leaf == "weight" else randn(0.1)
    if "mask_head.predictor" in name:
        return randn(SYNTH["predictor_std"]) if leaf == "weight" else randn(0.1)
    if name.endswith("maskiou.weight"):
        return randn(SYNTH["maskiou_std"])
    if name.endswith("maskiou.bias"):
        return randn(0.05, 0.5)
    if "score_lowres" in name:                        # ConvTranspose2d k4 s2: every output pixel sums Cin * 4 taps -> logits of order 1
        return randn(3.0 * math.sqrt(1.0 / (4 * shape[0]))) if leaf == "weight" else randn(0.1)
    if "_tower." in name and len(shape) == 1 and int(name.split(".")[-2]) % 3 == 1:   # GroupNorm affine
        return rand(0.5, 1.5) if leaf == "weight" else randn(0.1)
    if "fpn_lateral" in name and len(shape) == 4:
        return randn(0.35 * math.sqrt(1.0 / shape[1]))  # no ReLU follows: keep p-levels O(1)
    if ("fpn_output" in name or "top_block" in name) and len(shape) == 4:
        return randn(math.sqrt(1.0 / (shape[1] * 9)))
    if len(shape) == 4:
        fan_in = shape[1] * shape[2] * shape[3]
        if "deconv" in name:
            fan_in = shape[0]
        return randn(math.sqrt(2.0 / fan_in))       # Kaiming-normal(fan_in): activations neither vanish nor explode
    if len(shape) == 2:
        return randn(math.sqrt(2.0 / shape[1]))
    return randn(0.1)                                 # remaining biases


def make_synthetic_state_dict(conv_body: str = "V-39-eSE", seed: int = 0, shapes=None, **dcn) -> Dict[str, torch.Tensor]:
    """Deep bodies (stages of >= 3 OSA blocks: V-57, V-99) get the FrozenBN affine of every identity block's 1x1 aggregation scaled by
    1/sqrt(blocks in the stage).  dcn: the DCN and keypoint keywords of model_param_shapes (default off).  Each identity block computes x + eSE(concat(x)); with unit-gain random branches the activations grow
    geometrically over 9 blocks (V-99: |p3| up to 450) and the fp32 arithmetic of the REFERENCE itself then sits 1.6e-4 (features),
    2e-3 (logits) and 0.9 px (boxes) away from a float64 evaluation (tools/diag_v99.py) — no fp32 implementation could be compared
    with it at 1e-3.  A trained network keeps its residual branches small; so does this scaling (|p3| <= 33, fp32 vs fp64 7e-7)."""
    import re
    shapes = shapes if shapes is not None else model_param_shapes(conv_body, **dcn)
    sd = OrderedDict((k, synthetic_tensor(k, v, seed).float().contiguous()) for k, v in shapes.items())
    if conv_body == MOBILENETV2:
        return sd
    if resnet_body(conv_body) is not None:
        # relu(conv3(..) + shortcut(x) or x): conv3 and the shortcut are Kaiming-normal (gain 2) with no ReLU of their own behind them,
        # so each branch doubles the second moment, and the sum adds the branches up; unscaled, the activations double in every one
        # of the 16-50 blocks.  The FrozenBN affine that ends a branch is scaled by 1/sqrt(2) for the gain and by 1/sqrt(branches): the
        # two branches of a stage's first block by 1/2, the identity blocks of a stage (which share one unit of growth, the 1/sqrt(blocks)
        # rule of the VoVNet bodies below) by 1/sqrt(2 * blocks in the stage).
        per_stage = RESNET_BLOCKS[resnet_body(conv_body)[0]]
        for k in sd:
            m = re.search(r"\.res(\d)\.(\d+)\.(conv3|shortcut)\.norm\.(weight|bias)$", k)
            if m:
                sd[k] = (sd[k] * (4 if m.group(2) == "0" else 2 * per_stage[int(m.group(1)) - 2]) ** -0.5).contiguous()
        return sd
    blocks = STAGE_SPECS[conv_body]["block_per_stage"]
    for k in sd:
        m = re.search(r"stage(\d)\.OSA\d_(\d+)\.concat\..*norm\.(weight|bias)$", k)
        if m and int(m.group(2)) >= 2 and blocks[int(m.group(1)) - 2] >= 3:
            sd[k] = (sd[k] * blocks[int(m.group(1)) - 2] ** -0.5).contiguous()
    return sd


def make_synthetic_images(batch: int, height: int = 800, width: int = 1280, seed0: int = 1234,
                          first: int = 0) -> torch.Tensor:
    """(batch,3,H,W) float32: uint8-valued BGR noise minus PIXEL_MEAN (deploy_utils.py:81-83).
    Image i of the global job uses seed seed0+i; `first` is the global index of this batch's first image.
    Smooth blobs are blended in so the image is not pure white noise (keeps activations image-dependent)."""
    imgs = []
    mean = torch.tensor(PIXEL_MEAN).view(3, 1, 1)
    for i in range(batch):
        g = torch.Generator()
        g.manual_seed(seed0 + first + i)
        coarse = torch.randint(0, 256, (1, 3, max(height // 32, 1), max(width // 32, 1)), generator=g).float()
        low = torch.nn.functional.interpolate(coarse, size=(height, width), mode="bilinear", align_corners=False)[0]
        noise = torch.randint(0, 256, (3, height, width), generator=g).float()
        img = torch.floor(0.75 * low + 0.25 * noise).clamp_(0, 255)
        imgs.append(img - mean)
    return torch.stack(imgs).contiguous()
