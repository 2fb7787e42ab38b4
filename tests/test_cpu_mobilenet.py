"""not gpu: the MobileNetV2 backbone's host side — builders and their state-dict keys against the reference's listing
(tests/golden/make_golden_mnv2.py), config, the Lite yaml, synthetic weights, and the C ABI boundary of the fused depth-wise kernel."""
import ctypes
import os
import re

import pytest
import torch

from .helpers import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITE = dict(fpn_ch=128, mask_dim=128, num_tower_convs=2, mask_num_conv=2, maskiou_num_conv=2)
ALL = ["res2", "res3", "res4", "res5"]


def reference_keys():
    """{builder name: its state-dict keys in the reference's order} from state_dict_keys_Mv2.txt."""
    out, cur = {}, None
    for line in open(os.path.join(GOLDEN, "state_dict_keys_Mv2.txt")).read().split("\n"):
        if line.startswith("# "):
            cur = out.setdefault(line[2:].strip(), [])
        elif line:
            cur.append(line)
    return out


def lite_cfg(*pairs):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_lite_Mv2_FPN_ms_4x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(pairs))
    return cfg


def test_builders_register_with_the_reference_keys_and_shapes():
    import centermask2_amd.modeling  # noqa: F401  registers the plugins
    from centermask2_amd.registry import BACKBONE_REGISTRY
    from centermask2_amd.structures import ShapeSpec
    ref = reference_keys()
    assert list(ref) == ["build_mnv2_backbone", "build_fcos_mobilenetv2_fpn_backbone", "build_mobilenetv2_fpn_backbone"]
    for name in ref:
        assert name in BACKBONE_REGISTRY
    body = BACKBONE_REGISTRY.get("build_mnv2_backbone")(lite_cfg("MODEL.RESNETS.OUT_FEATURES", ALL), ShapeSpec(channels=3))
    assert list(body.state_dict().keys()) == ref["build_mnv2_backbone"]
    shp = body.output_shape()
    assert list(shp) == ALL and [shp[k].channels for k in ALL] == [24, 32, 96, 320] and [shp[k].stride for k in ALL] == [4, 8, 16, 32]
    fcos_bb = BACKBONE_REGISTRY.get("build_fcos_mobilenetv2_fpn_backbone")(lite_cfg(), ShapeSpec(channels=3))
    assert list(fcos_bb.state_dict().keys()) == ref["build_fcos_mobilenetv2_fpn_backbone"]
    shp = fcos_bb.output_shape()
    assert list(shp) == ["p3", "p4", "p5", "p6", "p7"] and all(s.channels == 128 for s in shp.values()) and fcos_bb.size_divisibility == 32
    for top, levels in ((1, ["p3", "p4", "p5", "p6"]), (0, ["p3", "p4", "p5"])):
        bb = BACKBONE_REGISTRY.get("build_fcos_mobilenetv2_fpn_backbone")(lite_cfg("MODEL.FCOS.TOP_LEVELS", top), ShapeSpec(channels=3))
        assert list(bb.output_shape()) == levels and bb.size_divisibility == 32
    mp = BACKBONE_REGISTRY.get("build_mobilenetv2_fpn_backbone")(lite_cfg("MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.FPN.IN_FEATURES", ALL),
                                                                 ShapeSpec(channels=3))
    assert list(mp.state_dict().keys()) == ref["build_mobilenetv2_fpn_backbone"]
    shp = mp.output_shape()
    assert list(shp) == ["p2", "p3", "p4", "p5", "p6"] and [shp[k].stride for k in shp] == [4, 8, 16, 32, 64] and mp.size_divisibility == 32
    with pytest.raises(ValueError):
        BACKBONE_REGISTRY.get("build_mnv2_backbone")(lite_cfg("MODEL.RESNETS.OUT_FEATURES", ["res6"]), ShapeSpec(channels=3))


def test_config_has_resnets_and_the_lite_yaml_merges():
    from centermask2_amd.config import get_cfg
    assert get_cfg().MODEL.RESNETS.OUT_FEATURES == ["res4"]
    m = lite_cfg().MODEL
    assert m.BACKBONE.NAME == "build_fcos_mobilenetv2_fpn_backbone" and m.BACKBONE.FREEZE_AT == 0 and m.MOBILENET is True
    assert m.RESNETS.OUT_FEATURES == ["res3", "res4", "res5"] and m.FPN.IN_FEATURES == ["res3", "res4", "res5"] and m.FPN.OUT_CHANNELS == 128
    assert m.FCOS.NUM_CLS_CONVS == 2 and m.FCOS.NUM_BOX_CONVS == 2 and m.FCOS.POST_NMS_TOPK_TEST == 50
    assert m.ROI_MASK_HEAD.CONV_DIM == 128 and m.ROI_MASK_HEAD.NUM_CONV == 2
    assert m.ROI_MASKIOU_HEAD.CONV_DIM == 128 and m.ROI_MASKIOU_HEAD.NUM_CONV == 2
    cfg = lite_cfg()
    assert cfg.INPUT.MIN_SIZE_TEST == 600 and cfg.INPUT.MAX_SIZE_TEST == 1000
    text = open(os.path.join(ROOT, "centermask2_amd", "configs", "centermask", "centermask_lite_Mv2_FPN_ms_4x.yaml")).read()
    assert "RECALLED" in text.split("MODEL:")[0]            # the recipe is not in the reference tree, and the file says so


def test_lite_model_builds_on_cpu_and_loads_the_synthetic_weights():
    from centermask2_amd import synthetic as S
    from centermask2_amd._lib import CmkError
    from centermask2_amd.modeling import build_model
    model = build_model(lite_cfg()).eval()
    shapes = S.model_param_shapes(S.MOBILENETV2, **LITE)
    sd = S.make_synthetic_state_dict(S.MOBILENETV2, 0, **LITE)
    assert set(sd) == set(shapes) == set(model.state_dict())
    assert all(tuple(model.state_dict()[k].shape) == tuple(shapes[k]) for k in shapes)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    body = S.mobilenetv2_param_shapes()
    assert list(body) == reference_keys()["build_mnv2_backbone"]
    # the naming rules: a ReLU6 follows the stem, expand and depth-wise convs (gain 2), the project conv is linear (gain 1)
    bu = "backbone.bottom_up.features."
    assert float(sd[bu + "0.1.running_var"].min()) >= 200.0 and float(sd[bu + "5.conv.4.running_var"].max()) <= 1.5
    w_exp, w_dw, w_proj = sd[bu + "5.conv.0.weight"], sd[bu + "5.conv.3.weight"], sd[bu + "5.conv.6.weight"]
    assert tuple(w_exp.shape) == (192, 32, 1, 1) and tuple(w_dw.shape) == (192, 1, 3, 3) and tuple(w_proj.shape) == (32, 192, 1, 1)
    assert float(w_exp.var()) == pytest.approx(2.0 / 32, rel=0.1) and float(w_proj.var()) == pytest.approx(1.0 / 192, rel=0.1)
    assert float(w_dw.var()) == pytest.approx(2.0 / 9, rel=0.15)
    assert float(sd[bu + "1.conv.3.weight"].var()) == pytest.approx(1.0 / 32, rel=0.2)            # the t = 1 block's project conv
    with pytest.raises(CmkError):                                                                   # no CPU fallback
        model.backbone(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError):
        from centermask2_amd.modeling.backbone.mobilenet import MobileNetV2
        MobileNetV2(lite_cfg(), width_mult=0.5)


def test_fused_depthwise_entry_is_declared_and_refuses_bad_arguments_without_gpu():
    from centermask2_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "cmk.h")).read()
    assert re.search(r"\bint\s+cmk_dwconv3x3_bn_act_nhwc\s*\(", header)
    assert "cmk_dwconv3x3_bn_act_nhwc" in _lib.SIGNATURES and hasattr(ops, "dwconv3x3_bn_act")
    lib = _lib.load()
    assert lib.cmk_version() == 5
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    inf = float("inf")

    def call(x=p, w=p, scale=p, shift=p, y=p, x_cs=16, x_co=0, y_cs=16, y_co=0, n=1, h=2, wd=2, c=16, stride=1):
        rc = lib.cmk_dwconv3x3_bn_act_nhwc(x, x_cs, x_co, w, scale, shift, 6.0, 0.0, 6.0, y, y_cs, y_co, n, h, wd, c, stride, None)
        return rc, lib.cmk_last_error()

    for kw in (dict(x=None), dict(w=None), dict(scale=None), dict(shift=None), dict(y=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"null pointer" in msg, (kw, msg)
    rc, msg = call(c=6, x_cs=8, y_cs=8)
    assert rc == -1 and b"multiple of 4" in msg and b"C = 6" in msg, msg
    for kw in (dict(x_co=2), dict(y_co=6), dict(x_cs=18)):
        rc, msg = call(**kw)
        assert rc == -1 and b"misaligned" in msg, (kw, msg)
    rc, msg = call(x_co=4)                                  # [4, 20) of a 16-float pixel
    assert rc == -1 and b"leaves the pixel" in msg, msg
    rc, msg = call(stride=3)
    assert rc == -1 and b"stride 3" in msg, msg
    for kw in (dict(n=0), dict(h=0), dict(wd=0), dict(c=0)):
        rc, msg = call(**kw)
        assert rc == -1 and b"empty" in msg, (kw, msg)
    rc, msg = call(x=p + 4)
    assert rc == -1 and b"16-byte aligned" in msg, msg
    rc = lib.cmk_dwconv3x3_bn_act_nhwc(p, 16, 0, p, p, p, inf, 6.0, 0.0, p, 16, 0, 1, 2, 2, 16, 1, None)
    assert rc == -1 and b"clamp bounds" in lib.cmk_last_error()


def test_recorded_clamp_shares_exercise_both_clamps():
    """Every ReLU6 site of the reference body, on both fixture inputs: the upper clamp fires on 0.1 % .. 50 % of the values entering it,
    so the backbone fixtures tell min(., 6) from a plain ReLU at every fused launch."""
    g = golden("mnv2_backbone")
    for key in ("clamp_shares", "clamp_shares_odd"):
        shares = g[key]
        assert tuple(shares.shape) == (34, 2)
        assert float(shares[:, 0].min()) >= 0.001 and float(shares[:, 0].max()) <= 0.5, shares[:, 0]
        assert float(shares[:, 1].min()) > 0.0
