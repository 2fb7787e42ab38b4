"""not gpu: the ResNet backbones' host side — builders and their state-dict keys against the listing of tests/golden/make_golden_resnet.py,
config, the two R-* yamls, the refusals, synthetic weights, and the C ABI boundary of the fused stem kernel."""
import ctypes
import hashlib
import os
import re

import pytest
import torch

from .helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ["res2", "res3", "res4", "res5"]
# sha256 over (key, shape, bytes) of make_synthetic_state_dict("V-39-eSE", 0), computed on the commit before the ResNet entries were added
V39_SEED0_SHA256 = "9d38646dec978dcaacb1024f0af94a939e01f2cf0a4d9a279acf8b1e7962ffc2"


def reference_keys():
    """{'<builder>[ depth 101]': its state-dict keys in order} from state_dict_keys_R50.txt."""
    out, cur = {}, None
    for line in open(os.path.join(GOLDEN, "state_dict_keys_R50.txt")).read().split("\n"):
        if line.startswith("# "):
            cur = out.setdefault(line[2:].strip(), [])
        elif line:
            cur.append(line)
    return out


def r_cfg(*pairs, depth=50):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_R_{}_FPN_ms_3x.yaml".format(depth)))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(pairs))
    return cfg


def build(name, *pairs, depth=50):
    import centermask2_amd.modeling  # noqa: F401  registers the plugins
    from centermask2_amd.registry import BACKBONE_REGISTRY
    from centermask2_amd.structures import ShapeSpec
    return BACKBONE_REGISTRY.get(name)(r_cfg(*pairs, depth=depth), ShapeSpec(channels=3))


def test_builders_register_with_the_reference_keys_and_shapes():
    from centermask2_amd.config import get_cfg
    from centermask2_amd.registry import BACKBONE_REGISTRY
    import centermask2_amd.modeling  # noqa: F401
    ref = reference_keys()
    assert list(ref) == ["build_resnet_backbone", "build_resnet_backbone depth 101", "build_fcos_resnet_fpn_backbone", "build_resnet_fpn_backbone"]
    assert get_cfg().MODEL.BACKBONE.NAME in BACKBONE_REGISTRY             # the default builder name now resolves
    body = build("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL)
    assert list(body.state_dict().keys()) == ref["build_resnet_backbone"]
    assert not any("num_batches_tracked" in k or k.endswith("conv1.bias") for k in body.state_dict())
    shp = body.output_shape()
    assert list(shp) == ALL and [shp[k].channels for k in ALL] == [256, 512, 1024, 2048] and [shp[k].stride for k in ALL] == [4, 8, 16, 32]
    body101 = build("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, depth=101)
    assert list(body101.state_dict().keys()) == ref["build_resnet_backbone depth 101"]
    assert [len(getattr(body101, s)) for s in ALL] == [3, 4, 23, 3]
    body152 = build("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ["stem", "res3"], "MODEL.RESNETS.DEPTH", 152)
    assert [len(getattr(body152, s)) for s in ALL[:2]] == [3, 8] and not hasattr(body152, "res4")     # no stage past the last one asked for
    shp = body152.output_shape()
    assert list(shp) == ["stem", "res3"] and shp["stem"].channels == 64 and shp["stem"].stride == 4 and shp["res3"].stride == 8
    fcos_bb = build("build_fcos_resnet_fpn_backbone")
    assert list(fcos_bb.state_dict().keys()) == ref["build_fcos_resnet_fpn_backbone"]
    shp = fcos_bb.output_shape()
    assert list(shp) == ["p3", "p4", "p5", "p6", "p7"] and all(s.channels == 256 for s in shp.values()) and fcos_bb.size_divisibility == 32
    assert [shp[k].stride for k in shp] == [8, 16, 32, 64, 128]
    for top, levels in ((1, ["p3", "p4", "p5", "p6"]), (0, ["p3", "p4", "p5"])):
        bb = build("build_fcos_resnet_fpn_backbone", "MODEL.FCOS.TOP_LEVELS", top)
        assert list(bb.output_shape()) == levels and bb.size_divisibility == 32
    mp = build("build_resnet_fpn_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.FPN.IN_FEATURES", ALL)
    assert list(mp.state_dict().keys()) == ref["build_resnet_fpn_backbone"]
    shp = mp.output_shape()
    assert list(shp) == ["p2", "p3", "p4", "p5", "p6"] and [shp[k].stride for k in shp] == [4, 8, 16, 32, 64] and mp.size_divisibility == 32


def test_block_layout_follows_the_config():
    body = build("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL)
    assert [b.stride for b in body.res2] == [1, 1, 1] and [b.stride for b in body.res3] == [2, 1, 1, 1]
    b = body.res3[0]
    assert b.conv1.stride == (2, 2) and b.conv2.stride == (1, 1) and b.shortcut.stride == (2, 2) and body.res3[1].shortcut is None
    assert tuple(b.conv1.weight.shape) == (128, 256, 1, 1) and tuple(b.conv3.weight.shape) == (512, 128, 1, 1)
    assert tuple(body.stem.conv1.weight.shape) == (64, 3, 7, 7) and body.stem.conv1.norm.eps == 1e-5
    b = build("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.RESNETS.STRIDE_IN_1X1", False).res4[0]
    assert b.conv1.stride == (1, 1) and b.conv2.stride == (2, 2) and b.shortcut.stride == (2, 2)
    wide = build("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.RESNETS.WIDTH_PER_GROUP", 32, "MODEL.RESNETS.RES2_OUT_CHANNELS", 128)
    assert tuple(wide.res5[0].conv2.weight.shape) == (256, 256, 3, 3) and wide.output_shape()["res5"].channels == 1024
    # FREEZE_AT (default 2: stem and res2) only clears requires_grad
    assert not body.stem.conv1.weight.requires_grad and not body.res2[2].conv3.weight.requires_grad and body.res3[0].conv1.weight.requires_grad
    thawed = build("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.BACKBONE.FREEZE_AT", 0)
    assert thawed.stem.conv1.weight.requires_grad


@pytest.mark.parametrize("pairs, key", [
    (("MODEL.RESNETS.DEPTH", 18), "DEPTH"), (("MODEL.RESNETS.DEPTH", 34), "DEPTH"), (("MODEL.RESNETS.NUM_GROUPS", 32), "NUM_GROUPS"),
    (("MODEL.RESNETS.RES5_DILATION", 2), "RES5_DILATION"), (("MODEL.RESNETS.DEFORM_ON_PER_STAGE", [False, True, True, True]), "DEFORM_ON_PER_STAGE"),
    (("MODEL.RESNETS.NORM", "GN"), "NORM"), (("MODEL.RESNETS.STEM_OUT_CHANNELS", 32), "STEM_OUT_CHANNELS"),
    (("MODEL.RESNETS.WIDTH_PER_GROUP", 24), "WIDTH_PER_GROUP"), (("MODEL.RESNETS.RES2_OUT_CHANNELS", 72), "RES2_OUT_CHANNELS"),
    (("MODEL.RESNETS.OUT_FEATURES", ["res6"]), "OUT_FEATURES")])
def test_unbuilt_options_are_refused_with_their_key(pairs, key):
    with pytest.raises(NotImplementedError, match="MODEL.RESNETS." + key):
        build("build_resnet_backbone", *pairs)


def test_config_defaults_and_the_two_yamls():
    from centermask2_amd.config import get_cfg
    r = get_cfg().MODEL.RESNETS
    assert (r.DEPTH, r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1, r.RES5_DILATION, r.RES2_OUT_CHANNELS, r.STEM_OUT_CHANNELS, r.NORM) == \
        (50, 1, 64, True, 1, 256, 64, "FrozenBN")
    assert list(r.DEFORM_ON_PER_STAGE) == [False] * 4 and r.DEFORM_MODULATED is False and r.DEFORM_NUM_GROUPS == 1 and r.OUT_FEATURES == ["res4"]
    from centermask2_amd.modeling import build_model
    for depth in (50, 101):
        m = r_cfg(depth=depth).MODEL
        assert m.BACKBONE.NAME == "build_fcos_resnet_fpn_backbone" and m.RESNETS.DEPTH == depth and m.MASK_ON is True and m.MASKIOU_ON is True
        assert m.RESNETS.OUT_FEATURES == ["res3", "res4", "res5"] and m.FPN.IN_FEATURES == ["res3", "res4", "res5"]
        text = open(os.path.join(ROOT, "centermask2_amd", "configs", "centermask", "centermask_R_{}_FPN_ms_3x.yaml".format(depth))).read()
        assert "RECALLED" in text.split("MODEL:")[0]            # the recipe is not in the reference tree, and the file says so
        model = build_model(r_cfg(depth=depth)).eval()
        assert list(model.backbone.output_shape()) == ["p3", "p4", "p5", "p6", "p7"]
        assert len(model.backbone.bottom_up.res4) == {50: 6, 101: 23}[depth]


def test_synthetic_weights_load_strict_and_stay_level():
    from centermask2_amd import synthetic as S
    from centermask2_amd._lib import CmkError
    from centermask2_amd.modeling import build_model
    model = build_model(r_cfg()).eval()
    shapes = S.model_param_shapes("R-50")
    sd = S.make_synthetic_state_dict("R-50", 0)
    assert set(sd) == set(shapes) == set(model.state_dict())
    assert all(tuple(model.state_dict()[k].shape) == tuple(shapes[k]) for k in shapes)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(S.resnet_param_shapes(50)) == reference_keys()["build_resnet_backbone"]
    assert list(S.resnet_param_shapes(101)) == reference_keys()["build_resnet_backbone depth 101"]
    bu = "backbone.bottom_up."
    assert float(sd[bu + "stem.conv1.norm.running_var"].min()) >= 200.0 and float(sd[bu + "res2.0.conv1.norm.running_var"].max()) <= 1.5
    # the branch ends: 1/2 in a stage's first block, 1/sqrt(2 * blocks) in its identity blocks; every other FrozenBN weight in [0.5, 1.5]
    assert float(sd[bu + "res4.0.conv3.norm.weight"].max()) <= 0.75 and float(sd[bu + "res4.0.shortcut.norm.weight"].min()) >= 0.25
    assert float(sd[bu + "res4.3.conv3.norm.weight"].max()) <= 1.5 / 12 ** 0.5 + 1e-6 and float(sd[bu + "res4.3.conv2.norm.weight"].min()) >= 0.5
    sd101 = S.make_synthetic_state_dict("R-101", 0)
    assert float(sd101[bu + "res4.22.conv3.norm.weight"].max()) <= 1.5 / 46 ** 0.5 + 1e-6
    assert torch.equal(sd101[bu + "res2.1.conv2.weight"], sd[bu + "res2.1.conv2.weight"])            # a tensor depends on its key and seed only
    with pytest.raises(CmkError):                                                                   # no CPU fallback
        model.backbone(torch.zeros(1, 3, 64, 64))


def test_v39_synthetic_state_dict_is_unchanged():
    from centermask2_amd import synthetic as S
    m = hashlib.sha256()
    for k, v in S.make_synthetic_state_dict("V-39-eSE", 0).items():
        m.update(k.encode())
        m.update(str(tuple(v.shape)).encode())
        m.update(v.numpy().tobytes())
    assert m.hexdigest() == V39_SEED0_SHA256


def test_mobilenet_flag_routes_the_fcos_builder_to_mobilenetv2():
    from centermask2_amd.modeling.backbone.mobilenet import MobileNetV2
    bb = build("build_fcos_resnet_fpn_backbone", "MODEL.MOBILENET", True)
    assert isinstance(bb.bottom_up, MobileNetV2) and list(bb.output_shape()) == ["p3", "p4", "p5", "p6", "p7"]
    assert tuple(bb.fpn_lateral5.weight.shape) == (256, 320, 1, 1)


def test_pack_stem7_weight_orders_taps_kh_kw_ci():
    from centermask2_amd import ops
    w = torch.arange(64 * 3 * 7 * 7, dtype=torch.float32).reshape(64, 3, 7, 7)
    p = ops.pack_stem7_weight(w)
    assert tuple(p.shape) == (147, 64) and p.is_contiguous()
    for co, ci, kh, kw in ((0, 0, 0, 0), (5, 2, 6, 6), (63, 1, 3, 4), (17, 0, 6, 0)):
        assert float(p[(kh * 7 + kw) * 3 + ci, co]) == float(w[co, ci, kh, kw])
    with pytest.raises(AssertionError):
        ops.pack_stem7_weight(torch.zeros(64, 3, 3, 3))


def test_fused_stem_entry_is_declared_and_refuses_bad_arguments_without_gpu():
    from centermask2_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "cmk.h")).read()
    assert re.search(r"\bint\s+cmk_stem7x7_bn_relu_maxpool_nchw3\s*\(", header)
    assert "cmk_stem7x7_bn_relu_maxpool_nchw3" in _lib.SIGNATURES and hasattr(ops, "stem7x7_bn_relu_maxpool") and hasattr(ops, "pack_stem7_weight")
    lib = _lib.load()
    assert lib.cmk_version() == 5
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(x=p, w=p, scale=p, shift=p, y=p, y_cs=64, y_co=0, n=1, h=2, wd=2, cout=64):
        rc = lib.cmk_stem7x7_bn_relu_maxpool_nchw3(x, w, scale, shift, y, y_cs, y_co, n, h, wd, cout, None)
        return rc, lib.cmk_last_error()

    for kw in (dict(x=None), dict(w=None), dict(scale=None), dict(shift=None), dict(y=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"null pointer" in msg, (kw, msg)
    for cout in (32, 128, 0):
        rc, msg = call(cout=cout)
        assert rc == -1 and b"must be 64" in msg and "Cout = {}".format(cout).encode() in msg, msg
    for kw in (dict(n=0), dict(h=0), dict(wd=0), dict(h=-3)):
        rc, msg = call(**kw)
        assert rc == -1 and b"empty" in msg, (kw, msg)
    for kw in (dict(y_co=2, y_cs=72), dict(y_cs=66), dict(y_co=-4, y_cs=72), dict(y_co=16, y_cs=64)):
        rc, msg = call(**kw)
        assert rc == -1 and b"output view" in msg, (kw, msg)
    rc, msg = call(y=p + 4)
    assert rc == -1 and b"aligned" in msg, msg
    rc, msg = call(h=30000, wd=30000)
    assert rc == -1 and b"too large" in msg, msg
