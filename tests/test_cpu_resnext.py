"""not gpu: the ResNeXt backbones' host side — module tree and state-dict keys against the listing of tests/golden/make_golden_resnext.py,
synthetic weights, construction refusals and acceptances, the X-101-32x8d yaml, the grouped conv's weight packing and the C ABI boundary
of cmk_group_conv3x3_nhwc."""
import ctypes
import os
import re

import pytest
import torch

from .helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ["res2", "res3", "res4", "res5"]
YAML = "centermask_X_101_32x8d_FPN_ms_3x.yaml"


def reference_keys():
    out, cur = {}, None
    for line in open(os.path.join(GOLDEN, "state_dict_keys_X.txt")).read().split("\n"):
        if line.startswith("# "):
            cur = out.setdefault(line[2:].strip(), [])
        elif line:
            cur.append(line)
    return out


def x_cfg(*pairs):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path(YAML))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(pairs))
    return cfg


def build(name, *pairs):
    import centermask2_amd.modeling  # noqa: F401  registers the plugins
    from centermask2_amd.registry import BACKBONE_REGISTRY
    from centermask2_amd.structures import ShapeSpec
    return BACKBONE_REGISTRY.get(name)(x_cfg(*pairs), ShapeSpec(channels=3))


def body(depth, groups, wpg, *pairs):
    return build("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.RESNETS.DEPTH", depth, "MODEL.RESNETS.NUM_GROUPS", groups,
                 "MODEL.RESNETS.WIDTH_PER_GROUP", wpg, *pairs)


def test_module_tree_and_keys_equal_the_reference_listing():
    ref = reference_keys()
    assert list(ref) == ["build_resnet_backbone X-50-32x4d", "build_resnet_backbone X-101-32x8d", "build_fcos_resnet_fpn_backbone X-101-32x8d"]
    x50 = body(50, 32, 4)
    assert list(x50.state_dict().keys()) == ref["build_resnet_backbone X-50-32x4d"]
    assert tuple(x50.res2[0].conv2.weight.shape) == (128, 4, 3, 3) and x50.res2[0].conv2.groups == 32
    assert tuple(x50.res5[2].conv2.weight.shape) == (1024, 32, 3, 3)
    x101 = body(101, 32, 8)
    assert list(x101.state_dict().keys()) == ref["build_resnet_backbone X-101-32x8d"]
    assert tuple(x101.res3[0].conv2.weight.shape) == (512, 16, 3, 3) and tuple(x101.res5[0].conv2.weight.shape) == (2048, 64, 3, 3)
    assert tuple(x101.res3[0].conv1.weight.shape) == (512, 256, 1, 1) and tuple(x101.res3[0].conv3.weight.shape) == (512, 512, 1, 1)
    b = x101.res3[0]                                                     # STRIDE_IN_1X1 False: the stride sits on the grouped conv
    assert b.conv1.stride == (1, 1) and b.conv2.stride == (2, 2) and b.num_groups == 32
    shp = x101.output_shape()
    assert [shp[k].channels for k in ALL] == [256, 512, 1024, 2048] and [shp[k].stride for k in ALL] == [4, 8, 16, 32]
    fcos_bb = build("build_fcos_resnet_fpn_backbone")
    assert list(fcos_bb.state_dict().keys()) == ref["build_fcos_resnet_fpn_backbone X-101-32x8d"]


def test_synthetic_weights_load_strictly_and_leave_r50_unchanged():
    from centermask2_amd import synthetic as S
    assert S.RESNEXT_BODIES == {"X-50-32x4d": (50, 32, 4), "X-101-32x4d": (101, 32, 4), "X-101-64x4d": (101, 64, 4), "X-101-32x8d": (101, 32, 8)}
    for name, (depth, groups, wpg) in (("X-50-32x4d", (50, 32, 4)), ("X-101-32x8d", (101, 32, 8))):
        sd = S.make_synthetic_state_dict(name, 0)
        bb = build("build_fcos_resnet_fpn_backbone", "MODEL.RESNETS.DEPTH", depth, "MODEL.RESNETS.NUM_GROUPS", groups, "MODEL.RESNETS.WIDTH_PER_GROUP", wpg)
        res = bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert tuple(sd["backbone.bottom_up.res2.0.conv2.weight"].shape) == (groups * wpg, wpg, 3, 3)
    # Kaiming on the grouped fan-in 9 * Cg: the activations stay level through a grouped body
    w = S.make_synthetic_state_dict("X-101-32x8d", 0)["backbone.bottom_up.res4.5.conv2.weight"]
    assert tuple(w.shape) == (1024, 32, 3, 3) and abs(float(w.std()) - (2.0 / (9 * 32)) ** 0.5) < 0.02 * (2.0 / (9 * 32)) ** 0.5
    # the new `groups` argument changes nothing at its default: shapes and tensors of R-50 are what they were
    assert S.resnet_param_shapes(50, "p.") == S.resnet_param_shapes(50, "p.", groups=1)
    assert S.resnet_param_shapes(50, "p.")["p.res3.0.conv2.weight"] == (128, 128, 3, 3)
    key = "backbone.bottom_up.res3.0.conv2.weight"
    assert torch.equal(S.make_synthetic_state_dict("R-50", 0)[key], S.synthetic_tensor(key, (128, 128, 3, 3), 0))
    key = "backbone.bottom_up.res3.0.conv3.norm.weight"                   # first block of a stage: scaled by 1/2
    assert torch.equal(S.make_synthetic_state_dict("R-50", 0)[key], (S.synthetic_tensor(key, (512,), 0) * 4 ** -0.5).contiguous())


@pytest.mark.parametrize("pairs, named", [
    (("MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 16, "MODEL.RESNETS.OUT_FEATURES", ALL), ("WIDTH_PER_GROUP", "res5", "128")),
    (("MODEL.RESNETS.NUM_GROUPS", 3, "MODEL.RESNETS.WIDTH_PER_GROUP", 64), ("WIDTH_PER_GROUP",)),
    (("MODEL.RESNETS.NUM_GROUPS", 3, "MODEL.RESNETS.WIDTH_PER_GROUP", 8), ("WIDTH_PER_GROUP",))])
def test_out_of_range_grouped_configs_are_refused_with_their_key(pairs, named):
    with pytest.raises(NotImplementedError, match=r"^MODEL\.RESNETS\.NUM_GROUPS") as e:
        build("build_resnet_backbone", *pairs)
    assert all(n in str(e.value) for n in named), str(e.value)


def test_other_refusals_keep_their_place():
    for pairs, key in ((("MODEL.RESNETS.DEPTH", 18), "DEPTH"), (("MODEL.RESNETS.DEPTH", 34), "DEPTH"), (("MODEL.RESNETS.RES5_DILATION", 2), "RES5_DILATION"),
                       (("MODEL.RESNETS.DEFORM_ON_PER_STAGE", [False, True, True, True]), "DEFORM_ON_PER_STAGE"), (("MODEL.RESNETS.NORM", "GN"), "NORM"),
                       (("MODEL.RESNETS.STEM_OUT_CHANNELS", 32), "STEM_OUT_CHANNELS")):
        with pytest.raises(NotImplementedError, match=r"^MODEL\.RESNETS\." + key):
            build("build_resnet_backbone", *pairs)                     # on top of the grouped yaml: the earlier refusals still come first


def test_in_range_grouped_configs_build():
    b = build("build_resnet_backbone", "MODEL.RESNETS.NUM_GROUPS", 64, "MODEL.RESNETS.WIDTH_PER_GROUP", 4, "MODEL.RESNETS.OUT_FEATURES", ALL)
    assert tuple(b.res2[0].conv2.weight.shape) == (256, 4, 3, 3) and tuple(b.res5[0].conv2.weight.shape) == (2048, 32, 3, 3)
    b = build("build_resnet_backbone", "MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 16, "MODEL.RESNETS.OUT_FEATURES", ["res3", "res4"])
    assert not hasattr(b, "res5") and tuple(b.res4[0].conv2.weight.shape) == (2048, 64, 3, 3)


def test_shipped_yaml_builds_the_x101_model():
    from centermask2_amd.config import config_path
    from centermask2_amd.modeling import build_model
    text = open(config_path(YAML)).read()
    assert "RECALLED" in text
    cfg = x_cfg()
    r = cfg.MODEL.RESNETS
    assert (r.DEPTH, r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1) == (101, 32, 8, False)
    assert list(cfg.MODEL.PIXEL_STD) == [57.375, 57.120, 58.395]
    model = build_model(cfg)
    assert list(model.backbone.output_shape()) == ["p3", "p4", "p5", "p6", "p7"]
    assert len(model.backbone.bottom_up.res4) == 23 and model.backbone.bottom_up.res4[7].conv2.groups == 32


def test_pack_group_weight_layouts():
    from centermask2_amd import _lib, ops
    assert ops.group_conv_supported(256, 32) and ops.group_conv_supported(2048, 32) and ops.group_conv_supported(128, 32)
    assert not ops.group_conv_supported(4096, 32) and not ops.group_conv_supported(64, 1) and not ops.group_conv_supported(96, 8) and not ops.group_conv_supported(100, 3)
    # Cg = 8: [tap][ci][C]
    c, g, cg = 24, 3, 8
    w = torch.arange(c * cg * 9, dtype=torch.float32).reshape(c, cg, 3, 3)
    p = ops.pack_group_weight(w, g)
    assert p.dim() == 1 and p.numel() == w.numel() and p.is_contiguous()
    for cout, ci, kh, kw in ((0, 0, 0, 0), (5, 3, 1, 2), (23, 7, 2, 2), (9, 0, 2, 0)):
        assert float(p[((kh * 3 + kw) * cg + ci) * c + cout]) == float(w[cout, ci, kh, kw])
    # Cg = 32: [group][chunk][tap][tile][q][n][j] = weight[group*Cg + tile*16 + n][chunk*16 + 4q + j][kh][kw]
    c, g, cg = 64, 2, 32
    w = torch.arange(c * cg * 9, dtype=torch.float32).reshape(c, cg, 3, 3)
    p = ops.pack_group_weight(w, g)
    assert p.numel() == w.numel() and sorted(p.tolist()) == w.reshape(-1).tolist()
    t = cg // 16
    for grp, chunk, tap, tile, q, n, j in ((0, 0, 0, 0, 0, 0, 0), (1, 1, 8, 1, 3, 15, 3), (1, 0, 5, 1, 2, 7, 1), (0, 1, 3, 0, 1, 9, 2)):
        idx = (((((grp * t + chunk) * 9 + tap) * t + tile) * 4 + q) * 16 + n) * 4 + j
        assert float(p[idx]) == float(w[grp * cg + tile * 16 + n, chunk * 16 + 4 * q + j, tap // 3, tap % 3]), (grp, chunk, tap, tile, q, n, j)
    for bad, groups in ((torch.zeros(64, 32, 3, 3), 4), (torch.zeros(64, 32, 1, 1), 2), (torch.zeros(64, 64, 3, 3), 1), (torch.zeros(63, 21, 3, 3), 3)):
        with pytest.raises(_lib.CmkError):
            ops.pack_group_weight(bad, groups)
    with pytest.raises(_lib.CmkError, match="Cg = 128"):
        ops.PackedGroupConv(torch.zeros(256, 128, 3, 3), None, None, "cpu", 2)
    pc = ops.PackedGroupConv(torch.zeros(64, 16, 3, 3), None, None, "cpu", 4, stride=2)
    assert (pc.groups, pc.cg, pc.stride, pc.c) == (4, 16, 2, 64) and pc.w.numel() == 64 * 16 * 9 and tuple(pc.scale.shape) == tuple(pc.shift.shape) == (64,)


def test_group_conv_entry_is_declared_and_refuses_bad_arguments_without_gpu():
    from centermask2_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "cmk.h")).read()
    assert re.search(r"\bint\s+cmk_group_conv3x3_nhwc\s*\(", header)
    assert "cmk_group_conv3x3_nhwc" in _lib.SIGNATURES and all(hasattr(ops, n) for n in ("group_conv3x3", "pack_group_weight", "PackedGroupConv", "group_conv_supported"))
    lib = _lib.load()
    assert lib.cmk_version() == 5
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(x=p, w=p, scale=p, shift=p, y=p, x_cs=64, x_co=0, y_cs=64, y_co=0, n=1, h=2, wd=2, c=64, groups=4, stride=1):
        rc = lib.cmk_group_conv3x3_nhwc(x, x_cs, x_co, w, scale, shift, y, y_cs, y_co, n, h, wd, c, groups, stride, 1, None)
        return rc, lib.cmk_last_error()

    for kw in (dict(x=None), dict(w=None), dict(scale=None), dict(shift=None), dict(y=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"null pointer" in msg, (kw, msg)
    for kw in (dict(n=0), dict(h=0), dict(wd=0), dict(c=0), dict(h=-3)):
        rc, msg = call(**kw)
        assert rc == -1 and b"empty" in msg, (kw, msg)
    for kw in (dict(groups=3), dict(groups=7), dict(groups=1), dict(groups=0)):
        rc, msg = call(**kw)
        assert rc == -1 and b"divisible by groups" in msg, (kw, msg)
    for c, groups, cg in ((64, 32, 2), (256, 2, 128), (48, 4, 12), (64, 64, 1)):
        rc, msg = call(c=c, groups=groups, x_cs=256, y_cs=256)
        assert rc == -1 and "Cg = {}".format(cg).encode() in msg, msg
    for stride in (0, 3, -1):
        rc, msg = call(stride=stride)
        assert rc == -1 and b"must be 1 or 2" in msg, msg
    for kw in (dict(x_co=2, x_cs=72), dict(x_cs=66), dict(y_co=6, y_cs=72), dict(y_cs=70), dict(x_co=-4, x_cs=72), dict(y_co=-4, y_cs=72)):
        rc, msg = call(**kw)
        assert rc == -1 and b"misaligned" in msg, (kw, msg)
    for kw in (dict(x_co=16, x_cs=64), dict(y_co=4, y_cs=64), dict(x_cs=32), dict(y_cs=60)):
        rc, msg = call(**kw)
        assert rc == -1 and b"leaves the pixel" in msg, (kw, msg)
    for kw in (dict(x=p + 4), dict(w=p + 8), dict(scale=p + 4), dict(shift=p + 12), dict(y=p + 4)):
        rc, msg = call(**kw)
        assert rc == -1 and b"aligned" in msg, (kw, msg)
    rc, msg = call(n=64, h=4096, wd=4096, c=64, groups=4)
    assert rc == -1 and b"32 bits" in msg, msg


def test_no_cpu_fallback():
    from centermask2_amd import _lib
    from centermask2_amd.modeling import build_model
    model = build_model(x_cfg("MODEL.RESNETS.DEPTH", 50)).eval()
    with pytest.raises(_lib.CmkError):
        model.backbone(torch.zeros(1, 3, 64, 64))
