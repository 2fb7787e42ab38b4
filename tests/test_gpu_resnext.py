"""-m gpu: the ResNeXt backbones on the MI355X — the grouped 3x3 conv kernel against float64 torch on the CPU, non-finite inputs staying
inside their group, the bodies against what the reference's builder produced on the plain-torch stand-in for d2's ResNet
(tests/golden/make_golden_resnext.py), the X-101-32x8d CenterMask model end to end, and a captured graph of its step.  Tolerances: the kernel at
4x torch's own fp32 CPU error (see test_group_conv_matches_float64_torch), features within 1e-3 absolute like every backbone fixture,
the end-to-end comparisons those of test_lite_model_end_to_end_matches_reference."""
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

from centermask2_amd import ops, synthetic as S
from centermask2_amd.ops import View

from .helpers import close_abs, golden

pytestmark = pytest.mark.gpu

ALL = ["res2", "res3", "res4", "res5"]
YAML = "centermask_X_101_32x8d_FPN_ms_3x.yaml"
MAPS = [(1, 1, 1), (1, 2, 3), (1, 7, 9), (2, 13, 17), (2, 21, 41)]          # the last one spans several workgroup tiles at every Cg and stride
CONV_CASES = [(cg, 4, s) for cg in (4, 8, 16, 32, 64) for s in (1, 2)] + [(cg, 32, s) for cg in (4, 8, 64) for s in (1, 2)]
WIDE_MAPS = [(1, 5, 6)]                                                      # groups = 32: the real widths 256 and 2048 (and 128 at Cg 4)
NAN_MAP, NAN_AT, NAN_GROUP = (1, 6, 7), (3, 3), 1


def _maps(groups):
    return MAPS if groups == 4 else WIDE_MAPS


def _params(cg, groups):
    """A grouped conv2 as the synthetic ResNeXt bodies have it: Kaiming-normal on the grouped fan-in 9 * Cg, a synthetic FrozenBN folded."""
    c = cg * groups
    key = "backbone.bottom_up.res{}.0.conv2.".format({4: 2, 8: 2, 16: 3, 32: 4, 64: 5}[cg])
    w = S.synthetic_tensor(key + "weight", (c, cg, 3, 3))
    scale, shift = ops.fold_frozen_bn(*[S.synthetic_tensor(key + "norm." + n, (c,)) for n in ("weight", "bias", "running_mean", "running_var")])
    return w, scale, shift


def _input(case, m):
    """Non-negative, post-ReLU-like: half zeros, the rest half-normal."""
    cg, groups, s = case
    n, h, wd = m
    g = torch.Generator()
    g.manual_seed(7000 + 1000 * cg + 10 * groups + s + 31 * h + wd)
    return torch.relu(torch.randn((n, cg * groups, h, wd), generator=g))


def _torch(x, w, scale, shift, groups, stride, dtype):
    """conv2d(groups) -> affine -> relu in `dtype` on the CPU, NHWC out."""
    y = F.conv2d(x.to(dtype), w.to(dtype), None, stride=stride, padding=1, groups=groups) * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    return F.relu(y).permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def conv_refs():
    """Per case and map: the input and the float64 result; `bar` is 4x the largest normalised distance of torch's own fp32 CPU result from
    the float64 one over all of them."""
    refs, params, worst = {}, {}, 0.0
    for case in CONV_CASES:
        cg, groups, s = case
        params[(cg, groups)] = _params(cg, groups)
        w, scale, shift = params[(cg, groups)]
        for m in _maps(groups):
            x = _input(case, m)
            ref64 = _torch(x, w, scale, shift, groups, s, torch.float64)
            ref32 = _torch(x, w, scale, shift, groups, s, torch.float32)
            d = float((ref32.double() - ref64).abs().max()) / max(1.0, float(ref64.abs().max()))
            worst = max(worst, d)
            refs[(case, m)] = (x, ref64)
    print("group conv: largest torch fp32 distance from float64 {:.3e}, bar {:.3e}".format(worst, 4 * worst))
    return dict(refs=refs, params=params, bar=4 * worst)


def _run(dev, x, params, groups, stride, x_co=8, x_extra=12, y_co=16, y_extra=48):
    """The kernel reading channels [x_co, x_co + C) of a wider buffer and writing channels [y_co, y_co + C) of a wider sentinel-filled one."""
    w, scale, shift = params
    n, c, h, wd = x.shape
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    xbuf = torch.full((n, h, wd, c + x_extra), 3.25, device=dev)
    xbuf[..., x_co:x_co + c] = x.permute(0, 2, 3, 1).to(dev)
    keep = xbuf.clone()
    ybuf = torch.full((n, ho, wo, c + y_extra), -7.5, device=dev)
    pc = ops.PackedGroupConv(w, scale, shift, dev, groups, stride=stride)
    y = ops.group_conv3x3(View(xbuf, x_co, c), pc, View(ybuf, y_co, c), relu=True)
    torch.cuda.synchronize()
    assert y.t is ybuf and torch.equal(xbuf.view(torch.int32), keep.view(torch.int32)), "the input must be untouched"     # bit patterns: a NaN equals itself
    assert bool((ybuf[..., :y_co] == -7.5).all()) and bool((ybuf[..., y_co + c:] == -7.5).all()), "neighbouring channels must be untouched"
    return ybuf[..., y_co:y_co + c].cpu(), pc


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "cg{}-g{}-s{}".format(*c))
def test_group_conv_matches_float64_torch(dev, conv_refs, case):
    """cmk_group_conv3x3_nhwc against F.conv2d(groups) -> affine -> relu in float64, per (Cg, groups, stride) on every map of its list: a single
    pixel, odd and even sizes at both strides, several images, and the (2, 21, 41) map that spans several tiles at every Cg.  Tile sizes
    (csrc/conv_group3.hip): for Cg 16 / 32 / 64 a workgroup is one group (Cg channels: 4 channel tiles here) x 8 x 16 output pixels at stride 1
    (3 x 3 tiles on that map) and 4 x 16 at stride 2 (3 x 2 tiles on its 11 x 21 output); for Cg 4 / 8 a thread is 4 channels x 2 rows x
    2 columns at stride 1 (11 x 21 thread tiles per image) and 2 x 4 at stride 2 (6 x 6), a workgroup 16 channel quads x 16 consecutive thread
    tiles: 4 or 8 channel quads and 5 or more workgroups on that map, and 2 (Cg 4) and 4 (Cg 8) channel chunks in the groups = 32 cases.  The input is read from a channel slice of a
    wider buffer and the output written into a slice of a sentinel-filled one; the dense call must equal it bit for bit.  The bar is 4x the
    largest distance of torch's own fp32 CPU result from the float64 one over all these cases, normalised by max(1, max|ref|): the K =
    9 * Cg sums are ordered differently; a wrong tap, channel or group is off by orders of magnitude more.
    Measured (torch 2 on an x86 host): torch's fp32 distance is 4.48e-07 at most, so the bar is 1.79e-06; the kernel on an MI355X is 9.01e-07 from
    float64 at most (Cg 64, stride 2, the (2, 21, 41) map), 2.1e-07 at most for Cg 4 / 8 and 3.6e-07 for Cg 16."""
    cg, groups, s = case
    params = conv_refs["params"][(cg, groups)]
    for m in _maps(groups):
        x, ref64 = conv_refs["refs"][(case, m)]
        got, pc = _run(dev, x, params, groups, s)
        assert tuple(got.shape) == tuple(ref64.shape)
        d = float((got.double() - ref64).abs().max()) / max(1.0, float(ref64.abs().max()))
        print("group conv {} map {}: kernel vs float64 {:.3e}, bar {:.3e}".format(case, m, d, conv_refs["bar"]))
        assert d <= conv_refs["bar"], "group conv {} map {}: {:.3e} > {:.3e}".format(case, m, d, conv_refs["bar"])
        dense = ops.group_conv3x3(View(x.permute(0, 2, 3, 1).contiguous().to(dev)), pc, relu=True)
        torch.cuda.synchronize()
        assert dense.cs == cg * groups and dense.co == 0 and torch.equal(dense.t.cpu(), got), "the dense output equals the channel-slice one"


@pytest.mark.parametrize("cg", [4, 8, 16])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_group_conv_keeps_non_finite_values_inside_their_group(dev, conv_refs, cg, poison):
    """One NaN (or one +Inf) in a channel of group 1 of 4, stride 1: the outputs are non-finite exactly where float64 torch's are (the 3x3
    neighbourhood, group 1 only; an Inf that the ReLU clips to 0 is finite in both), NaN where torch has NaN and Inf where it has Inf;
    every finite output, all of the other groups among them, meets the bar of test_group_conv_matches_float64_torch."""
    groups = 4
    params = conv_refs["params"][(cg, groups)]
    x = _input((cg, groups, 1), NAN_MAP).clone()
    x[0, NAN_GROUP * cg + cg // 2, NAN_AT[0], NAN_AT[1]] = poison
    ref64 = _torch(x, *params, groups, 1, torch.float64)
    bad = ~torch.isfinite(ref64)
    inside = torch.zeros_like(bad)
    inside[0, NAN_AT[0] - 1:NAN_AT[0] + 2, NAN_AT[1] - 1:NAN_AT[1] + 2, NAN_GROUP * cg:(NAN_GROUP + 1) * cg] = True
    assert bool(bad.any()) and not bool((bad & ~inside).any()), "the reference keeps the poison inside group 1's 3x3 neighbourhood"
    got, _ = _run(dev, x, params, groups, 1)
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)) and torch.equal(torch.isinf(got), torch.isinf(ref64))
    other = torch.ones(cg * groups, dtype=torch.bool)
    other[NAN_GROUP * cg:(NAN_GROUP + 1) * cg] = False
    assert bool(torch.isfinite(got[..., other]).all()), "every output of every other group is finite"
    ok = ~bad
    d = float((got.double()[ok] - ref64[ok]).abs().max()) / max(1.0, float(ref64[ok].abs().max()))
    assert d <= conv_refs["bar"], "group conv beside a non-finite value: {:.3e} > {:.3e}".format(d, conv_refs["bar"])


# ---------------------------------------------------------------------------------------------------------------------------------------
def _x_cfg(*pairs):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path(YAML))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda"] + list(pairs))
    return cfg


def _bare_body(dev, depth, groups, wpg, stride_in_1x1):
    """The bare body with the tensors make_golden_resnext.py loaded into the reference."""
    import centermask2_amd.modeling  # noqa: F401  registers the builders
    from centermask2_amd.registry import BACKBONE_REGISTRY
    from centermask2_amd.structures import ShapeSpec
    cfg = _x_cfg("MODEL.BACKBONE.NAME", "build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.RESNETS.DEPTH", depth, "MODEL.RESNETS.NUM_GROUPS", groups,
                 "MODEL.RESNETS.WIDTH_PER_GROUP", wpg, "MODEL.RESNETS.STRIDE_IN_1X1", stride_in_1x1)
    bb = BACKBONE_REGISTRY.get("build_resnet_backbone")(cfg, ShapeSpec(channels=3)).eval()
    shapes = S.resnet_param_shapes(depth, "backbone.bottom_up.", width=groups * wpg, groups=groups)
    sd = S.make_synthetic_state_dict("X-50-32x4d", 0, shapes=shapes)
    res = bb.load_state_dict(OrderedDict((k[len("backbone.bottom_up."):], v) for k, v in sd.items()), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return bb.to(dev)


def _check_features(out, ref, names, what):
    assert list(out.keys()) == names
    for k in names:
        assert tuple(out[k].shape) == tuple(ref[k].shape), (k, tuple(out[k].shape))
        close_abs(out[k], ref[k], 1e-3, "{} features {}".format(what, k))


def test_resnext_bodies_match_reference(dev):
    """res2..res5 of the bare X-50-32x4d (Cg 4 / 8 / 16 / 32, STRIDE_IN_1X1 True) on the 1x3x64x96 image, and of a depth-50 body with 32
    groups of width 8 (Cg 8 / 16 / 32 / 64) and STRIDE_IN_1X1 False on the odd 1x3x75x109 image: a stride-2 grouped conv on an odd map in
    the first block of res3, res4 and res5."""
    g = golden("resnext_backbone_32x4d")
    x_small = S.make_synthetic_images(1, 64, 96, seed0=int(g["image_seed0"])).to(dev)
    out = _bare_body(dev, 50, 32, 4, True)(x_small)
    torch.cuda.synchronize()
    _check_features(out, g, ALL, "resnext 32x4d")
    odd = dict(golden("resnext_backbone_32x8d"), **golden("resnext_backbone_32x8d_b"))
    x_odd = S.make_synthetic_images(1, 75, 109, seed0=int(odd["image_seed0_odd"])).to(dev)
    out = _bare_body(dev, 50, 32, 8, False)(x_odd)
    torch.cuda.synchronize()
    _check_features(out, odd, ALL, "resnext 32x8d odd")


@pytest.fixture(scope="module")
def x101_model(dev):
    from centermask2_amd.modeling import build_model
    model = build_model(_x_cfg()).eval()
    model.load_state_dict(S.make_synthetic_state_dict("X-101-32x8d", 0), strict=True)
    return model


def test_x101_model_end_to_end_matches_reference(dev, x101_model):
    """Two images through X-101-32x8d-FPN -> FCOS -> CenterROIHeads (the shipped yaml) against what the reference's own modules produced:
    labels, ROI locations and their order exact, boxes, scores, mask probabilities and mask scores at the tolerances of
    test_lite_model_end_to_end_matches_reference."""
    from centermask2_amd.structures import FakeImageList
    from .test_gpu_model import ORDER_TOL, _check_against_reference_image, _probe_check
    g = golden("e2e_x101")
    h, w = (int(v) for v in g["image_hw"])
    x = S.make_synthetic_images(2, h, w, seed0=int(g["image_seed0"])).to(dev)
    sizes = [(h, w), (h, w)]
    names = ("p3", "p4", "p5", "p6", "p7")
    feats = x101_model.backbone(x)
    for k in names:
        _probe_check(feats[k], g[k], 1e-3, "x101 " + k)
    lg, reg, ctr, _ = x101_model.proposal_generator.fcos_head([feats[k] for k in names])
    for l in range(5):
        _probe_check(lg[l], g["logits{}".format(l)], 1e-3, "x101 logits{}".format(l))
        _probe_check(reg[l], g["reg{}".format(l)], 1e-3, "x101 reg{}".format(l))
        _probe_check(ctr[l], g["ctr{}".format(l)], 1e-3, "x101 ctr{}".format(l))
    res = x101_model.inference(FakeImageList(x, sizes), do_preprocess=False, do_postprocess=False)
    torch.cuda.synchronize()
    for i in range(2):
        r, inst = g["img{}".format(i)], res[i]
        assert 5 <= r["scores"].shape[0] <= 50
        _check_against_reference_image(inst, r, "x101 e2e image {}".format(i), ORDER_TOL)
        assert inst.pred_classes.dtype == torch.int64 and tuple(inst.pred_masks.shape[1:]) == (1, 28, 28)


def test_x101_graph_replay_of_inference_padded_equals_eager(dev, x101_model):
    """The launch sequence of the X-101 step is static (the grouped conv is one launch with no workspace): a graph of inference_padded
    captured on one batch and replayed on new images gives what an eager run on those images gives, bit for bit."""
    sizes = [(256, 320), (256, 320)]
    a = S.make_synthetic_images(2, 256, 320, seed0=4100).to(dev)
    b = S.make_synthetic_images(2, 256, 320, seed0=4200).to(dev)
    static = a.clone()
    x101_model.inference_padded(static, sizes)                 # warm-up: packs the weights, fills the allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = x101_model.inference_padded(static, sizes)
    static.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    names = ("box", "score", "cls", "loc", "counts", "pred_masks", "mask_scores")
    got = {k: out[k].clone() for k in names}
    eager = x101_model.inference_padded(b, sizes)
    torch.cuda.synchronize()
    assert int(eager["counts"].min()) > 0 and not torch.equal(got["pred_masks"], x101_model.inference_padded(a, sizes)["pred_masks"])
    for k in names:
        assert torch.equal(got[k], eager[k]), k
