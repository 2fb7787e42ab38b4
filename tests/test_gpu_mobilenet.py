"""-m gpu: the MobileNetV2 backbone on the MI355X — the fused depth-wise kernel against torch on the CPU, the body and the three builders
against what the reference's own modules produced (tests/golden/make_golden_mnv2.py), the CenterMask-Lite model end to end, and a
captured graph of its step.  Tolerances: the kernel at the bar of test_depthwise_conv3x3 (1e-5 x max(1, max|ref|)), features within
1e-3 absolute like every backbone fixture, the end-to-end comparisons those of test_end_to_end_800x1280_matches_reference."""
import pytest
import torch
import torch.nn.functional as F

from centermask2_amd import ops, synthetic as S
from centermask2_amd.ops import View

from .helpers import close, close_abs, golden

pytestmark = pytest.mark.gpu

INF = float("inf")
LITE = dict(fpn_ch=128, mask_dim=128, num_tower_convs=2, mask_num_conv=2, maskiou_num_conv=2)
ALL = ["res2", "res3", "res4", "res5"]


def _dw_reference(x_nhwc, wt, scale, shift, stride, in_max, out_min, out_max):
    """torch on the CPU: conv2d(groups=C) on clamp(max=in_max), the affine, then the clamp.  NHWC in, NHWC out."""
    c = wt.shape[0]
    xc = x_nhwc.permute(0, 3, 1, 2).cpu()
    if in_max != INF:
        xc = xc.clamp(max=in_max)
    y = F.conv2d(xc, wt, None, stride=stride, padding=1, groups=c) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if out_min != -INF or out_max != INF:
        y = y.clamp(min=out_min, max=out_max)
    return y.permute(0, 2, 3, 1)


# (N, H, W, C, stride, clamps on)
DW_CASES = [(2, 37, 53, 64, 1, True), (1, 40, 64, 112, 2, True), (3, 9, 7, 144, 1, True), (1, 1, 1, 4, 2, True), (1, 1, 1, 4, 1, False),
            (2, 30, 31, 96, 2, False), (1, 25, 40, 960, 1, True), (2, 13, 21, 576, 2, True), (1, 5, 3, 8, 1, False), (8, 50, 80, 192, 1, True),
            (2, 201, 323, 68, 1, True), (2, 203, 321, 136, 2, True),      # large enough for the largest per-thread tiles, odd edges
            (4, 50, 81, 144, 1, True), (8, 100, 161, 96, 2, True)]        # ... and for the middle ones


@pytest.mark.parametrize("case", DW_CASES)
def test_fused_depthwise_bn_act_matches_torch(dev, case):
    n, h, w, c, stride, clamps = case
    g = torch.Generator().manual_seed(17)
    # inputs of std 4 around 1: a good share above 6 and below 0; 3x3 sums of std ~4 after the affine: both output clamps fire
    buf = (torch.randn((n, h, w, c + 16), generator=g) * 4.0 + 1.0).to(dev)
    wt = torch.randn((c, 1, 3, 3), generator=g) / 3.0
    scale = torch.rand(c, generator=g) + 0.5
    shift = torch.randn(c, generator=g) + 2.0
    in_max, lo, hi = (6.0, 0.0, 6.0) if clamps else (INF, -INF, INF)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    ybuf = torch.full((n, ho, wo, c + 8), 7.0, device=dev)
    before = buf.clone()
    y = ops.dwconv3x3_bn_act(View(buf, 8, c), ops.pack_dw_weight(wt).to(dev), scale.to(dev), shift.to(dev), View(ybuf, 4, c), stride=stride,
                             in_max=in_max, out_min=lo, out_max=hi)
    torch.cuda.synchronize()
    ref = _dw_reference(before[..., 8:8 + c], wt, scale, shift, stride, in_max, lo, hi)
    close(ybuf[..., 4:4 + c], ref, 1e-5, "dwconv3x3_bn_act")
    assert float(ybuf[..., :4].min()) == 7.0 and float(ybuf[..., 4 + c:].max()) == 7.0        # neighbouring channels untouched
    assert torch.equal(buf, before) and y.c == c
    if clamps and ref.numel() >= 64:                     # the case does exercise all three clamps
        xin = before[..., 8:8 + c].cpu()
        assert float((xin > 6).float().mean()) > 0.02 and float((ref == 0).float().mean()) > 0.02 and float((ref == 6).float().mean()) > 0.02
        assert float(ybuf[..., 4:4 + c].min()) == 0.0 and float(ybuf[..., 4:4 + c].max()) == 6.0


def test_fused_depthwise_allocates_its_output_and_defaults_to_no_clamp(dev):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((2, 11, 14, 32), generator=g) * 5.0).to(dev)
    wt, scale, shift = torch.randn((32, 1, 3, 3), generator=g), torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    y = ops.dwconv3x3_bn_act(View(x), ops.pack_dw_weight(wt).to(dev), scale.to(dev), shift.to(dev), stride=2)
    torch.cuda.synchronize()
    assert tuple(y.t.shape) == (2, 6, 7, 32)
    close(y.t, _dw_reference(x, wt, scale, shift, 2, INF, -INF, INF), 1e-5, "dwconv3x3_bn_act defaults")


@pytest.mark.parametrize("stride", [1, 2])
def test_fused_depthwise_propagates_nan(dev, stride):
    """One NaN in the input: exactly the outputs of its channel whose 3x3 window holds it are NaN, as with torch.nn.ReLU6 (a clamp written
    with fminf / fmaxf would return the bound)."""
    n, h, w, c = 1, 9, 10, 16
    g = torch.Generator().manual_seed(23)
    x = torch.randn((n, h, w, c), generator=g) * 4.0
    x[0, 4, 5, 6] = float("nan")
    wt, scale, shift = torch.randn((c, 1, 3, 3), generator=g) / 3.0, torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    y = ops.dwconv3x3_bn_act(View(x.to(dev)), ops.pack_dw_weight(wt).to(dev), scale.to(dev), shift.to(dev), stride=stride, in_max=6.0, out_min=0.0,
                             out_max=6.0)
    torch.cuda.synchronize()
    ref = _dw_reference(x, wt, scale, shift, stride, 6.0, 0.0, 6.0)
    got = y.t.cpu()
    want = torch.zeros_like(got, dtype=torch.bool)
    for oh in range(got.shape[1]):
        for ow in range(got.shape[2]):
            want[0, oh, ow, 6] = abs(oh * stride - 4) <= 1 and abs(ow * stride - 5) <= 1
    assert int(want.sum()) == (9 if stride == 1 else 2) and torch.equal(torch.isnan(got), want)
    ok = ~torch.isnan(ref) & ~want
    close(got[ok], ref[ok], 1e-5, "dwconv3x3_bn_act beside a NaN")


# ---------------------------------------------------------------------------------------------------------------------------------------
def _lite_cfg(*pairs):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_lite_Mv2_FPN_ms_4x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda"] + list(pairs))
    return cfg


def _backbone(dev, name, fpn_in, top_levels, bare=False):
    import centermask2_amd.modeling  # noqa: F401  registers the builders
    from centermask2_amd.registry import BACKBONE_REGISTRY
    from centermask2_amd.structures import ShapeSpec
    cfg = _lite_cfg("MODEL.BACKBONE.NAME", name, "MODEL.RESNETS.OUT_FEATURES", fpn_in, "MODEL.FPN.IN_FEATURES", fpn_in, "MODEL.FCOS.TOP_LEVELS", top_levels)
    bb = BACKBONE_REGISTRY.get(name)(cfg, ShapeSpec(channels=3)).eval()
    sd = S.make_synthetic_state_dict(S.MOBILENETV2, 0, fpn_in=fpn_in, top_levels=top_levels, **LITE)
    prefix = "backbone.bottom_up." if bare else "backbone."
    res = bb.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return bb.to(dev)


def _fixture_inputs(g):
    return (S.make_synthetic_images(2, 64, 96, seed0=int(g["image_seed0"])), S.make_synthetic_images(1, 75, 109, seed0=int(g["image_seed0_odd"])))


def test_mobilenetv2_body_matches_reference(dev):
    """res2..res5 of the bare body on the 2x3x64x96 batch and on the odd 1x3x75x109 image; NCHW with the true channel counts (res2 is
    sliced back from its 32-channel buffer, whose pad lanes must be zeros)."""
    g = golden("mnv2_backbone")
    body = _backbone(dev, "build_mnv2_backbone", ALL, 0, bare=True)
    for tag, x in zip(("", "_odd"), _fixture_inputs(g)):
        out = body(x.to(dev))
        torch.cuda.synchronize()
        assert list(out.keys()) == ALL
        for k in ALL:
            assert tuple(out[k].shape) == tuple(g[k + tag].shape), (k, tuple(out[k].shape))
            close_abs(out[k], g[k + tag], 1e-3, "mnv2 features " + k + tag)
        views = body.forward_views(x.to(dev))
        torch.cuda.synchronize()
        assert views["res2"].c == 32 and float(views["res2"].t[..., 24:].abs().max()) == 0.0
        assert torch.equal(views["res2"].t[..., :24].permute(0, 3, 1, 2), out["res2"])


@pytest.mark.parametrize("case", [("fcos_top2", "build_fcos_mobilenetv2_fpn_backbone", ALL[1:], 2), ("fcos_top1", "build_fcos_mobilenetv2_fpn_backbone", ALL[1:], 1),
                                  ("maxpool", "build_mobilenetv2_fpn_backbone", ALL, 0)])
def test_mobilenetv2_fpn_builders_match_reference(dev, case):
    """The FPN builders on the 64x96 batch: FCOS with TOP_LEVELS 2 and 1 over res3..res5, and FPN + LastLevelMaxPool over res2..res5 (the
    24-channel lateral reads the zero-padded 32-wide view)."""
    tag, name, fpn_in, top = case
    g = golden("mnv2_backbone")
    bb = _backbone(dev, name, fpn_in, top)
    out = bb(_fixture_inputs(g)[0].to(dev))
    torch.cuda.synchronize()
    assert list(out.keys()) == list(g[tag].keys())
    for k in out:
        assert tuple(out[k].shape) == tuple(g[tag][k].shape), (k, tuple(out[k].shape))
        close_abs(out[k], g[tag][k], 1e-3, "mnv2 {} features {}".format(tag, k))
    if tag == "maxpool":
        assert torch.equal(out["p6"], out["p5"][:, :, ::2, ::2])


@pytest.fixture(scope="module")
def lite_model(dev):
    from centermask2_amd.modeling import build_model
    model = build_model(_lite_cfg()).eval()
    model.load_state_dict(S.make_synthetic_state_dict(S.MOBILENETV2, 0, **LITE), strict=True)
    return model


def test_lite_model_end_to_end_matches_reference(dev, lite_model):
    """Two images through MobileNetV2-FPN -> FCOS (2 tower convs, 128 wide) -> CenterROIHeads (2 + 2 convs, 128 wide) against what the
    reference's own modules produced: labels, ROI locations and their order exact, boxes, scores, mask probabilities and mask scores at
    the tolerances of test_end_to_end_800x1280_matches_reference."""
    from centermask2_amd.structures import FakeImageList
    from .test_gpu_model import ORDER_TOL, _check_against_reference_image, _probe_check
    g = golden("e2e_mnv2_lite")
    h, w = (int(v) for v in g["image_hw"])
    x = S.make_synthetic_images(2, h, w, seed0=int(g["image_seed0"])).to(dev)
    sizes = [(h, w), (h, w)]
    names = ("p3", "p4", "p5", "p6", "p7")
    feats = lite_model.backbone(x)
    for k in names:
        _probe_check(feats[k], g[k], 1e-3, "lite " + k)
    lg, reg, ctr, _ = lite_model.proposal_generator.fcos_head([feats[k] for k in names])
    for l in range(5):
        _probe_check(lg[l], g["logits{}".format(l)], 1e-3, "lite logits{}".format(l))
        _probe_check(reg[l], g["reg{}".format(l)], 1e-3, "lite reg{}".format(l))
        _probe_check(ctr[l], g["ctr{}".format(l)], 1e-3, "lite ctr{}".format(l))
    res = lite_model.inference(FakeImageList(x, sizes), do_preprocess=False, do_postprocess=False)
    torch.cuda.synchronize()
    for i in range(2):
        r, inst = g["img{}".format(i)], res[i]
        assert 5 <= r["scores"].shape[0] <= 50
        _check_against_reference_image(inst, r, "lite e2e image {}".format(i), ORDER_TOL)
        assert inst.pred_classes.dtype == torch.int64 and tuple(inst.pred_masks.shape[1:]) == (1, 28, 28)


def test_lite_graph_replay_of_inference_padded_equals_eager(dev, lite_model):
    """The launch sequence of the Lite step is static (no memset for the padded channels, no host sync): a graph of inference_padded
    captured on one batch and replayed on new images gives what an eager run on those images gives, bit for bit."""
    sizes = [(256, 320), (256, 320)]
    a = S.make_synthetic_images(2, 256, 320, seed0=4100).to(dev)
    b = S.make_synthetic_images(2, 256, 320, seed0=4200).to(dev)
    static = a.clone()
    lite_model.inference_padded(static, sizes)                # warm-up: packs the weights, fills the allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lite_model.inference_padded(static, sizes)
    static.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    names = ("box", "score", "cls", "loc", "counts", "pred_masks", "mask_scores")
    got = {k: out[k].clone() for k in names}
    eager = lite_model.inference_padded(b, sizes)
    torch.cuda.synchronize()
    assert int(eager["counts"].min()) > 0 and not torch.equal(got["pred_masks"], lite_model.inference_padded(a, sizes)["pred_masks"])
    for k in names:
        assert torch.equal(got[k], eager[k]), k
