"""-m gpu: the ResNet backbones on the MI355X — the fused 7x7 stem + max-pool kernel against float64 torch on the CPU, the body and the
FPN builders against what the reference's builder produced on a plain-torch stand-in for d2's ResNet (tests/golden/make_golden_resnet.py),
the R-50 CenterMask model end to end, and a captured graph of its step.  Tolerances: the stem kernel at 4x torch's own fp32 CPU error
(see test_fused_stem_matches_float64_torch), features within 1e-3 absolute like every backbone fixture, the end-to-end comparisons
those of test_lite_model_end_to_end_matches_reference."""
import pytest
import torch
import torch.nn.functional as F

from centermask2_amd import ops, synthetic as S
from centermask2_amd.ops import View

from .helpers import close_abs, golden

pytestmark = pytest.mark.gpu

ALL = ["res2", "res3", "res4", "res5"]
STEM_CASES = [(1, 1, 1), (1, 2, 3), (1, 7, 9), (2, 64, 96), (1, 75, 109), (3, 131, 257)]
NAN_CASE = (1, 21, 22)
NAN_AT = (1, 9, 12)          # (ci, ih, iw) of the poisoned input value


def _stem_params():
    """Stem weights as the synthetic R-50 has them: Kaiming-normal 7x7 filters, a FrozenBN whose running_var is pixel-scale."""
    key = "backbone.bottom_up.stem.conv1."
    w = S.synthetic_tensor(key + "weight", (64, 3, 7, 7))
    bn = [S.synthetic_tensor(key + "norm." + n, (64,)) for n in ("weight", "bias", "running_mean", "running_var")]
    scale, shift = ops.fold_frozen_bn(*bn)
    return w, scale, shift


def _stem_torch(x, w, scale, shift, dtype):
    """conv2d -> affine -> relu -> max_pool2d(3, 2, 1) in `dtype` on the CPU, NHWC out."""
    y = F.conv2d(x.to(dtype), w.to(dtype), None, stride=2, padding=3) * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    return F.max_pool2d(F.relu(y), kernel_size=3, stride=2, padding=1).permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def stem_refs():
    """Per case: the pixel-scale input, the float64 result, and the normalised distance of torch's own fp32 CPU result from it.  `bar` is
    4x the largest of those distances: what the kernel is allowed."""
    w, scale, shift = _stem_params()
    refs, worst = {}, 0.0
    for i, (n, h, wd) in enumerate(STEM_CASES + [NAN_CASE]):
        x = S.make_synthetic_images(n, h, wd, seed0=500 + 10 * i)
        ref64 = _stem_torch(x, w, scale, shift, torch.float64)
        if (n, h, wd) != NAN_CASE:
            ref32 = _stem_torch(x, w, scale, shift, torch.float32)
            d = float((ref32.double() - ref64).abs().max()) / max(1.0, float(ref64.abs().max()))
            worst = max(worst, d)
            print("stem {}: torch fp32 vs float64 {:.3e} (max|ref| {:.2f})".format((n, h, wd), d, float(ref64.abs().max())))
        refs[(n, h, wd)] = (x, ref64)
    print("stem: largest fp32 distance {:.3e}, bar {:.3e}".format(worst, 4 * worst))
    return dict(w=w, scale=scale, shift=shift, refs=refs, bar=4 * worst)


def _run_stem(dev, x, p, co=16, extra=48):
    """The kernel into channels [co, co + 64) of a wider buffer filled with a sentinel."""
    n, _, h, wd = x.shape
    hp, wp = ((h - 1) // 2) // 2 + 1, ((wd - 1) // 2) // 2 + 1
    buf = torch.full((n, hp, wp, 64 + extra), -7.5, device=dev)
    xd = x.to(dev)
    keep = xd.clone()
    y = ops.stem7x7_bn_relu_maxpool(xd, ops.pack_stem7_weight(p["w"]).to(dev), p["scale"].to(dev), p["shift"].to(dev), View(buf, co, 64))
    torch.cuda.synchronize()
    assert y.t is buf and torch.equal(xd.view(torch.int32), keep.view(torch.int32)), "the input must be untouched"      # bit patterns: a NaN equals itself
    assert bool((buf[..., :co] == -7.5).all()) and bool((buf[..., co + 64:] == -7.5).all()), "neighbouring channels must be untouched"
    return buf[..., co:co + 64].cpu()


@pytest.mark.parametrize("case", STEM_CASES)
def test_fused_stem_matches_float64_torch(dev, stem_refs, case):
    """cmk_stem7x7_bn_relu_maxpool_nchw3 against conv2d -> affine -> relu -> max_pool2d(3, 2, 1) in float64: a single pixel, every parity
    of H and W, pooled edges whose window hangs over the conv map, several images, several workgroup tiles both ways.  The bar is 4x the
    largest distance of torch's own fp32 CPU result from the float64 one over these cases, normalised by max(1, max|ref|): the K = 147
    sums are ordered differently and the MFMA accumulates in another tree; a wrong tap or a shifted window is off by orders of magnitude
    more.  Measured (torch 2 on an x86 host): torch's fp32 distance is 7.26e-07 at most (case (3, 131, 257), max|ref| 25.3), so the bar is 2.90e-06;
    the kernel on an MI355X is 9.52e-07 from float64 at most (same case)."""
    x, ref64 = stem_refs["refs"][case]
    got = _run_stem(dev, x, stem_refs)
    assert tuple(got.shape) == tuple(ref64.shape)
    d = float((got.double() - ref64).abs().max()) / max(1.0, float(ref64.abs().max()))
    print("stem {}: kernel vs float64 {:.3e}, bar {:.3e}".format(case, d, stem_refs["bar"]))
    assert d <= stem_refs["bar"], "stem {}: {:.3e} > {:.3e}".format(case, d, stem_refs["bar"])
    dense = ops.stem7x7_bn_relu_maxpool(x.to(dev), ops.pack_stem7_weight(stem_refs["w"]).to(dev), stem_refs["scale"].to(dev), stem_refs["shift"].to(dev))
    torch.cuda.synchronize()
    assert dense.cs == 64 and torch.equal(dense.t.cpu(), got), "the dense output equals the channel-slice one"


def test_fused_stem_propagates_a_nan_like_torch(dev, stem_refs):
    """One NaN in the input: exactly the pooled outputs whose 3x3 window holds a conv pixel whose 7x7 window read it are NaN, in every
    channel (relu keeps a NaN, max_pool2d returns it); the rest meet the bar of test_fused_stem_matches_float64_torch."""
    n, h, wd = NAN_CASE
    x, _ = stem_refs["refs"][NAN_CASE]
    x = x.clone()
    ci, ih, iw = NAN_AT
    x[0, ci, ih, iw] = float("nan")
    ref64 = _stem_torch(x, stem_refs["w"], stem_refs["scale"], stem_refs["shift"], torch.float64)
    hc, wc = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    conv_rows = [r for r in range(hc) if 2 * r - 3 <= ih <= 2 * r + 3]
    conv_cols = [c for c in range(wc) if 2 * c - 3 <= iw <= 2 * c + 3]
    expect = torch.zeros((1, hp, wp, 64), dtype=torch.bool)
    for pr in range(hp):
        for pc in range(wp):
            if any(2 * pr - 1 <= r <= 2 * pr + 1 for r in conv_rows) and any(2 * pc - 1 <= c <= 2 * pc + 1 for c in conv_cols):
                expect[0, pr, pc, :] = True
    assert 0 < int(expect.sum()) < expect.numel() and torch.equal(torch.isnan(ref64), expect)
    got = _run_stem(dev, x, stem_refs)
    assert torch.equal(torch.isnan(got), expect)
    ok = ~expect
    d = float((got.double()[ok] - ref64[ok]).abs().max()) / max(1.0, float(ref64[ok].abs().max()))
    assert d <= stem_refs["bar"], "stem beside a NaN: {:.3e} > {:.3e}".format(d, stem_refs["bar"])


# ---------------------------------------------------------------------------------------------------------------------------------------
def _r50_cfg(*pairs):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_R_50_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda"] + list(pairs))
    return cfg


def _backbone(dev, name, fpn_in, top_levels, bare=False, pairs=()):
    import centermask2_amd.modeling  # noqa: F401  registers the builders
    from centermask2_amd.registry import BACKBONE_REGISTRY
    from centermask2_amd.structures import ShapeSpec
    cfg = _r50_cfg("MODEL.BACKBONE.NAME", name, "MODEL.RESNETS.OUT_FEATURES", fpn_in, "MODEL.FPN.IN_FEATURES", fpn_in, "MODEL.FCOS.TOP_LEVELS", top_levels, *pairs)
    bb = BACKBONE_REGISTRY.get(name)(cfg, ShapeSpec(channels=3)).eval()
    sd = S.make_synthetic_state_dict("R-50", 0, fpn_in=fpn_in, top_levels=top_levels)
    prefix = "backbone.bottom_up." if bare else "backbone."
    res = bb.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return bb.to(dev)


def _check_features(out, ref, names, tag, what):
    assert list(out.keys()) == names
    for k in names:
        assert tuple(out[k].shape) == tuple(ref[k + tag].shape), (k, tuple(out[k].shape))
        close_abs(out[k], ref[k + tag], 1e-3, "{} features {}".format(what, k + tag))


def test_resnet50_body_matches_reference(dev):
    """res2..res5 of the bare R-50 on the 1x3x64x96 image and the odd 1x3x75x109 image (odd maps at every down-sampling block), and on the
    first image with STRIDE_IN_1X1 False (the stride on the 3x3 conv2, only the shortcut reads the subsampled view)."""
    g = golden("resnet_backbone")
    odd = dict(golden("resnet_backbone_odd"), **{k: v for k, v in golden("resnet_backbone_fpn").items() if k.endswith("_odd")})
    x_small = S.make_synthetic_images(1, 64, 96, seed0=int(g["image_seed0"])).to(dev)
    x_odd = S.make_synthetic_images(1, 75, 109, seed0=int(g["image_seed0_odd"])).to(dev)
    body = _backbone(dev, "build_resnet_backbone", ALL, 0, bare=True)
    out = body(x_small)
    torch.cuda.synchronize()
    _check_features(out, g, ALL, "", "resnet")
    out = body(x_odd)
    torch.cuda.synchronize()
    _check_features(out, odd, ALL, "_odd", "resnet")
    body3 = _backbone(dev, "build_resnet_backbone", ALL, 0, bare=True, pairs=("MODEL.RESNETS.STRIDE_IN_1X1", False))
    out = body3(x_small)
    torch.cuda.synchronize()
    _check_features(out, golden("resnet_backbone_s3x3"), ALL, "", "resnet stride-in-3x3")


@pytest.mark.parametrize("case", [("fcos_top2", "build_fcos_resnet_fpn_backbone", ALL[1:], 2), ("maxpool", "build_resnet_fpn_backbone", ALL, 0)])
def test_resnet_fpn_builders_match_reference(dev, case):
    """The FPN builders on the 64x96 image: FCOS with TOP_LEVELS 2 over res3..res5, and d2's FPN + LastLevelMaxPool over res2..res5."""
    tag, name, fpn_in, top = case
    g = golden("resnet_backbone")
    ref = golden("resnet_backbone_fpn")[tag]
    bb = _backbone(dev, name, fpn_in, top)
    out = bb(S.make_synthetic_images(1, 64, 96, seed0=int(g["image_seed0"])).to(dev))
    torch.cuda.synchronize()
    _check_features(out, ref, list(ref.keys()), "", "resnet " + tag)
    if tag == "maxpool":
        assert torch.equal(out["p6"], out["p5"][:, :, ::2, ::2])


@pytest.fixture(scope="module")
def r50_model(dev):
    from centermask2_amd.modeling import build_model
    model = build_model(_r50_cfg()).eval()
    model.load_state_dict(S.make_synthetic_state_dict("R-50", 0), strict=True)
    return model


def test_r50_model_end_to_end_matches_reference(dev, r50_model):
    """Two images through ResNet-50-FPN -> FCOS -> CenterROIHeads against what the reference's own modules produced: labels, ROI locations
    and their order exact, boxes, scores, mask probabilities and mask scores at the tolerances of
    test_lite_model_end_to_end_matches_reference."""
    from centermask2_amd.structures import FakeImageList
    from .test_gpu_model import ORDER_TOL, _check_against_reference_image, _probe_check
    g = golden("e2e_r50")
    h, w = (int(v) for v in g["image_hw"])
    x = S.make_synthetic_images(2, h, w, seed0=int(g["image_seed0"])).to(dev)
    sizes = [(h, w), (h, w)]
    names = ("p3", "p4", "p5", "p6", "p7")
    feats = r50_model.backbone(x)
    for k in names:
        _probe_check(feats[k], g[k], 1e-3, "r50 " + k)
    lg, reg, ctr, _ = r50_model.proposal_generator.fcos_head([feats[k] for k in names])
    for l in range(5):
        _probe_check(lg[l], g["logits{}".format(l)], 1e-3, "r50 logits{}".format(l))
        _probe_check(reg[l], g["reg{}".format(l)], 1e-3, "r50 reg{}".format(l))
        _probe_check(ctr[l], g["ctr{}".format(l)], 1e-3, "r50 ctr{}".format(l))
    res = r50_model.inference(FakeImageList(x, sizes), do_preprocess=False, do_postprocess=False)
    torch.cuda.synchronize()
    for i in range(2):
        r, inst = g["img{}".format(i)], res[i]
        assert 5 <= r["scores"].shape[0] <= 50
        _check_against_reference_image(inst, r, "r50 e2e image {}".format(i), ORDER_TOL)
        assert inst.pred_classes.dtype == torch.int64 and tuple(inst.pred_masks.shape[1:]) == (1, 28, 28)


def test_r50_graph_replay_of_inference_padded_equals_eager(dev, r50_model):
    """The launch sequence of the R-50 step is static (no memset, no host sync): a graph of inference_padded captured on one batch and
    replayed on new images gives what an eager run on those images gives, bit for bit."""
    sizes = [(256, 320), (256, 320)]
    a = S.make_synthetic_images(2, 256, 320, seed0=4100).to(dev)
    b = S.make_synthetic_images(2, 256, 320, seed0=4200).to(dev)
    static = a.clone()
    r50_model.inference_padded(static, sizes)                 # warm-up: packs the weights, fills the allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = r50_model.inference_padded(static, sizes)
    static.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    names = ("box", "score", "cls", "loc", "counts", "pred_masks", "mask_scores")
    got = {k: out[k].clone() for k in names}
    eager = r50_model.inference_padded(b, sizes)
    torch.cuda.synchronize()
    assert int(eager["counts"].min()) > 0 and not torch.equal(got["pred_masks"], r50_model.inference_padded(a, sizes)["pred_masks"])
    for k in names:
        assert torch.equal(got[k], eager[k]), k
