"""MODEL.KEYPOINT_ON without a GPU: the model builds with the keypoint head under the reference's parameter names (the fixture
tests/golden/roi_keypoint.pt carries the reference head's own state dict), the score_lowres repack equals torch's conv_transpose2d, the
config defaults, the refusals at construction, and every place that hands results on — post-processing, COCO json, the multi-GPU record
and its C ABI's argument checks."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from centermask2_amd import synthetic as S
from centermask2_amd.config import config_path, get_cfg
from centermask2_amd.structures import Boxes, Instances, ShapeSpec

from .helpers import golden

K = 17


def _cfg(*opts):
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.KEYPOINT_ON", True] + list(opts))
    return cfg


P345 = ["MODEL.ROI_KEYPOINT_HEAD.IN_FEATURES", ["p3", "p4", "p5"]]


def test_new_config_defaults():
    cfg = get_cfg()
    kh = cfg.MODEL.ROI_KEYPOINT_HEAD
    assert (kh.POOLER_RESOLUTION, kh.POOLER_SAMPLING_RATIO, kh.POOLER_TYPE, kh.NUM_KEYPOINTS) == (14, 0, "ROIAlignV2", 17)
    assert tuple(kh.CONV_DIMS) == (512,) * 8
    assert (kh.MIN_KEYPOINTS_PER_IMAGE, kh.NORMALIZE_LOSS_BY_VISIBLE_KEYPOINTS, kh.LOSS_WEIGHT) == (1, True, 1.0)
    assert (kh.NAME, list(kh.IN_FEATURES), kh.ASSIGN_CRITERION) == ("KRCNNConvDeconvUpsampleHead", ["p2", "p3", "p4", "p5"], "ratio")
    assert list(cfg.TEST.KEYPOINT_OKS_SIGMAS) == [] and cfg.MODEL.KEYPOINT_ON is False


def test_keypoint_model_builds_on_cpu_and_loads_synthetic_weights():
    from centermask2_amd.modeling import build_model
    from centermask2_amd.modeling.centermask.keypoint_head import KRCNNConvDeconvUpsampleHead
    from centermask2_amd.registry import ROI_KEYPOINT_HEAD_REGISTRY
    model = build_model(_cfg(*P345)).eval()
    heads = model.roi_heads
    assert heads.keypoint_on and list(heads.kp_in_features) == ["p3", "p4", "p5"]
    assert isinstance(heads.keypoint_head, KRCNNConvDeconvUpsampleHead) and "KRCNNConvDeconvUpsampleHead" in ROI_KEYPOINT_HEAD_REGISTRY
    pool = heads.keypoint_pooler
    assert (pool.output_size, pool.sampling_ratio, pool.aligned, pool.assign_crit) == (14, 0, True, "ratio")
    assert pool.scales == (1 / 8, 1 / 16, 1 / 32) and (pool.min_level, pool.max_level) == (3, 5)
    shapes = S.model_param_shapes("V-39-eSE", keypoint_on=True)
    kp = {k: v for k, v in shapes.items() if k.startswith("roi_heads.keypoint_head.")}
    assert len(kp) == 18 and kp["roi_heads.keypoint_head.conv_fcn1.weight"] == (512, 256, 3, 3)
    assert kp["roi_heads.keypoint_head.score_lowres.weight"] == (512, K, 4, 4) and kp["roi_heads.keypoint_head.score_lowres.bias"] == (K,)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == dict(shapes)
    sd = S.make_synthetic_state_dict("V-39-eSE", 0, keypoint_on=True)
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    # existing names keep their values: every tensor has its own generator
    base = S.make_synthetic_state_dict("V-39-eSE", 0)
    assert list(S.model_param_shapes("V-39-eSE")) == list(base) and all(torch.equal(sd[k], v) for k, v in base.items())
    w = sd["roi_heads.keypoint_head.score_lowres.weight"]
    assert abs(float(w.std()) - 3.0 * (1.0 / (4 * 512)) ** 0.5) < 0.02 * float(w.std())


@pytest.mark.parametrize("setup", ["p3_p5", "p2_p5"])
def test_head_parameters_equal_the_reference_heads(setup):
    """Names and shapes of roi_heads.keypoint_head.* equal the state dict of the reference's own head (the fixture's), which then loads."""
    from centermask2_amd.modeling.centermask.center_heads import CenterROIHeads
    fx = golden("roi_keypoint")[setup]
    feats = fx["in_features"]
    cfg = _cfg("MODEL.ROI_KEYPOINT_HEAD.IN_FEATURES", feats, "MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", tuple(fx["conv_dims"].tolist()))
    shapes = {"p{}".format(l): ShapeSpec(channels=fx[feats[0]].shape[1] if "p{}".format(l) in feats else 256, stride=2 ** l) for l in range(2, 8)}
    heads = CenterROIHeads(cfg, shapes)
    ours = {k: tuple(v.shape) for k, v in heads.keypoint_head.state_dict().items()}
    assert ours == {k: tuple(v.shape) for k, v in fx["state_dict"].items()} and list(ours) == list(fx["state_dict"])
    heads.keypoint_head.load_state_dict(fx["state_dict"], strict=True)
    assert heads.keypoint_pooler.min_level == int(feats[0][1]) and len(heads.keypoint_pooler.scales) == len(feats)


def test_score_lowres_repack_equals_conv_transpose2d():
    from centermask2_amd.modeling.centermask.keypoint_head import deconv4x4s2_as_conv3x3
    from . import keypoint_ref as KR
    g = torch.Generator().manual_seed(3)
    cin, k, s, m = 24, 5, 7, 3
    w = torch.randn((cin, k, 4, 4), generator=g, dtype=torch.float64)
    b = torch.randn((k,), generator=g, dtype=torch.float64)
    x = torch.randn((m, cin, s, s), generator=g, dtype=torch.float64)
    w3, b3 = deconv4x4s2_as_conv3x3(w, b)
    assert tuple(w3.shape) == (4 * k, cin, 3, 3) and torch.equal(b3, b.repeat(4))
    assert int((w3 != 0).sum()) == 16 * cin * k                       # every tap of the 4x4 kernel lands exactly once
    packed = F.conv2d(x, w3, b3, padding=1).permute(0, 2, 3, 1)       # (M,S,S,4K), the layout cmk_keypoint_decode documents
    want = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    assert float((KR.depth_to_space(packed, k) - want).abs().max()) <= 1e-12
    # ... and on the reference head's own weights, against the fixture's float64 score_lowres maps (stored as fp32)
    from . import keypoint_head_ref as HR
    fx = golden("roi_keypoint")["p3_p5"]
    sd = fx["state_dict"]
    x = fx["pooled"][:fx["score_lowres"].shape[0]].double()
    for i in (1, 2):
        x = F.relu(F.conv2d(x, sd["conv_fcn{}.weight".format(i)].double(), sd["conv_fcn{}.bias".format(i)].double(), padding=1))
    w3, b3 = deconv4x4s2_as_conv3x3(sd["score_lowres.weight"].double(), sd["score_lowres.bias"].double())
    got = KR.depth_to_space(F.conv2d(x, w3, b3, padding=1).permute(0, 2, 3, 1), K)
    assert float((got - fx["score_lowres"].double()).abs().max()) <= 1e-6 * float(fx["score_lowres"].abs().max())
    assert torch.equal(HR.pack(KR.depth_to_space(packed, k)), packed)


def test_refusals_at_construction():
    from centermask2_amd.modeling import build_model
    with pytest.raises(ValueError, match="p2"):                                         # the yaml's backbone builds p3..p7
        build_model(_cfg())
    with pytest.raises(NotImplementedError, match="POOLER_RESOLUTION 17"):
        build_model(_cfg(*P345, "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", 17))
    with pytest.raises(ValueError, match="NUM_KEYPOINTS"):
        build_model(_cfg(*P345, "MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS", 0))
    with pytest.raises(NotImplementedError, match="ROIPool"):
        build_model(_cfg(*P345, "MODEL.ROI_KEYPOINT_HEAD.POOLER_TYPE", "ROIPool"))
    # the builder with p2 takes the default IN_FEATURES
    model = build_model(_cfg("MODEL.BACKBONE.NAME", "build_vovnet_fpn_backbone", "MODEL.ROI_HEADS.IN_FEATURES", ["p3", "p4", "p5"],
                             "MODEL.FCOS.IN_FEATURES", ["p3", "p4", "p5", "p6"], "MODEL.FCOS.FPN_STRIDES", [8, 16, 32, 64],
                             "MODEL.FPN.IN_FEATURES", ["stage2", "stage3", "stage4", "stage5"],
                             "MODEL.VOVNET.OUT_FEATURES", ["stage2", "stage3", "stage4", "stage5"]))
    assert model.roi_heads.keypoint_pooler.scales == (1 / 4, 1 / 8, 1 / 16, 1 / 32)


def _instances(n, hw=(100, 200)):
    g = torch.Generator().manual_seed(n)
    x0 = torch.rand((n, 1), generator=g) * 100
    y0 = torch.rand((n, 1), generator=g) * 50
    boxes = torch.cat([x0, y0, x0 + 5 + torch.rand((n, 1), generator=g) * 90, y0 + 5 + torch.rand((n, 1), generator=g) * 40], 1)
    kp = torch.rand((n, K, 3), generator=g) * torch.tensor([200.0, 100.0, 1.0])
    return Instances(hw, pred_boxes=Boxes(boxes), scores=torch.rand((n,), generator=g), pred_classes=torch.zeros(n, dtype=torch.int64),
                     pred_keypoints=kp)


def test_detector_postprocess_d2_scales_keypoints():
    from centermask2_amd.postprocess import detector_postprocess_d2
    inst = _instances(6)
    inst.pred_boxes.tensor[2] = torch.tensor([300.0, 10.0, 400.0, 20.0])     # outside the image: clipped to empty and dropped
    inst.pred_keypoints[0, 0, :2] = torch.tensor([-7.0, 130.0])              # keypoints are not clipped
    kp0 = inst.pred_keypoints.clone()
    out = detector_postprocess_d2(inst, 250, 300)                             # scale_x 1.5, scale_y 2.5
    keep = [0, 1, 3, 4, 5]
    assert len(out) == 5 and tuple(out.pred_keypoints.shape) == (5, K, 3)
    assert torch.equal(out.pred_keypoints[:, :, 0], kp0[keep][:, :, 0] * 1.5) and torch.equal(out.pred_keypoints[:, :, 1], kp0[keep][:, :, 1] * 2.5)
    assert torch.equal(out.pred_keypoints[:, :, 2], kp0[keep][:, :, 2])
    assert float(out.pred_keypoints[0, 0, 0]) == -10.5 and float(out.pred_keypoints[0, 0, 1]) == 325.0
    assert torch.equal(inst.pred_keypoints, kp0), "the input Instances keep their keypoints"
    empty = detector_postprocess_d2(_instances(0), 250, 300)
    assert tuple(empty.pred_keypoints.shape) == (0, K, 3)


def test_coco_json_keypoints_minus_half():
    from centermask2_amd.wire import instances_to_coco_json
    inst = _instances(3)
    res = instances_to_coco_json(inst, 42)
    assert len(res) == 3
    for i, r in enumerate(res):
        want = inst.pred_keypoints[i].clone()
        want[:, :2] -= 0.5
        assert r["keypoints"] == want.flatten().tolist() and len(r["keypoints"]) == 3 * K
        assert r["keypoints"][2] == float(inst.pred_keypoints[i, 0, 2]) and "segmentation" not in r
    assert float(inst.pred_keypoints[0, 0, 0]) == float(_instances(3).pred_keypoints[0, 0, 0]), "the Instances are not modified"
    inst.remove("pred_keypoints")
    assert "keypoints" not in instances_to_coco_json(inst, 42)[0]


def _padded(n=3, k=5, hw=28, nkp=K, seed=5):
    g = torch.Generator().manual_seed(seed)
    return dict(box=torch.randn((n, k, 4), generator=g), score=torch.rand((n, k), generator=g), mask_scores=torch.rand((n, k), generator=g),
                loc=torch.randn((n, k, 2), generator=g), cls=torch.randint(0, 80, (n, k), generator=g),
                pred_masks=torch.rand((n, k, 1, hw, hw), generator=g), pred_keypoints=torch.randn((n, k, nkp, 3), generator=g),
                counts=torch.tensor([k, 0, 2][:n], dtype=torch.int32))


def test_record_round_trip_with_keypoints_on_cpu():
    from centermask2_amd.dist import pack_records, record_width, unpack_records
    assert record_width(100) == 100 * 793 + 1 and record_width(50, 14) == 50 * 205 + 1            # the defaults are unchanged
    assert record_width(100, 28, K) == 100 * (793 + 3 * K) + 1
    out = _padded()
    rec = pack_records(out)
    n, k = out["score"].shape
    assert rec.shape == (n, record_width(k, 28, K)) and rec.dtype == torch.float32
    assert torch.equal(rec[:, 9 * k + 784 * k: -1], out["pred_keypoints"].reshape(n, -1)) and torch.equal(rec[:, -1], out["counts"].float())
    back = unpack_records(rec, k, 28, K)
    assert list(back) == ["box", "score", "mask_scores", "loc", "cls", "pred_masks", "pred_keypoints", "counts"]
    for name, v in out.items():
        assert torch.equal(back[name], v) and back[name].dtype == v.dtype, name
    # without keypoints: today's record, field for field
    plain = {name: v for name, v in out.items() if name != "pred_keypoints"}
    rec0 = pack_records(plain)
    assert rec0.shape == (n, record_width(k)) and torch.equal(rec0[:, :-1], rec[:, :9 * k + 784 * k])
    assert "pred_keypoints" not in unpack_records(rec0, k)
    with pytest.raises(NotImplementedError, match="keypoint-only"):
        pack_records({name: v for name, v in out.items() if name not in ("pred_masks", "mask_scores")})


def test_pack_records_kp_abi_argument_validation_without_gpu(cmk_lib):
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    names = ("box", "score", "mask_scores", "loc", "cls", "masks", "keypoints", "counts")

    def call(n=2, k=5, hw=28, nkp=K, rec=p, **ptrs):
        args = [ptrs.get(name, p) for name in names]
        rc = cmk_lib.cmk_pack_records_kp(*args, n, k, hw, nkp, rec, None)
        return rc, cmk_lib.cmk_last_error()

    for name in names:
        rc, msg = call(**{name: None})
        assert rc == -1 and b"pack_records_kp: null" in msg, name
    rc, msg = call(rec=None)
    assert rc == -1 and b"null" in msg
    for kw, what in ((dict(n=0), b"bad shape"), (dict(n=65536), b"bad shape"), (dict(k=0), b"bad shape"), (dict(hw=0), b"bad shape"),
                     (dict(nkp=0), b"bad shape"), (dict(nkp=-3), b"bad shape"), (dict(k=1 << 20, hw=1 << 10), b"too wide")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg, (kw, msg)
    assert cmk_lib.cmk_version() == 5
