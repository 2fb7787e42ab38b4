"""-m gpu: test-time augmentation (TEST.AUG).  The three pieces of csrc/resize.hip it adds — the mirrored vertical pass, the box maps, the
mask average — bit for bit against what exists (ops.resize_preprocess_images, torch.flip) and against the numpy restatement
tests/tta_ref.py; GeneralizedRCNNWithTTA end to end against a result composed from GeneralizedRCNN.inference, its detected_instances
hook and the restatement; the degenerate one-scale case against the plain Predictor; and the Predictor's routing."""
import numpy as np
import pytest
import torch

from centermask2_amd import GeneralizedRCNNWithTTA, Predictor, ops, synthetic as S
from centermask2_amd.postprocess import detector_postprocess_d2
from centermask2_amd.structures import Boxes, Instances
from . import resize_ref, tta_ref
from .helpers import build_gpu_model, close, close_abs, match_detections

pytestmark = pytest.mark.gpu

MEAN, STD = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
H0, W0 = 128, 160
MIN_SIZES, MAX_SIZE = (192, 256), 400
SEED = 132               # of the end-to-end image: chosen so that the preconditions the test asserts on its reference hold
MODEL_SEED_PLAIN, SEED_PLAIN = 44, 182         # weights and image of the one-scale test, likewise (see there)


def raw_image(h, w, seed):
    """As tests/test_gpu_predictor.py: a synthetic model input turned back into (h, w, 3) uint8, BGR."""
    x = S.make_synthetic_images(1, h, w, seed0=seed)[0] + torch.tensor(S.PIXEL_MEAN).view(3, 1, 1)
    return x.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# the mirrored front end
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_mirrored_front_end_is_the_flip_of_the_plain_slot(dev, reverse):
    """A 37 x 53 source.  Target widths at the edges of the 256-thread blocks, reached through the shortest-edge rule so that the plain
    slot can be held to ops.resize_preprocess_images; (37, 53) skips both passes.  A divisibility of 48 keeps every canvas wider than
    the image."""
    g = torch.Generator().manual_seed(11)
    src = torch.randint(0, 256, (37, 53, 3), generator=g, dtype=torch.uint8).to(dev)
    rules = [(4000, nw) for nw in (1, 5, 255, 256, 257)] + [(37, 53)]
    shapes = [ops.resize_shortest_edge_shape(37, 53, short, mx) for short, mx in rules]
    assert shapes == [(1, 1), (3, 5), (178, 255), (179, 256), (179, 257), (37, 53)]
    canvases = ops.resize_preprocess_augmented(src, shapes, True, MEAN, STD, 48, reverse_channels=reverse)
    torch.cuda.synchronize()
    for (short, mx), (nh, nw), canvas in zip(rules, shapes, canvases):
        plain, sizes = ops.resize_preprocess_images([src], short, mx, MEAN, STD, 48, reverse_channels=reverse)
        assert sizes == [(nh, nw)] and tuple(canvas.shape) == (2,) + tuple(plain.shape[1:]) and canvas.shape[3] > nw
        assert torch.equal(canvas[0], plain[0]), (nh, nw)
        assert torch.equal(canvas[1][:, :, :nw], torch.flip(canvas[0][:, :, :nw], dims=[2])), (nh, nw)
        assert not canvas[1][:, :, nw:].any() and not canvas[1][:, nh:, :].any(), (nh, nw)
        assert canvas[1][:, :nh, :nw].abs().sum() > 0


@pytest.mark.parametrize("reverse", [False, True])
def test_mirrored_front_end_with_one_pass_skipped(dev, reverse):
    """Shapes the shortest-edge rule cannot give: nh == h (the vertical pass copies) and nw == w (no horizontal pass), against the pure
    resize followed by ops.preprocess_images — the same bits by the contract of cmk_resize_v_preprocess."""
    g = torch.Generator().manual_seed(12)
    src = torch.randint(0, 256, (37, 53, 3), generator=g, dtype=torch.uint8).to(dev)
    shapes = [(37, 60), (50, 53)]
    canvases = ops.resize_preprocess_augmented(src, shapes, [True, False], MEAN, STD, 48, reverse_channels=reverse)
    assert [c.shape[0] for c in canvases] == [2, 1]
    for (nh, nw), canvas in zip(shapes, canvases):
        resized = ops.resize_bilinear_u8(src, nh, nw)
        assert np.array_equal(resized.cpu().numpy(), resize_ref.resize_bilinear_u8(src.cpu().numpy(), nh, nw))
        chw = (resized.flip(2) if reverse else resized).permute(2, 0, 1).contiguous()
        plain, _ = ops.preprocess_images([chw], MEAN, STD, 48)
        assert torch.equal(canvas[0], plain[0]), (nh, nw)
        if canvas.shape[0] == 2:
            assert torch.equal(canvas[1][:, :, :nw], torch.flip(canvas[0][:, :, :nw], dims=[2])) and not canvas[1][:, :, nw:].any()


# ---------------------------------------------------------------------------------------------------------------
# the box maps
# ---------------------------------------------------------------------------------------------------------------
def _detections(rng, augs, k, counts):
    """Random padded detections per augmentation, in its frame, reaching 20 px over every edge."""
    a = len(augs)
    box = np.zeros((a, k, 4), dtype=np.float32)
    for i, (nh, nw, _) in enumerate(augs):
        p = rng.uniform([-20, -20], [nw + 20, nh + 20], size=(k, 2, 2))
        box[i, :, :2], box[i, :, 2:] = p.min(axis=1), p.max(axis=1)
        box[i, :4] = [[-7.5, -3.25, nw + 9.0, nh + 4.5], [-30, 5, -2, 40], [nw + 1, 2, nw + 8, 9], [3, nh + 2, 30, nh + 6]]
    loc = (box[:, :, :2] + box[:, :, 2:]) * np.float32(0.5)
    return dict(box=box, score=rng.random((a, k), dtype=np.float32), cls=rng.integers(0, 80, size=(a, k)).astype(np.int64),
                loc=loc.astype(np.float32), counts=np.asarray(counts, dtype=np.int32))


@pytest.mark.parametrize("min_sizes,flip,counts", [((300,), False, [37]), ((300,), False, [0]), ((200, 333), True, [0, 40, 40, 13]),
                                                  ((200, 333), True, [40, 1, 0, 40])])
def test_box_maps_equal_the_restatement(dev, min_sizes, flip, counts):
    h, w, k = 240, 317, 40
    rng = np.random.default_rng(len(counts) * 100 + sum(counts))
    augs = tta_ref.augmentations(h, w, min_sizes, 500, flip)
    assert len(augs) == len(counts) and (len(augs) == 1 or [f for _, _, f in augs] == [False, True, False, True])
    det = _detections(rng, augs, k, counts)
    want = tta_ref.boxes_to_image(det["box"], det["score"], det["cls"], det["loc"], det["counts"], augs, h, w)
    m = int(sum(counts))
    assert want["box"].shape == (m, 4)
    if m:
        assert want["box"].min() == 0 and (want["box"][:, 0::2].max(), want["box"][:, 1::2].max()) == (w, h)      # the clip was exercised
    cand = ops.tta_boxes_to_image({n: torch.from_numpy(v).to(dev) for n, v in det.items()}, ops.tta_table(augs, h, w, True, dev), h, w)
    torch.cuda.synchronize()
    assert cand["counts"].tolist() == [m] and cand["cap"] == len(augs) * k and cand["cls"].dtype == torch.int32
    for name in ("box", "score", "cls", "loc"):        # bit for bit, and in augmentation order then the detector's order
        assert np.array_equal(cand[name][0, :m].cpu().numpy(), want[name]), name
    # the inverse, on boxes in the image frame
    lo = rng.uniform([0, 0], [w - 1, h - 1], size=(k, 2))
    box = np.concatenate([lo, np.minimum(lo + rng.uniform(0.5, 200, size=(k, 2)), [w, h])], axis=1).astype(np.float32)
    for count in (0, 7, k):
        got, got_counts = ops.tta_boxes_to_aug(torch.from_numpy(box).to(dev), torch.tensor([count], dtype=torch.int32, device=dev),
                                               ops.tta_table(augs, h, w, False, dev))
        torch.cuda.synchronize()
        assert got_counts.tolist() == [count] * len(augs)
        assert np.array_equal(got.cpu().numpy(), tta_ref.boxes_to_aug(box, count, augs, h, w)), count
        assert not got[:, count:].any()


# ---------------------------------------------------------------------------------------------------------------
# the mask average
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [28, 12])
@pytest.mark.parametrize("a", [1, 2, 3, 18])
def test_mask_reduce_equals_the_restatement(dev, a, s):
    k = 100
    rng = np.random.default_rng(a * 100 + s)
    masks = rng.random((a, k, s, s), dtype=np.float32)
    scores = rng.random((a, k), dtype=np.float32)
    flips = np.asarray([i % 2 if i < 4 else (i * 7 // 3) % 2 for i in range(a)], dtype=np.int32)     # mixed, not only alternating
    assert a == 1 or (flips.any() and not flips.all())
    dm, ds, df = torch.from_numpy(masks).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(flips).to(dev)
    for count in (0, 1, 65):
        want_m, want_s = tta_ref.reduce_masks(masks, flips, scores, count)
        got_m, got_s = ops.tta_reduce_masks(dm, df, ds, torch.tensor([count], dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        assert np.array_equal(got_m.cpu().numpy(), want_m) and np.array_equal(got_s.cpu().numpy(), want_s), count
        assert not got_m[count:].any() and not got_s[count:].any()
        only_m, none = ops.tta_reduce_masks(dm, df, None, torch.tensor([count], dtype=torch.int32, device=dev))
        assert none is None and torch.equal(only_m, got_m)
    if a == 18:         # the order is part of the contract: a pairwise tree over the same addends rounds differently
        unflipped = [masks[i, :, :, ::-1] if flips[i] else masks[i] for i in range(a)]
        while len(unflipped) > 1:
            unflipped = [unflipped[i] + unflipped[i + 1] if i + 1 < len(unflipped) else unflipped[i] for i in range(0, len(unflipped), 2)]
        tree = unflipped[0] / np.float32(a)
        want_m, _ = tta_ref.reduce_masks(masks, flips, None, k)
        assert tree.dtype == np.float32 and not np.array_equal(tree, want_m)
        got_m, _ = ops.tta_reduce_masks(dm, df, None, torch.tensor([k], dtype=torch.int32, device=dev))
        assert np.array_equal(got_m.cpu().numpy(), want_m)


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    return build_gpu_model()[0]


def tta_cfg(*extra):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MIN_SIZE_TEST", 256, "INPUT.MAX_SIZE_TEST", MAX_SIZE, "TEST.AUG.MIN_SIZES", MIN_SIZES,
                         "TEST.AUG.MAX_SIZE", MAX_SIZE] + list(extra))
    cfg.freeze()
    return cfg


def pair_ious(box, cls):
    """IoU (float64) of every same-class pair i < j of boxes (n,4); other pairs are -1."""
    b = np.asarray(box, dtype=np.float64)
    iw = np.clip(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), 0, None)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    union = area[:, None] + area[None, :] - iw * ih
    iou = np.where(union > 0, iw * ih / np.where(union > 0, union, 1), 0.0)
    same = (np.asarray(cls)[:, None] == np.asarray(cls)[None, :]) & np.triu(np.ones((len(b), len(b)), dtype=bool), 1)
    return np.where(same, iou, -1.0)


def compose_reference(model, raw, cfg):
    """The TTA result from pieces that exist without it: host resize + flip, GeneralizedRCNN.inference per scale batch, the restatement's
    maps and NMS, the detected_instances hook (CenterROIHeads.forward_with_given_boxes) on the mapped boxes, the restatement's average.
    Returns (soft Instances in the image frame, the candidate set, the kept indices)."""
    dev = model.device
    h, w = int(raw.shape[0]), int(raw.shape[1])
    topk, thr = int(cfg.TEST.DETECTIONS_PER_IMAGE), float(cfg.MODEL.FCOS.NMS_TH)
    augs = tta_ref.augmentations(h, w, MIN_SIZES, MAX_SIZE, True)
    batches = []
    for nh, nw, _ in augs[::2]:
        resized = resize_ref.resize_bilinear_u8(raw.numpy(), nh, nw)
        batches.append([{"image": torch.from_numpy(np.ascontiguousarray(x)).permute(2, 0, 1).float().contiguous()}
                        for x in (resized, resized[:, ::-1])])
    k = int(cfg.MODEL.FCOS.POST_NMS_TOPK_TEST)
    det = dict(box=np.zeros((len(augs), k, 4), np.float32), score=np.zeros((len(augs), k), np.float32), cls=np.zeros((len(augs), k), np.int64),
               loc=np.zeros((len(augs), k, 2), np.float32), counts=np.zeros(len(augs), np.int32))
    with torch.no_grad():
        for i, batch in enumerate(batches):
            for j, r in enumerate(model.inference(batch, do_postprocess=False)):
                a, n = 2 * i + j, len(r)
                assert tuple(r.image_size) == augs[a][:2]
                det["box"][a, :n], det["score"][a, :n] = r.pred_boxes.tensor.cpu().numpy(), r.scores.cpu().numpy()
                det["cls"][a, :n], det["loc"][a, :n], det["counts"][a] = r.pred_classes.cpu().numpy(), r.locations.cpu().numpy(), n
    cand = tta_ref.boxes_to_image(det["box"], det["score"], det["cls"], det["loc"], det["counts"], augs, h, w)
    keep = tta_ref.nms(cand["box"], cand["score"], cand["cls"], thr, topk)
    n = len(keep)
    box, score, cls, loc = cand["box"][keep], cand["score"][keep], cand["cls"][keep].astype(np.int64), cand["loc"][keep]
    res = Instances((h, w), pred_boxes=Boxes(torch.from_numpy(box).to(dev)), scores=torch.from_numpy(score).to(dev),
                    pred_classes=torch.from_numpy(cls).to(dev), locations=torch.from_numpy(loc).to(dev))
    if n:
        in_aug = tta_ref.boxes_to_aug(box, n, augs, h, w)
        masks, mscores = [], []
        with torch.no_grad():
            for i, batch in enumerate(batches):
                given = [Instances(augs[2 * i + j][:2], pred_boxes=Boxes(torch.from_numpy(in_aug[2 * i + j]).to(dev)),
                                   pred_classes=torch.from_numpy(cls).to(dev), scores=torch.from_numpy(score).to(dev)) for j in range(2)]
                for r in model.inference(batch, detected_instances=given, do_postprocess=False):
                    masks.append(r.pred_masks[:, 0].cpu().numpy())
                    mscores.append(r.mask_scores.cpu().numpy())
        red_m, red_s = tta_ref.reduce_masks(np.stack(masks), [f for _, _, f in augs], np.stack(mscores), n)
        res.pred_masks = torch.from_numpy(red_m).to(dev).unsqueeze(1)
        res.mask_scores = torch.from_numpy(red_s).to(dev)
    return res, cand, keep


def test_tta_equals_the_composed_reference(dev, model):
    cfg = tta_cfg()
    raw = raw_image(H0, W0, SEED)
    assert tta_ref.augmentations(H0, W0, MIN_SIZES, MAX_SIZE, True) == [(192, 240, False), (192, 240, True), (256, 320, False), (256, 320, True)]
    ref, cand, keep = compose_reference(model, raw, cfg)
    thr = float(cfg.MODEL.FCOS.NMS_TH)
    # the reference alone: it detects something, and neither the merge nor the matching below sits on a knife's edge
    assert len(keep) > 0, "the reference path alone must detect something"
    ious = pair_ious(cand["box"], cand["cls"])
    near = np.abs(ious - thr) < 1e-3
    assert not near.any(), "same-class candidate pairs with an IoU within 1e-3 of NMS_TH: {}".format(ious[near].tolist())
    ks, kc = cand["score"][keep].astype(np.float64), cand["cls"][keep]
    tie = (np.abs(ks[:, None] - ks[None, :]) <= 1e-4) & (kc[:, None] != kc[None, :])
    assert not tie.any(), "kept scores within 1e-4 of each other across a class boundary: {}".format(ks[tie.any(axis=1)].tolist())

    tta = GeneralizedRCNNWithTTA(cfg, model)
    hwc = raw.to(dev)
    soft = tta.merged_instances(hwc)
    got = tta([{"image": raw.permute(2, 0, 1).contiguous(), "height": H0, "width": W0}])[0]["instances"]
    torch.cuda.synchronize()
    print("TTA end to end: {} candidates, {} kept, {} from the device".format(len(cand["score"]), len(keep), len(soft)))
    assert len(soft) == len(ref) == len(keep)
    p = match_detections(ref.scores, ref.pred_classes, ref.locations, soft.scores, soft.pred_classes, soft.locations, tol=1e-4).to(dev)
    assert torch.equal(soft.pred_classes[p], ref.pred_classes)
    close(soft.pred_boxes.tensor[p], ref.pred_boxes.tensor, 1e-4, "TTA merged boxes (pixels)")
    assert tuple(soft.pred_masks.shape) == (len(ref), 1, 28, 28)
    close_abs(soft.pred_masks[p], ref.pred_masks, 1e-3, "TTA averaged soft masks")
    close_abs(soft.mask_scores[p], ref.mask_scores, 1e-3, "TTA averaged mask_scores")
    want = detector_postprocess_d2(ref, H0, W0)
    assert tuple(got.image_size) == (H0, W0) and len(got) == len(want)
    q = match_detections(want.scores, want.pred_classes, want.locations, got.scores, got.pred_classes, got.locations, tol=1e-4).to(dev)
    assert torch.equal(got.pred_classes[q], want.pred_classes)
    close(got.pred_boxes.tensor[q], want.pred_boxes.tensor, 1e-4, "TTA output boxes (pixels)")
    close_abs(got.mask_scores[q], want.mask_scores, 1e-3, "TTA output mask_scores")
    assert got.pred_masks.dtype == torch.bool and tuple(got.pred_masks.shape) == (len(want), H0, W0) and bool(got.pred_masks.any())


def test_one_scale_without_flip_equals_plain_inference(dev):
    """MIN_SIZES (256,), no flip: the one augmentation is the plain input, so the merge sees the plain detections — mapped to the image
    frame and CLIPPED to it before the NMS, as detectron2's merge does (step 3), and the mask pass sees the clipped boxes.  The plain
    path runs its NMS and its mask head on the unclipped boxes.  Where a box hangs over the image edge the two therefore differ by
    design: two such boxes can overlap more once clipped, so the merge drops one the plain path kept (default synthetic weights, image
    seed 79: 22 of 50 kept, exactly what the float64 NMS of tests/tta_ref.py keeps of the clipped plain boxes), and the mask head pools
    another box (weights seed 2, image seed 85: mask_scores off by up to 1.6e-2 on the five clipped detections, equal elsewhere).
    Equality with plain inference is defined where every plain box lies inside the frame; the weights and the image are chosen so
    that this holds (the first such pair of a scan over weight seeds 0.. and image seeds 77..), and it is asserted first, with the
    check that no same-class pair sits just below NMS_TH.  With this pair 43 of the 50 detections are empty boxes (zero height):
    they pass through the merge like the others and leave in the postprocess of either path, 7 remain."""
    from centermask2_amd.structures import ImageList
    model = build_gpu_model(seed=MODEL_SEED_PLAIN)[0]
    raw = raw_image(H0, W0, SEED_PLAIN)
    plain = Predictor(tta_cfg(), model=model)
    assert plain.tta is None
    ref = plain(raw)["instances"]
    batch, sizes = ops.resize_preprocess_images([raw.to(dev)], 256, MAX_SIZE, model.pixel_mean.flatten().tolist(),
                                                model.pixel_std.flatten().tolist(), model.backbone.size_divisibility)
    with torch.no_grad():
        unclipped = model.inference(ImageList(batch, sizes), do_preprocess=False, do_postprocess=False)[0].pred_boxes.tensor.cpu()
    torch.cuda.synchronize()
    thr = float(plain.cfg.MODEL.FCOS.NMS_TH)
    nonempty = (unclipped[:, 2] > unclipped[:, 0]) & (unclipped[:, 3] > unclipped[:, 1])          # the others leave in the postprocess
    assert len(ref) > 0 and int(nonempty.sum()) == len(ref) and sizes == [(256, 320)]
    assert float(unclipped.min()) >= 0 and float(unclipped[:, 0::2].max()) <= 320 and float(unclipped[:, 1::2].max()) <= 256, \
        "a plain box hangs over the image edge: the clip of the merge would change it"
    ious = pair_ious(ref.pred_boxes.tensor.cpu().numpy(), ref.pred_classes.cpu().numpy())
    edge = ious > thr - 1e-3
    assert not edge.any(), "plain same-class pairs the second NMS could drop: {}".format(ious[edge].tolist())
    tta = GeneralizedRCNNWithTTA(tta_cfg("TEST.AUG.MIN_SIZES", (256,), "TEST.AUG.FLIP", False), model)
    got = tta([{"image": raw.permute(2, 0, 1).contiguous()}])[0]["instances"]
    torch.cuda.synchronize()
    print("one-scale TTA: {} plain detections, {} from TTA, largest same-class IoU {:.4f}".format(len(ref), len(got), float(ious.max())))
    assert tuple(got.image_size) == (H0, W0) and len(got) == len(ref)
    assert torch.equal(got.pred_classes, ref.pred_classes) and torch.equal(got.scores, ref.scores)        # scores pass through untouched
    close(got.pred_boxes.tensor, ref.pred_boxes.tensor, 1e-4, "one-scale TTA boxes (pixels)")
    close_abs(got.mask_scores, ref.mask_scores, 1e-3, "one-scale TTA mask_scores")
    assert got.pred_masks.dtype == torch.bool and tuple(got.pred_masks.shape) == (len(ref), H0, W0)


def test_predictor_routes_through_tta_when_enabled(dev, model):
    cfg = tta_cfg("TEST.AUG.ENABLED", True)
    pred = Predictor(cfg, model=model)
    assert isinstance(pred.tta, GeneralizedRCNNWithTTA)
    raws = [raw_image(H0, W0, SEED), raw_image(96, 176, 79)]
    direct = GeneralizedRCNNWithTTA(cfg, model)([{"image": raws[0].permute(2, 0, 1).contiguous()}])[0]["instances"]
    one = pred(raws[0])["instances"]
    both = pred.predict_batch(raws)
    torch.cuda.synchronize()
    assert len(direct) > 0 and len(both) == 2
    for got in (one, both[0]["instances"]):
        assert tuple(got.image_size) == (H0, W0) and len(got) == len(direct)
        for name in ("scores", "pred_classes", "locations", "mask_scores", "pred_masks"):
            assert torch.equal(got.get(name), direct.get(name)), name
        assert torch.equal(got.pred_boxes.tensor, direct.pred_boxes.tensor)
    second = both[1]["instances"]
    assert tuple(second.image_size) == (96, 176) and tuple(second.pred_masks.shape) == (len(second), 96, 176)
