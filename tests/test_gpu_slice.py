"""-m gpu: sliced inference (TEST.SLICE).  The map kernel of csrc/slice/slice.hip bit for bit against the numpy restatement
tests/slice_ref.py; the metric NMS (cmk_nms_topk_metric) against the restatement's float64 NMS and, with metric 0, against cmk_nms_topk;
SlicedInference end to end against a result composed from ops.resize_preprocess_images, GeneralizedRCNN.inference and the restatement;
the one-tile case against the plain Predictor; a planted duplicate through the merge; and the Predictor's routing."""
import numpy as np
import pytest
import torch

from centermask2_amd import Predictor, SlicedInference, ops, synthetic as S
from centermask2_amd.postprocess import detector_postprocess_d2
from centermask2_amd.structures import ImageList
from . import slice_ref
from .helpers import build_gpu_model, close

pytestmark = pytest.mark.gpu

H0, W0 = 300, 420
TILE, OVERLAP = (160, 200), 0.25
MIN_SIZE, MAX_SIZE = 192, 333
SEED = 155               # of the end-to-end image: of image seeds 132 and 140..174 the one whose merge decisions lie farthest (2.0e-2) from MATCH_THRESH
MODEL_SEED_PLAIN, SEED_PLAIN = 44, 182         # weights and image of the one-tile test: those of the one-scale test of tests/test_gpu_tta.py


def raw_image(h, w, seed):
    """As tests/test_gpu_predictor.py: a synthetic model input turned back into (h, w, 3) uint8, BGR."""
    x = S.make_synthetic_images(1, h, w, seed0=seed)[0] + torch.tensor(S.PIXEL_MEAN).view(3, 1, 1)
    return x.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def slice_cfg(*extra):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MIN_SIZE_TEST", MIN_SIZE, "INPUT.MAX_SIZE_TEST", MAX_SIZE, "TEST.SLICE.TILE", TILE,
                         "TEST.SLICE.OVERLAP", OVERLAP, "TEST.SLICE.BATCH", 4] + list(extra))
    cfg.freeze()
    return cfg


@pytest.fixture(scope="module")
def model(dev):
    return build_gpu_model()[0]


# ---------------------------------------------------------------------------------------------------------------
# 1. the map kernel
# ---------------------------------------------------------------------------------------------------------------
def _detections(rng, pss, k, counts):
    """Random padded detections per pass, in the frame of the resized pass, reaching 20 px over every edge; NaN from the count on."""
    a = len(pss)
    box = np.zeros((a, k, 4), dtype=np.float32)
    for i, (_, _, _, _, nh, nw) in enumerate(pss):
        p = rng.uniform([-20, -20], [nw + 20, nh + 20], size=(k, 2, 2))
        box[i, :, :2], box[i, :, 2:] = p.min(axis=1), p.max(axis=1)
        box[i, :4] = [[-7.5, -3.25, nw + 9.0, nh + 4.5], [-30, 5, -2, 40], [nw + 1, 2, nw + 8, 9], [3, nh + 2, 30, nh + 6]]
    loc = ((box[:, :, :2] + box[:, :, 2:]) * np.float32(0.5)).astype(np.float32)
    score = rng.random((a, k), dtype=np.float32)
    cls = rng.integers(0, 80, size=(a, k)).astype(np.int64)
    for i, c in enumerate(counts):
        n = min(max(c, 0), k)
        box[i, n:], loc[i, n:], score[i, n:] = np.nan, np.nan, np.nan
        cls[i, n:] = 1 << 40
    return dict(box=box, score=score, cls=cls, loc=loc, counts=np.asarray(counts, dtype=np.int32))


@pytest.mark.parametrize("full", [False, True])
def test_map_kernel_equals_the_restatement(dev, full):
    k = 40
    pss = slice_ref.passes(H0, W0, TILE[0], TILE[1], OVERLAP, MIN_SIZE, MAX_SIZE, full)
    assert len(pss) == 9 + full and pss[8][:2] == (140, 220) and all(p[2:] == (160, 200, 192, 240) for p in pss[:9])
    counts = [0, k, 57, 13, 1, k, 0, 39, 100] + ([25] if full else [])
    rng = np.random.default_rng(700 + full)
    det = _detections(rng, pss, k, counts)
    want = slice_ref.boxes_to_image(det["box"], det["score"], det["cls"], det["loc"], det["counts"], pss)
    m = sum(min(c, k) for c in counts)
    assert want["box"].shape == (m, 4) and np.isfinite(want["box"]).all()
    starts = np.cumsum([0] + [min(c, k) for c in counts])
    for i, (y0, x0, th, tw, _, _) in enumerate(pss):          # the clip to the pass's own window was exercised, on every side
        if counts[i] >= 4:
            b = want["box"][starts[i]:starts[i] + 4]
            assert (b[:, 0::2].min(), b[:, 1::2].min(), b[:, 0::2].max(), b[:, 1::2].max()) == (x0, y0, x0 + tw, y0 + th)
    table = ops.slice_table(pss, dev)
    assert np.array_equal(table.cpu().numpy(), slice_ref.table(pss))
    cand = ops.slice_boxes_to_image({n: torch.from_numpy(v).to(dev) for n, v in det.items()}, table, H0, W0)
    torch.cuda.synchronize()
    assert cand["counts"].tolist() == [m] and cand["cap"] == len(pss) * k and cand["cls"].dtype == torch.int32 and cand["src"].dtype == torch.int32
    for name in ("box", "score", "cls", "loc"):        # bit for bit, in pass order then the detector's order; nothing of the NaN rows
        got = cand[name][0, :m].cpu().numpy()
        assert np.array_equal(got, want[name]), name
    assert np.array_equal(cand["src"][:m].cpu().numpy(), want["src"])
    assert want["src"][:k].tolist() == list(range(k, 2 * k)) and want["src"][k] == 2 * k          # pass 0 is empty; pass 2 clamps to K


# ---------------------------------------------------------------------------------------------------------------
# 2. the metric NMS
# ---------------------------------------------------------------------------------------------------------------
def _nms_candidates(count, thr, seed):
    """`count` boxes of three classes on a 1/4-pixel lattice inside [0, 500): clusters of jittered copies, boxes nested in them, boxes of
    zero area; scores from 50 values, so most are tied.  A box that is part of a same-class pair whose IoU or IoS (float64) lies within
    2e-3 of thr is drawn again, until none is left: the decisions of an fp32 kernel and of the float64 restatement cannot differ."""
    rng = np.random.default_rng(seed)

    def draw(n):
        c = rng.uniform(40, 440, size=(max(1, count // 12), 2))
        ctr = c[rng.integers(0, len(c), size=n)] + rng.normal(0, 6, size=(n, 2))
        half = rng.choice([3.0, 8.0, 20.0, 35.0], size=(n, 2)) * rng.uniform(0.7, 1.3, size=(n, 2))
        b = np.concatenate([ctr - half, ctr + half], axis=1)
        return (np.round(np.clip(b, 0, 499.75) * 4) / 4).astype(np.float32)

    box = draw(count)
    cls = rng.integers(0, 3, size=count).astype(np.int32)
    score = (rng.integers(1, 51, size=count) / 50).astype(np.float32)
    flat = rng.random(count) < 0.03
    box[flat, 2] = box[flat, 0]                               # zero area
    for _ in range(200):
        near = np.zeros(count, dtype=bool)
        for metric in ("iou", "ios"):
            m = slice_ref.pair_metric(box, cls, metric)
            near |= (np.abs(m - thr) < 2e-3).any(axis=0)
        if not near.any():
            break
        box[near] = draw(int(near.sum()))
    return box, score, cls


def _run_nms(dev, box, score, cls, loc, thr, topk, metric=None, entry=None):
    cand = dict(box=torch.from_numpy(box)[None].to(dev), score=torch.from_numpy(score)[None].to(dev), cls=torch.from_numpy(cls)[None].to(dev),
                loc=torch.from_numpy(loc)[None].to(dev), counts=torch.tensor([len(score)], dtype=torch.int32, device=dev))
    if entry is None:
        out = ops.nms_topk(cand, thr, topk, metric=metric)
    else:                                                     # a C entry itself: cmk_nms_topk, or cmk_nms_topk_metric with metric 0
        from centermask2_amd import _lib
        n, cap = cand["score"].shape
        out = dict(box=torch.empty((n, topk, 4), device=dev), score=torch.empty((n, topk), device=dev),
                   cls=torch.empty((n, topk), dtype=torch.int64, device=dev), loc=torch.empty((n, topk, 2), device=dev),
                   idx=torch.empty((n, topk), dtype=torch.int32, device=dev), counts=torch.empty((n,), dtype=torch.int32, device=dev))
        ws = torch.empty((n, 4, cap), dtype=torch.int32, device=dev)
        head = (cand["box"].data_ptr(), cand["score"].data_ptr(), cand["cls"].data_ptr(), cand["loc"].data_ptr(), cand["counts"].data_ptr(), n, cap,
                float(thr))
        tail = (topk, out["box"].data_ptr(), out["score"].data_ptr(), out["cls"].data_ptr(), out["loc"].data_ptr(), out["idx"].data_ptr(),
                out["counts"].data_ptr(), ws.data_ptr(), ops._stream())
        _lib.check(getattr(_lib.load(), entry)(*(head + ((0,) if entry == "cmk_nms_topk_metric" else ()) + tail)), entry)
    torch.cuda.synchronize()
    return {k: v[0].cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("count", [1, 1024 + 1, 10 * 40])
def test_metric_nms_equals_the_restatement(dev, count):
    thr, topk = 0.5, 100
    box, score, cls = _nms_candidates(count, thr, seed=count)
    loc = ((box[:, :2] + box[:, 2:]) * np.float32(0.5)).astype(np.float32)
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    if count > 1:
        assert len(set(cls.tolist())) == 3 and len(set(score.tolist())) < count // 2 and (area == 0).any()
    keeps = {}
    for metric in ("ios", "iou"):
        m = slice_ref.pair_metric(box, cls, metric)
        near = np.abs(m - thr) < 1e-3
        assert not near.any(), "same-class pairs with {} within 1e-3 of the threshold: {}".format(metric, m[near].tolist())
        keep = keeps[metric] = slice_ref.nms(box, score, cls, thr, topk, metric)
        got = _run_nms(dev, box, score, cls, loc, thr, topk, metric=metric)
        n = len(keep)
        print("metric NMS {}: {} candidates, {} kept".format(metric, count, n))
        assert got["counts"] == n and got["idx"][:n].tolist() == keep, metric
        assert np.array_equal(got["box"][:n], box[keep]) and np.array_equal(got["score"][:n], score[keep]), metric
        assert np.array_equal(got["cls"][:n], cls[keep].astype(np.int64)) and np.array_equal(got["loc"][:n], loc[keep]), metric
        assert (got["idx"][n:] == -1).all() and not got["box"][n:].any() and not got["score"][n:].any(), metric
    if count > 1:
        assert keeps["ios"] != keeps["iou"] and len(keeps["ios"]) <= len(keeps["iou"])            # the metric matters on these inputs
        assert any(area[i] == 0 for i in keeps["ios"])                                              # a zero area is not suppressed
    old = _run_nms(dev, box, score, cls, loc, thr, topk, entry="cmk_nms_topk")
    new = _run_nms(dev, box, score, cls, loc, thr, topk, entry="cmk_nms_topk_metric")
    wrapped = _run_nms(dev, box, score, cls, loc, thr, topk, metric="iou")
    for name in old:
        assert np.array_equal(old[name], new[name]) and np.array_equal(old[name], wrapped[name]), name


# ---------------------------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------------------------
def compose_reference(model, raw, cfg):
    """The sliced result from pieces that exist without it: the same crops through ops.resize_preprocess_images in the same chunks,
    GeneralizedRCNN.inference per chunk, the restatement's map and NMS, a host gather of the masks and the mask scores.  Returns
    (dict of numpy fields in the image frame, the candidate set, the kept indices)."""
    dev = model.device
    h, w = int(raw.shape[0]), int(raw.shape[1])
    sl = cfg.TEST.SLICE
    pss = slice_ref.passes(h, w, sl.TILE[0], sl.TILE[1], sl.OVERLAP, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, sl.FULL_IMAGE)
    tiles = pss[:-1] if sl.FULL_IMAGE else pss
    img = raw.to(dev)
    crops = [img[y0:y0 + th, x0:x0 + tw].contiguous() for y0, x0, th, tw, _, _ in tiles]
    chunks = [crops[i:i + sl.BATCH] for i in range(0, len(crops), sl.BATCH)] + ([[img]] if sl.FULL_IMAGE else [])
    k = int(cfg.MODEL.FCOS.POST_NMS_TOPK_TEST)
    a_n = len(pss)
    det = dict(box=np.zeros((a_n, k, 4), np.float32), score=np.zeros((a_n, k), np.float32), cls=np.zeros((a_n, k), np.int64),
               loc=np.zeros((a_n, k, 2), np.float32), counts=np.zeros(a_n, np.int32))
    masks, mscores = None, np.zeros((a_n * k,), np.float32)
    a = 0
    with torch.no_grad():
        for chunk in chunks:
            batch, sizes = ops.resize_preprocess_images(chunk, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, model.pixel_mean.flatten().tolist(),
                                                        model.pixel_std.flatten().tolist(), model.backbone.size_divisibility)
            for r, size in zip(model.inference(ImageList(batch, sizes), do_preprocess=False, do_postprocess=False), sizes):
                n = len(r)
                assert tuple(size) == pss[a][4:] and n <= k
                det["box"][a, :n], det["score"][a, :n] = r.pred_boxes.tensor.cpu().numpy(), r.scores.cpu().numpy()
                det["cls"][a, :n], det["loc"][a, :n], det["counts"][a] = r.pred_classes.cpu().numpy(), r.locations.cpu().numpy(), n
                pm = r.pred_masks.cpu().numpy()
                if masks is None:
                    masks = np.zeros((a_n * k,) + pm.shape[1:], np.float32)
                masks[a * k:a * k + n], mscores[a * k:a * k + n] = pm, r.mask_scores.cpu().numpy()
                a += 1
    assert a == a_n
    cand = slice_ref.boxes_to_image(det["box"], det["score"], det["cls"], det["loc"], det["counts"], pss)
    keep = slice_ref.nms(cand["box"], cand["score"], cand["cls"], float(sl.MATCH_THRESH), int(cfg.TEST.DETECTIONS_PER_IMAGE), sl.MATCH_METRIC.lower())
    src = cand["src"][keep]
    ref = dict(box=cand["box"][keep], score=cand["score"][keep], cls=cand["cls"][keep].astype(np.int64), loc=cand["loc"][keep],
               masks=masks[src], mask_scores=mscores[src])
    return ref, cand, keep, det


def test_sliced_equals_the_composed_reference(dev, model):
    cfg = slice_cfg()
    raw = raw_image(H0, W0, SEED)
    ref, cand, keep, det = compose_reference(model, raw, cfg)
    thr = float(cfg.TEST.SLICE.MATCH_THRESH)
    # the reference alone: it detects something in tiles and in the whole image, the merge drops something, and no decision sits on a knife's edge
    assert len(det["counts"]) == 10 and det["counts"][:9].sum() > 0 and det["counts"][9] > 0
    assert 0 < len(keep) < len(cand["score"]), "the merge must keep something and drop something"
    # (the random weights put boxes of a few shapes on the FCOS lattice: of the thousands of same-class pairs some always sit at the
    # threshold, so the margin is asked of the decisions the greedy scan takes, which is what can differ, not of every pair)
    again, margin = slice_ref.nms_margin(cand["box"], cand["score"], cand["cls"], thr, int(cfg.TEST.DETECTIONS_PER_IMAGE), "ios")
    assert again == keep and margin >= 1e-3, "a decision of the merge lies {:.2e} from MATCH_THRESH".format(margin)

    sliced = SlicedInference(cfg, model)
    soft = sliced.merged_instances(raw.to(dev))
    got = sliced([{"image": raw.permute(2, 0, 1).contiguous(), "height": H0, "width": W0}])[0]["instances"]
    torch.cuda.synchronize()
    print("sliced end to end: {} candidates of {} passes, {} kept, {} from the device".format(len(cand["score"]), len(det["counts"]), len(keep), len(soft)))
    assert tuple(soft.image_size) == (H0, W0) and len(soft) == len(keep)
    assert np.array_equal(soft.pred_boxes.tensor.cpu().numpy(), ref["box"])
    assert np.array_equal(soft.scores.cpu().numpy(), ref["score"]) and np.array_equal(soft.pred_classes.cpu().numpy(), ref["cls"])
    assert soft.pred_classes.dtype == torch.int64 and np.array_equal(soft.locations.cpu().numpy(), ref["loc"])
    assert tuple(soft.pred_masks.shape) == (len(keep), 1, 28, 28)
    assert np.array_equal(soft.pred_masks.cpu().numpy(), ref["masks"]) and np.array_equal(soft.mask_scores.cpu().numpy(), ref["mask_scores"])
    want = detector_postprocess_d2(soft, H0, W0)
    assert tuple(got.image_size) == (H0, W0) and len(got) == len(want) > 0
    for name in ("scores", "pred_classes", "locations", "mask_scores", "pred_masks"):
        assert torch.equal(got.get(name), want.get(name)), name
    assert torch.equal(got.pred_boxes.tensor, want.pred_boxes.tensor)
    assert got.pred_masks.dtype == torch.bool and tuple(got.pred_masks.shape) == (len(want), H0, W0) and bool(got.pred_masks.any())


# ---------------------------------------------------------------------------------------------------------------
# 4. one tile
# ---------------------------------------------------------------------------------------------------------------
def test_one_tile_without_the_full_image_equals_plain_inference(dev):
    """A tile as large as the image, FULL_IMAGE off, the detector's own metric and threshold: the one pass is the plain input, so the merge
    sees the plain detections -- mapped to the image frame and CLIPPED to it before the NMS.  As in the one-scale test of
    tests/test_gpu_tta.py, whose weights, image and sizes these are, equality with plain inference is defined where every plain box lies
    inside the frame and no same-class pair sits just below the threshold; both are asserted first.  The boxes get the distance that
    test grants, for its reason: the merge scales them into the image frame with one rounded multiplication of its own before the
    postprocess, the plain path scales once.  Scores and mask scores pass through untouched and are equal bit for bit."""
    from centermask2_amd.config import config_path, get_cfg
    h, w = 128, 160

    def cfg_of(*extra):
        cfg = get_cfg()
        cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
        cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MIN_SIZE_TEST", 256, "INPUT.MAX_SIZE_TEST", 400] + list(extra))
        cfg.freeze()
        return cfg

    model = build_gpu_model(seed=MODEL_SEED_PLAIN)[0]
    raw = raw_image(h, w, SEED_PLAIN)
    plain = Predictor(cfg_of(), model=model)
    assert plain.sliced is None and plain.tta is None
    ref = plain(raw)["instances"]
    batch, sizes = ops.resize_preprocess_images([raw.to(dev)], 256, 400, model.pixel_mean.flatten().tolist(), model.pixel_std.flatten().tolist(),
                                                model.backbone.size_divisibility)
    with torch.no_grad():
        unclipped = model.inference(ImageList(batch, sizes), do_preprocess=False, do_postprocess=False)[0].pred_boxes.tensor.cpu()
    torch.cuda.synchronize()
    thr = float(plain.cfg.MODEL.FCOS.NMS_TH)
    nonempty = (unclipped[:, 2] > unclipped[:, 0]) & (unclipped[:, 3] > unclipped[:, 1])          # the others leave in the postprocess
    assert len(ref) > 0 and int(nonempty.sum()) == len(ref) and sizes == [(256, 320)]
    assert float(unclipped.min()) >= 0 and float(unclipped[:, 0::2].max()) <= 320 and float(unclipped[:, 1::2].max()) <= 256, \
        "a plain box hangs over the image edge: the clip of the merge would change it"
    ious = slice_ref.pair_metric(ref.pred_boxes.tensor.cpu().numpy(), ref.pred_classes.cpu().numpy(), "iou")
    edge = ious > thr - 1e-3
    assert not edge.any(), "plain same-class pairs the second NMS could drop: {}".format(ious[edge].tolist())
    sliced = SlicedInference(cfg_of("TEST.SLICE.TILE", (h, w), "TEST.SLICE.FULL_IMAGE", False, "TEST.SLICE.MATCH_METRIC", "IOU",
                                    "TEST.SLICE.MATCH_THRESH", thr), model)
    assert sliced.passes(h, w) == [(0, 0, h, w, 256, 320)]
    got = sliced([{"image": raw.permute(2, 0, 1).contiguous()}])[0]["instances"]
    torch.cuda.synchronize()
    print("one tile: {} plain detections, {} sliced, largest same-class IoU {:.4f}".format(len(ref), len(got), float(ious.max())))
    assert tuple(got.image_size) == (h, w) and len(got) == len(ref)
    assert torch.equal(got.pred_classes, ref.pred_classes) and torch.equal(got.scores, ref.scores)
    assert torch.equal(got.mask_scores, ref.mask_scores)
    close(got.pred_boxes.tensor, ref.pred_boxes.tensor, 1e-4, "one-tile sliced boxes (pixels)")
    assert got.pred_masks.dtype == torch.bool and tuple(got.pred_masks.shape) == (len(ref), h, w)


# ---------------------------------------------------------------------------------------------------------------
# 5. a planted duplicate
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n_want", [("IOS", 3), ("IOU", 4)])
def test_planted_duplicate_is_merged(dev, model, metric, n_want):
    """Detections planted into the padded buffers of the passes of a 300 x 420 image: object O (class 3) lies in the overlap of tiles 0
    and 1 and is found by both and, a pixel off, by the whole-image pass; a box equal to O of class 4; object P (class 5) is found whole
    by tile 5 and, cut at the tile border to 3/8 of its width, by tile 4.  IoS leaves O once (the best score: tile 1's), the class-4
    box and P; IoU at the same threshold cannot tell that the cut box (IoU 0.375) is part of P."""
    sliced = SlicedInference(slice_cfg("TEST.SLICE.MATCH_METRIC", metric), model)
    pss = sliced.passes(H0, W0)
    assert pss == slice_ref.passes(H0, W0, TILE[0], TILE[1], OVERLAP, MIN_SIZE, MAX_SIZE, True)
    assert [p[:2] for p in pss[:2] + pss[4:6]] == [(0, 0), (0, 150), (120, 150), (120, 220)]
    k = 8
    a_n = len(pss)
    O, P, P_cut = (155.0, 20.0, 195.0, 60.0), (320.0, 200.0, 400.0, 260.0), (320.0, 200.0, 350.0, 260.0)

    def into(a, b, shift=0.0):                  # an image-frame box in the frame of resized pass a, in float64
        y0, x0, th, tw, nh, nw = pss[a]
        return [(b[0] - x0 + shift) * nw / tw, (b[1] - y0) * nh / th, (b[2] - x0 + shift) * nw / tw, (b[3] - y0) * nh / th]

    det = dict(box=np.full((a_n, k, 4), np.nan, np.float32), score=np.full((a_n, k), np.nan, np.float32), cls=np.zeros((a_n, k), np.int64),
               loc=np.full((a_n, k, 2), np.nan, np.float32), counts=np.zeros(a_n, np.int32))
    planted = [(0, O, 0.8, 3, 0.0), (1, O, 0.9, 3, 0.0), (9, O, 0.7, 3, 1.0), (9, O, 0.75, 4, 0.0), (5, P, 0.85, 5, 0.0), (4, P_cut, 0.6, 5, 0.0)]
    for a, b, s, c, shift in planted:
        j = det["counts"][a]
        det["box"][a, j], det["score"][a, j], det["cls"][a, j] = into(a, b, shift), s, c
        det["loc"][a, j] = [(det["box"][a, j, 0] + det["box"][a, j, 2]) / 2, (det["box"][a, j, 1] + det["box"][a, j, 3]) / 2]
        det["counts"][a] += 1
    table = sliced._geometry(H0, W0, dev)[1]
    cand, merged = sliced.merge({n: torch.from_numpy(v).to(dev) for n, v in det.items()}, table, H0, W0)
    torch.cuda.synchronize()
    assert cand["counts"].tolist() == [6] and cand["src"][:6].tolist() == [0, k, 4 * k, 5 * k, 9 * k, 9 * k + 1]
    n = int(merged["counts"][0])
    box, score, cls = merged["box"][0, :n].cpu().numpy(), merged["score"][0, :n].cpu().numpy(), merged["cls"][0, :n].tolist()
    src = cand["src"][merged["idx"][0, :n].long()].tolist()
    assert n == n_want
    assert cls[:3] == [3, 5, 4] and np.array_equal(score[:3], np.array([0.9, 0.85, 0.75], np.float32)) and src[:3] == [k, 5 * k, 9 * k + 1]
    assert np.abs(box[0] - O).max() < 1e-3 and np.abs(box[1] - P).max() < 1e-3 and np.abs(box[2] - O).max() < 1e-3
    assert cls.count(3) == 1                                                                        # O once, whatever the metric
    if metric == "IOU":
        assert cls[3] == 5 and src[3] == 4 * k and np.abs(box[3] - P_cut).max() < 1e-3


# ---------------------------------------------------------------------------------------------------------------
# 6. the Predictor
# ---------------------------------------------------------------------------------------------------------------
def test_predictor_routes_through_the_sliced_path_when_enabled(dev, model):
    cfg = slice_cfg("TEST.SLICE.ENABLED", True)
    pred = Predictor(cfg, model=model)
    assert isinstance(pred.sliced, SlicedInference) and pred.tta is None
    raws = [raw_image(H0, W0, SEED), raw_image(96, 176, 79)]
    direct = SlicedInference(cfg, model).inference_one_image(raws[0].to(dev), H0, W0)
    one = pred(raws[0])["instances"]
    both = pred.predict_batch(raws)
    torch.cuda.synchronize()
    assert len(direct) > 0 and len(both) == 2
    for got in (one, both[0]["instances"]):
        assert tuple(got.image_size) == (H0, W0) and len(got) == len(direct)
        for name in ("scores", "pred_classes", "locations", "mask_scores", "pred_masks"):
            assert torch.equal(got.get(name), direct.get(name)), name
        assert torch.equal(got.pred_boxes.tensor, direct.pred_boxes.tensor)
    second = both[1]["instances"]                                                                   # smaller than the tile: one tile and the image
    assert tuple(second.image_size) == (96, 176) and tuple(second.pred_masks.shape) == (len(second), 96, 176)
