"""No GPU: evaluation.COCOEvaluator and coco_eval.py (the restatement of pycocotools' COCOeval and rleFrPoly) on hand-built datasets
whose answers are worked out in the comments, against evaluation.average_precision where the two protocols coincide, and the polygon
rasteriser against properties of rectangles and a triangle.  These pin our own restatement, not pycocotools (absent here)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from centermask2_amd import coco_eval, evaluation, wire
from centermask2_amd.evaluation import COCOEvaluator
from tests import coco_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = dict(abs=1e-9)             # 1 / (1 + eps) stands for a precision of 1: sums of float64 rationals, not exact integers


def run(ds, per_image, **kw):
    ev = COCOEvaluator(ds, **kw)
    ev.process([{"image_id": i} for i, _ in per_image], [{"instances": inst} for _, inst in per_image])
    return ev.evaluate()


def test_perfect_detections_score_100_where_there_is_ground_truth():
    # a small (10x10 = 100 <= 32^2) and a large (100x100 = 10000 > 96^2) ground truth, no medium one: every detection is the ground truth
    # itself, so every precision and recall cell with ground truth is 1 and the medium cells stay -1 -> NaN
    boxes = [(5, 5, 15, 15), (60, 60, 160, 160)]
    ds = C.dataset({1: (200, 200)}, [C.ann(k + 1, 1, 1, b) for k, b in enumerate(boxes)])
    res = run(ds, [(1, C.instances(200, 200, boxes, [0.9, 0.8]))])
    for task in ("bbox", "segm"):
        r = res[task]
        for k in ("AP", "AP50", "AP75", "APs", "APl", "AR10", "AR100", "ARs", "ARl"):
            assert r[k] == pytest.approx(100.0, **EXACT), (task, k)
        assert r["AR1"] == pytest.approx(50.0, **EXACT)       # one detection per image recalls one of the two
        assert math.isnan(r["APm"]) and math.isnan(r["ARm"])
        assert not any(k.startswith("AP-") for k in r)         # one category: no per-category AP


def test_fp_above_two_tps_gives_two_thirds_at_every_threshold():
    # scores FP > TP > TP, all IoUs 1: cumulative (tp, fp) = (0,1), (1,1), (2,1): precision 0, 1/2, 2/3, recall 0, 1/2, 1.  The
    # right-to-left maximum makes the envelope 2/3 everywhere, so all 101 recall points read 2/3 at each of the ten thresholds.
    gts = [(10, 10, 50, 50), (100, 100, 150, 160)]
    ds = C.dataset({1: (200, 200)}, [C.ann(k + 1, 1, 1, b) for k, b in enumerate(gts)])
    res = run(ds, [(1, C.instances(200, 200, [(60, 5, 90, 30)] + gts, [0.9, 0.8, 0.7]))])
    for task in ("bbox", "segm"):
        assert res[task]["AP"] == pytest.approx(200.0 / 3, **EXACT)
        assert res[task]["AP50"] == pytest.approx(200.0 / 3, **EXACT) and res[task]["AP75"] == pytest.approx(200.0 / 3, **EXACT)
        assert res[task]["AR100"] == pytest.approx(100.0, **EXACT)


def _crowd_case(iscrowd, n_inside=1):
    h = w = 200
    region = C.rect_mask(h, w, 100, 100, 150, 150)
    anns = [C.ann(1, 1, 1, (10, 10, 30, 30)),
            C.ann(2, 1, 1, (100, 100, 150, 150), iscrowd=iscrowd, seg={"size": [h, w], "counts": wire.rle_counts(region)})]
    inside = [(110, 110, 120, 120), (125, 125, 140, 135)][:n_inside]
    inst = C.instances(h, w, inside + [(10, 10, 30, 30)], [0.95, 0.93][:n_inside] + [0.9])
    return C.dataset({1: (h, w)}, anns), [(1, inst)]


def test_detection_inside_a_crowd_region_is_ignored_and_a_false_positive_without_iscrowd():
    # crowd: IoU = inter / a_dt = 1 for the detection inside, it matches the crowd and is ignored; the other detection is the only
    # counted one and correct: AP 100.
    res = run(*_crowd_case(1))
    assert res["bbox"]["AP"] == pytest.approx(100.0, **EXACT) and res["segm"]["AP"] == pytest.approx(100.0, **EXACT)
    # the same region as an ordinary ground truth: IoU = 100 / 2500 = 0.04, the top-scored detection is a false positive and the
    # region is missed.  (tp, fp) = (0,1), (1,1) of 2 ground truths: precision 0, 1/2 -> envelope 1/2 up to recall 1/2, which are
    # the 51 recall points 0 .. 0.5; beyond, 0.  AP = 51 * 0.5 / 101.
    res = run(*_crowd_case(0))
    want = 100.0 * 51 * 0.5 / 101
    assert res["bbox"]["AP"] == pytest.approx(want, **EXACT) and res["segm"]["AP"] == pytest.approx(want, **EXACT)


def test_a_crowd_absorbs_several_detections():
    ds, per_image = _crowd_case(1, n_inside=2)
    res = run(ds, per_image)
    assert res["bbox"]["AP"] == pytest.approx(100.0, **EXACT) and res["segm"]["AP"] == pytest.approx(100.0, **EXACT)
    # the protocol itself: both detections inside match the (single) crowd column at every threshold and are ignored
    ious = np.array([[0.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
    e = coco_eval.evaluate_img(ious, [0.95, 0.93, 0.9], [100, 150, 400], [400, 2500], [False, True], [False, True], coco_eval.AREA_RNG[0], 100)
    assert e["dtm"].all() and e["dt_ig"][:, :2].all() and not e["dt_ig"][:, 2].any()


def test_area_ranges_ignore_ground_truth_outside():
    # one ground truth of area 20^2 = 400 <= 32^2 with its perfect detection: small and all see it, medium and large have no
    # non-ignored ground truth (-1 -> NaN); the detection, matched to an ignored ground truth there, is ignored too
    ds = C.dataset({1: (100, 100)}, [C.ann(1, 1, 1, (30, 30, 50, 50))])
    res = run(ds, [(1, C.instances(100, 100, [(30, 30, 50, 50)], [0.9]))])
    for task in ("bbox", "segm"):
        r = res[task]
        assert r["AP"] == pytest.approx(100.0, **EXACT) and r["APs"] == pytest.approx(100.0, **EXACT) and r["ARs"] == pytest.approx(100.0, **EXACT)
        assert all(math.isnan(r[k]) for k in ("APm", "APl", "ARm", "ARl"))


def test_max_dets_limits_recall():
    # two ground truths, two correct detections in one image: with one detection per image one of two is found
    gts = [(10, 10, 50, 50), (100, 100, 150, 160)]
    ds = C.dataset({1: (200, 200)}, [C.ann(k + 1, 1, 1, b) for k, b in enumerate(gts)])
    res = run(ds, [(1, C.instances(200, 200, gts, [0.9, 0.8]))])
    for task in ("bbox", "segm"):
        assert res[task]["AR1"] == pytest.approx(50.0, **EXACT) and res[task]["AR10"] == pytest.approx(100.0, **EXACT)
        assert res[task]["AR100"] == pytest.approx(100.0, **EXACT)


def test_segm_is_ranked_by_mask_score_and_bbox_by_score():
    # one ground truth, A correct and B elsewhere.  Ranked B, A: (tp, fp) = (0,1), (1,1), precision 0, 1/2 -> envelope 1/2 at every
    # recall point: AP 50.  Ranked A, B: AP 100.
    gt = (10, 10, 50, 50)
    ds = C.dataset({1: (100, 100)}, [C.ann(1, 1, 1, gt)])
    boxes = [gt, (60, 60, 90, 90)]
    res = run(ds, [(1, C.instances(100, 100, boxes, [0.5, 0.9], mask_scores=[0.9, 0.5]))])
    assert res["bbox"]["AP"] == pytest.approx(50.0, **EXACT) and res["segm"]["AP"] == pytest.approx(100.0, **EXACT)
    res = run(ds, [(1, C.instances(100, 100, boxes, [0.9, 0.5], mask_scores=[0.5, 0.9]))])
    assert res["bbox"]["AP"] == pytest.approx(100.0, **EXACT) and res["segm"]["AP"] == pytest.approx(50.0, **EXACT)


def test_iou_exactly_on_a_threshold_matches():
    # 40x40 against 40x30 inside it: 1200 / 1600 = 0.75 exactly.  It matches at 0.5 .. 0.75 (6 thresholds) and not above: AP 60.
    assert np.linspace(.5, .95, 10)[5] == 0.75 and coco_eval.IOU_THRS[5] == 0.75
    assert coco_eval.box_iou_xywh([[0, 0, 40, 30]], [[0, 0, 40, 40]], [False])[0, 0] == 0.75
    ds = C.dataset({1: (100, 100)}, [C.ann(1, 1, 1, (0, 0, 40, 40))])
    res = run(ds, [(1, C.instances(100, 100, [(0, 0, 40, 30)], [0.9]))])
    for task in ("bbox", "segm"):
        assert res[task]["AP75"] == pytest.approx(100.0, **EXACT) and res[task]["AP"] == pytest.approx(60.0, **EXACT)


# ---- agreement with evaluation.average_precision ------------------------------------------------------------------------------------

def _random_case(seed, n_img=4, h=48, w=64):
    rng = np.random.RandomState(seed)
    cats = (1, 2, 3)
    sizes, anns, per_image, preds, gts, aid = {}, [], [], [], [], 1

    def box():
        x0, y0 = rng.uniform(0, w - 14), rng.uniform(0, h - 14)
        return [x0, y0, x0 + rng.uniform(6, min(30, w - x0)), y0 + rng.uniform(6, min(30, h - y0))]

    def mask_of(b):
        return C.rect_mask(h, w, int(round(b[0])), int(round(b[1])), int(round(b[2])), int(round(b[3])))

    def jitter(b):
        d = b + rng.uniform(-4, 4, 4)
        x0, y0 = np.clip(d[0], 0, w - 8), np.clip(d[1], 0, h - 8)
        return [x0, y0, np.clip(d[2], x0 + 4, w), np.clip(d[3], y0 + 4, h)]

    for img in range(1, n_img + 1):
        sizes[img] = (h, w)
        g_boxes = np.array([box() for _ in range(rng.randint(3, 7))], dtype=np.float32)
        g_cls = rng.randint(0, 3, len(g_boxes))
        g_masks = np.stack([mask_of(b) for b in g_boxes])
        for b, c, m in zip(g_boxes, g_cls, g_masks):
            anns.append({"id": aid, "image_id": img, "category_id": cats[c], "iscrowd": 0, "area": float(m.sum()),
                         "bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])],
                         "segmentation": {"size": [h, w], "counts": wire.rle_counts(m)}})
            aid += 1
        d_boxes = [jitter(b) for b in g_boxes for _ in range(2)] + [box() for _ in range(4)]
        d_boxes = np.array(d_boxes, dtype=np.float32)
        d_cls = np.concatenate([np.repeat(g_cls, 2), rng.randint(0, 3, 4)])
        d_masks = np.stack([mask_of(b) for b in d_boxes])
        assert d_masks.reshape(len(d_masks), -1).any(1).all() and len(d_boxes) <= 100
        scores, mscores = rng.rand(len(d_boxes)).astype(np.float32), rng.rand(len(d_boxes)).astype(np.float32)
        inst = C.instances(h, w, d_boxes.tolist(), scores.tolist(), d_cls.tolist(), d_masks, mscores.tolist())
        per_image.append((img, inst))
        preds.append({"boxes": torch.from_numpy(d_boxes), "classes": torch.from_numpy(d_cls), "scores": torch.from_numpy(scores),
                      "masks": torch.from_numpy(d_masks), "mask_scores": torch.from_numpy(mscores)})
        gts.append({"boxes": torch.from_numpy(g_boxes), "classes": torch.from_numpy(g_cls), "masks": torch.from_numpy(g_masks)})
    return C.dataset(sizes, anns, cats), per_image, preds, gts


def _xywh(b):
    b = np.asarray(b, dtype=np.float64)
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)


@pytest.mark.parametrize("seed", [8, 17, 21])      # seeds whose IoUs keep clear of the thresholds (asserted below)
def test_agrees_with_average_precision_on_crowd_free_data(seed):
    ds, per_image, preds, gts = _random_case(seed)
    # the condition under which the two protocols must agree, checked on these inputs: no IoU within 1e-6 of a threshold
    for p, g in zip(preds, gts):
        none = [False] * len(g["boxes"])
        b = coco_eval.box_iou_xywh(_xywh(p["boxes"].numpy()), _xywh(g["boxes"].numpy()), none)
        inter, a_dt, a_gt = coco_eval.intersections_host(p["masks"].numpy(), [wire.rle_counts(m) for m in g["masks"].numpy()], 48, 64)
        m = coco_eval.mask_iou_from_counts(inter, a_dt, a_gt, none)
        for iou in (b, m):
            assert np.abs(iou[:, :, None] - coco_eval.IOU_THRS[None, None, :]).min() > 1e-6
    res = run(ds, per_image)
    for task, kind in (("bbox", "box"), ("segm", "mask")):
        want = evaluation.average_precision(preds, gts, kind)
        assert 0.0 < want < 1.0
        assert abs(res[task]["AP"] / 100.0 - want) <= 1e-9, (task, res[task]["AP"] / 100.0, want)


# ---- rasterisation and segmentation formats -----------------------------------------------------------------------------------------

def test_integer_rectangles_rasterise_to_their_half_open_pixel_ranges():
    h, w = 6, 7
    for x0 in range(w):
        for x1 in range(x0 + 1, w + 1):
            for y0 in range(h):
                for y1 in range(y0 + 1, h + 1):
                    got = coco_eval.counts_to_mask(coco_eval.poly_to_counts(C.rect_poly(x0, y0, x1, y1), h, w), h, w)
                    assert np.array_equal(got.astype(bool), C.rect_mask(h, w, x0, y0, x1, y1)), (x0, y0, x1, y1)


def test_triangle_rasterises_to_28_pixels():
    got = coco_eval.counts_to_mask(coco_eval.poly_to_counts([1, 1, 9, 1, 1, 9], 12, 12), 12, 12)
    want = np.zeros((12, 12), dtype=np.uint8)
    for y in range(1, 8):                      # rows y = 1..7 of widths 7..1 starting at x = 1
        want[y, 1:1 + 8 - y] = 1
    assert got.sum() == 28 and np.array_equal(got, want)


def test_two_polygons_of_one_annotation_are_ored():
    h, w = 20, 30
    a, b = C.rect_poly(2, 3, 12, 9), [8, 5, 25, 6, 15, 18]
    both = coco_eval.counts_to_mask(coco_eval.segmentation_to_counts([a, b], h, w), h, w)
    parts = [coco_eval.counts_to_mask(coco_eval.poly_to_counts(p, h, w), h, w) for p in (a, b)]
    assert np.array_equal(both, parts[0] | parts[1]) and (parts[0] & parts[1]).any() and both.sum() > max(p.sum() for p in parts)


def test_polygon_compressed_and_uncompressed_segmentations_score_identically():
    h, w = 60, 80
    poly = [10, 5, 60, 12, 50, 50, 20, 40]
    m = coco_eval.counts_to_mask(coco_eval.poly_to_counts(poly, h, w), h, w).astype(bool)
    segs = [[poly], wire.rle_encode(m), {"size": [h, w], "counts": wire.rle_counts(m)}]
    det = np.roll(m, (2, -3), axis=(0, 1))
    results = []
    for seg in segs:
        ds = C.dataset({1: (h, w)}, [C.ann(1, 1, 1, C.mask_box(m), seg=seg, area=int(m.sum()))])
        results.append(run(ds, [(1, C.instances(h, w, [C.mask_box(det)], [0.8], masks=det[None]))]))
    assert C.same(results[0], results[1]) and C.same(results[0], results[2])
    assert 0.0 < results[0]["segm"]["AP"] < 100.0


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------

def test_category_ids_map_to_contiguous_classes_and_back(tmp_path):
    ds, per_image = C.mixed_case()
    ev = COCOEvaluator(ds, output_dir=str(tmp_path / "out"))
    assert ev.thing_dataset_id_to_contiguous_id == {1: 0, 3: 1, 7: 2} and ev.thing_classes == ["c1", "c3", "c7"]
    ev.process([{"image_id": i} for i, _ in per_image], [{"instances": inst} for _, inst in per_image])
    res = ev.evaluate()
    assert set(res) == {"bbox", "segm"}
    for task in res:
        assert {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl", "AP-c1", "AP-c3", "AP-c7"} == set(res[task])
        assert 0.0 < res[task]["AP"] < 100.0
    dumped = json.load(open(str(tmp_path / "out" / "coco_instances_results.json")))
    classes = [int(c) for _, inst in per_image for c in inst.pred_classes.tolist()]
    assert [d["category_id"] for d in dumped] == [(1, 3, 7)[c] for c in classes]
    assert all(set(d) == {"image_id", "category_id", "bbox", "score", "segmentation", "mask_score"} for d in dumped)
    # the whole evaluation restricted to one image differs from the whole set
    assert not C.same(ev.evaluate(img_ids=[11]), res)


def test_no_predictions_and_no_annotations():
    ds, per_image = C.mixed_case()
    assert COCOEvaluator(ds).evaluate() == {}
    test_set = {k: v for k, v in ds.items() if k != "annotations"}
    assert run(test_set, per_image) == {}
    # an image processed with no instances at all: every metric NaN (the reference does the same for empty results), not a crash
    h, w = 97, 131
    res = run(ds, [(11, C.instances(h, w, [], []))])
    assert all(math.isnan(v) for v in res["bbox"].values())


def test_refusals(tmp_path):
    ds, per_image = C.mixed_case()
    with pytest.raises(NotImplementedError, match="keypoints"):
        COCOEvaluator(ds, tasks=("bbox", "keypoints"))
    ev = COCOEvaluator(ds)
    with pytest.raises(NotImplementedError, match="proposals"):
        ev.process([{"image_id": 11}], [{"proposals": object()}])
    wrong = C.instances(50, 60, [(1, 1, 20, 20)], [0.5])
    with pytest.raises(ValueError, match="50x60.*97x131"):
        ev.process([{"image_id": 11}], [{"instances": wrong}])
    path = tmp_path / "ann.json"
    path.write_text(json.dumps(ds))
    assert C.same(run(str(path), per_image), run(ds, per_image))      # a path loads the same dict


def dist_case():
    """Three images for the two-rank test: the mixed case plus a third image."""
    ds, per_image = C.mixed_case()
    ds["images"].append({"id": 13, "height": 40, "width": 50})
    ds["annotations"].append(C.ann(99, 13, 7, (5, 5, 30, 30)))
    per_image.append((13, C.instances(40, 50, [(6, 5, 30, 29), (20, 20, 45, 38)], [0.7, 0.6], [2, 2])))
    return ds, per_image


_GLOO_WORKER = r'''
import json, os, sys, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from centermask2_amd.evaluation import COCOEvaluator
from tests.test_cpu_coco_eval import dist_case
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
ds, per_image = dist_case()
mine = per_image[:2] if rank == 0 else per_image[2:]        # uneven shards
ev = COCOEvaluator(ds, distributed=True)
ev.process([{"image_id": i} for i, _ in mine], [{"instances": inst} for _, inst in mine])
res = ev.evaluate()
dist.barrier(); dist.destroy_process_group()
print("RESULT " + json.dumps(res))
'''


def test_two_gloo_ranks_give_rank_0_the_single_process_result(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=120)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    got = [json.loads([ln for ln in o.splitlines() if ln.startswith("RESULT ")][0][7:]) for o in outs]
    want = run(*dist_case())
    assert C.same(got[0], want) and got[0]["segm"]["AP"] > 0.0
    assert got[1] == {}


# ---- the device entries' checks that run before any launch ---------------------------------------------------------------------------

def test_mask_iou_c_abi_argument_validation_without_gpu():
    import ctypes
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def pack(masks=p, r=2, h=5, w=3, words=p, areas=p):
        return lib.cmk_mask_pack_bits(masks, r, h, w, words, areas, None)

    def decode(cum=p, off=p, m=2, h=5, w=3, words=p, areas=p, bits=None):
        return lib.cmk_rle_decode_pack(cum, off, m, h, w, words, areas, bits, None)

    def inter(det=p, n=2, gt=p, m=2, h=5, w=3, out=p):
        return lib.cmk_mask_intersections(det, n, gt, m, h, w, out, None)

    for fn, ptrs, counts in ((pack, ("masks", "words", "areas"), ("r",)), (decode, ("cum", "off", "words", "areas"), ("m",)),
                             (inter, ("det", "gt", "out"), ("n", "m"))):
        for name in ptrs:
            assert fn(**{name: None}) == -1 and b"null" in lib.cmk_last_error(), name
        assert fn(h=65536, w=32768) == -1 and b"int32" in lib.cmk_last_error()          # H*W = 2^31
        assert fn(h=46341, w=46341) == -1                                                # H*W just above 2^31
        assert fn(h=0) == -1 and fn(w=0) == -1 and b"at least 1" in lib.cmk_last_error()
        for c in counts:
            assert fn(**{c: 65536}) == -1 and b"65535" in lib.cmk_last_error()
            assert fn(**{c: -1}) == -1
            assert fn(**{c: 0}) == 0                                                     # nothing to do: no launch, no complaint
    assert pack(r=0, masks=None, words=None, areas=None) == 0


def test_mask_ops_refuse_host_and_malformed_input():
    from centermask2_amd import _lib, ops
    host = torch.zeros((2, 4, 4), dtype=torch.bool)
    with pytest.raises(_lib.CmkError, match="GPU"):
        ops.mask_pack_bits(host)
    with pytest.raises(_lib.CmkError, match="GPU"):
        ops.mask_intersections(host, [[16]], 4, 4)
    with pytest.raises(_lib.CmkError):
        ops.mask_pack_bits(np.zeros((2, 4, 4), dtype=bool))
    for bad in ([[3, 4]], [[17]], [[]], [[20, -4]]):                                     # runs that do not add up to 4x4
        with pytest.raises(_lib.CmkError, match="add up"):
            ops.mask_rle_decode(bad, 4, 4)
