"""not gpu: Boundary AP on the host.  The literal reference (tests/boundary_ref.py) against known answers, coco_eval.boundary_host against
the reference, the erosion distance rule, the argument checks of cmk_mask_boundary_bits (nothing is launched), and COCOEvaluator with the
task "boundary" on CPU Instances against numbers built here from the reference.  Every comparison is == on integers or on floats formed
from identical integers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from centermask2_amd import coco_eval, ops, wire
from centermask2_amd.evaluation import COCOEvaluator
from tests import boundary_ref as B
from tests import coco_cases as C

SHAPES = [(1, 1), (7, 9), (40, 20), (64, 64), (33, 65), (20, 128), (97, 131)]
DS = [1, 2, 5, 16, 40]


def test_reference_known_answers():
    """Answers worked out by hand, for the literal reference and for the host path alike."""
    full = np.ones((1, 20, 30), dtype=np.uint8)
    b = B.boundary_ref(full, 4)
    assert int(b.sum()) == 600 - 12 * 22 == 336 == int(coco_eval.boundary_host(full, 4).sum())
    assert not b[0, 4:16, 4:26].any() and b[0, :4].all() and b[0, :, :4].all() and b[0, 16:].all() and b[0, :, 26:].all()
    one = np.zeros((1, 9, 11), dtype=np.uint8)
    one[0, 4, 5] = 1
    for d in (1, 3, 20):
        assert np.array_equal(B.boundary_ref(one, d), one.astype(bool))
    r = B.rect(40, 50, 5, 16, 7, 40)[None]                               # 11 x 33
    assert np.array_equal(B.boundary_ref(r, 6), r.astype(bool))            # 2*6+1 > 11
    assert int(B.boundary_ref(r, 5).sum()) == 11 * 33 - 1 * 23              # 2*5+1 = 11: one row of 33 - 10 survives the erosion
    assert int(B.boundary_ref(r, 2).sum()) == 11 * 33 - 7 * 29
    # the same rectangle against two image edges: the outside is background, so the edge erodes as any other side does
    r = B.rect(40, 50, 0, 11, 0, 33)[None]
    assert int(B.boundary_ref(r, 2).sum()) == 11 * 33 - 7 * 29


@pytest.mark.parametrize("h,w", SHAPES)
def test_host_path_equals_the_literal_reference(h, w):
    m = B.mask_set(h, w, seed=h * 1000 + w)
    for d in DS:
        got = coco_eval.boundary_host(m, d)
        assert got.dtype == np.bool_ and got.shape == m.shape
        assert np.array_equal(got, B.boundary_ref(m, d)), (h, w, d)
        if 2 * d + 1 > min(h, w):
            assert np.array_equal(got, m.astype(bool))
    assert coco_eval.boundary_host(m[:0], 3).shape == (0, h, w)
    with pytest.raises(ValueError):
        coco_eval.boundary_host(m, 0)


def test_dilation_rule():
    assert ops.boundary_dilation(100, 100) == 3
    assert ops.boundary_dilation(800, 1280) == 30
    assert ops.boundary_dilation(5, 5) == 1
    assert ops.boundary_dilation(1, 1) == 1 and ops.boundary_dilation(100, 100, ratio=0.05) == 7
    assert ops.boundary_dilation(480, 640) == 16 and coco_eval.boundary_dilation(480, 640) == 16


def test_c_abi_refusals_without_gpu(cmk_lib):
    """Every refusal sits before any launch: -1 and a message; R == 0 is accepted and launches nothing."""
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    far = p + (1 << 40)                                                  # never dereferenced: the calls below are all refused
    f = cmk_lib.cmk_mask_boundary_bits

    def refused(args, word):
        rc = f(*args)
        err = cmk_lib.cmk_last_error().decode()
        assert rc == -1 and err.strip() and "mask_boundary_bits" in err and word in err, (args, rc, err)

    assert f(None, 0, 0, 0, 0, None, None, None) == 0
    refused((None, 1, 8, 8, 1, far, p, None), "null")
    refused((p, 1, 8, 8, 1, None, p, None), "null")
    refused((p, 1, 8, 8, 1, far, None, None), "null")
    refused((p, 1, 0, 8, 1, far, p, None), "at least 1")
    refused((p, 1, 8, 0, 1, far, p, None), "at least 1")
    refused((p, 1, 65536, 32768, 1, far, p, None), "int32")
    refused((p, 1, 46341, 46341, 1, far, p, None), "int32")
    refused((p, -1, 8, 8, 1, far, p, None), "65535")
    refused((p, 65536, 8, 8, 1, far, p, None), "65535")
    refused((p, 1, 8, 8, 0, far, p, None), "at least 1")
    refused((p, 1, 8, 8, -3, far, p, None), "at least 1")
    refused((p, 1, 300, 4096, 129, far, p, None), "CMK_BOUNDARY_MAX_D")
    refused((p, 1, 64, 64, 1, p + 8, p, None), "overlaps")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmk.h")) as fh:
        header = fh.read()
    assert "#define CMK_BOUNDARY_MAX_D 128" in header                    # the limit is stated where the contract is; not below 128


def _square_case(shift):
    """100x100, one class, one ground-truth square [10:50, 10:50], one detection: the same square `shift` pixels to the right."""
    ds = C.dataset({1: (100, 100)}, [C.ann(1, 1, 1, (10, 10, 50, 50))])
    inst = C.instances(100, 100, [[10 + shift, 10, 50 + shift, 50]], [0.9])
    return ds, inst


def _ious_by_brute_force(g, m, d):
    bg, bm = B.boundary_ref(g[None], d)[0], B.boundary_ref(m[None], d)[0]
    mask = int((g & m).sum()), int((g | m).sum())
    bnd = int((bg & bm).sum()), int((bg | bm).sum())
    return mask, bnd


ONE = 1.0 / (1.0 + np.spacing(1.0))       # COCOeval's precision of 1 true positive and no false one: tp / (fp + tp + eps)


def full(cells):
    """ "100": the mean of `cells` precisions of ONE, times 100, formed as the evaluator forms it (99.99999999999997, not 100.0)."""
    return float(np.mean(np.full(cells, ONE))) * 100


def _ap(iou):
    """One ground truth, one detection: the precision is ONE at every recall level of every threshold where the pair matches, else 0;
    AP averages 10 x 101 such cells, AP50 and AP75 101 each."""
    hit = np.repeat(np.where(iou >= coco_eval.IOU_THRS, ONE, 0.0)[:, None], len(coco_eval.REC_THRS), axis=1)
    return float(np.mean(hit.reshape(-1))) * 100, float(np.mean(hit[0])) * 100, float(np.mean(hit[5])) * 100


@pytest.mark.parametrize("shift", [0, 4])
def test_evaluator_known_answer_on_cpu_instances(shift):
    ds, inst = _square_case(shift)
    d = ops.boundary_dilation(100, 100)
    g = C.rect_mask(100, 100, 10, 10, 50, 50)
    m = C.rect_mask(100, 100, 10 + shift, 10, 50 + shift, 50)
    mask, bnd = _ious_by_brute_force(g, m, d)
    if shift == 4:
        assert mask == (1440, 1760) and bnd == (216, 672)
    else:
        assert mask == (1600, 1600) and bnd == (444, 444)
    iou_m, iou_b = mask[0] / mask[1], bnd[0] / bnd[1]
    ev = COCOEvaluator(ds, tasks=("bbox", "segm", "boundary"))
    ev.process([{"image_id": 1}], [{"instances": inst}])
    (pred,) = ev._predictions
    assert len(pred["table"]) == 3 and len(pred["boundary_table"]) == 3
    assert [int(np.asarray(v).reshape(-1)[0]) for v in pred["table"]] == [mask[0], 1600, 1600]
    assert [int(np.asarray(v).reshape(-1)[0]) for v in pred["boundary_table"]] == [bnd[0], 444, 444]
    res = ev.evaluate()
    assert set(res) == {"bbox", "segm", "boundary"} and set(res["boundary"]) == set(res["segm"])
    for task, iou in (("segm", iou_m), ("boundary", min(iou_m, iou_b))):
        ap, ap50, ap75 = _ap(iou)
        assert (res[task]["AP"], res[task]["AP50"], res[task]["AP75"]) == (ap, ap50, ap75), task
    if shift == 4:                                                         # the point of the metric, and of the minimum
        assert res["segm"]["AP50"] == res["segm"]["AP75"] == full(101) and res["boundary"]["AP"] == res["boundary"]["AP50"] == 0.0
    else:
        assert res["boundary"]["AP"] == full(1010) and res["boundary"]["AP50"] == res["boundary"]["AP75"] == full(101)
    # areas are the full masks': a 40x40 square is a medium object for boundary as for segm
    assert res["boundary"]["APm"] == res["boundary"]["AP"] and res["boundary"]["APs"] != res["boundary"]["APs"]


def test_boundary_iou_is_the_minimum_of_both():
    """A detection whose boundary fits better than its mask: the mask IoU decides."""
    g = C.rect_mask(100, 100, 10, 10, 50, 50)
    m2 = g.copy()
    m2[13:47, 13:47] = False                                               # exactly the ground truth's boundary ring
    ds = C.dataset({1: (100, 100)}, [C.ann(1, 1, 1, (10, 10, 50, 50))])
    inst = C.instances(100, 100, [[10, 10, 50, 50]], [0.9], masks=np.stack([m2]))
    ev = COCOEvaluator(ds, tasks=("boundary",))
    ev.process([{"image_id": 1}], [{"instances": inst}])
    t, bt = ev._predictions[0]["table"], ev._predictions[0]["boundary_table"]
    assert (int(t[0][0, 0]), int(t[1][0]), int(t[2][0])) == (444, 444, 1600)
    assert (int(bt[0][0, 0]), int(bt[1][0]), int(bt[2][0])) == (444, 444, 444)      # boundary IoU 1, mask IoU 444/1600 < 0.5
    assert ev.evaluate()["boundary"]["AP50"] == 0.0


def test_crowd_rule_in_the_boundary_term():
    """A thin detection inside the boundary band of a crowd region: inter_b / a_dt_b = 1 (the union rule would give 180 / a_gt_b), so
    it is matched to the crowd and ignored, and the other detection's perfect match is all that counts."""
    d = ops.boundary_dilation(100, 100)
    crowd = C.rect_mask(100, 100, 10, 50, 90, 90)
    thin = C.rect_mask(100, 100, 20, 50, 80, 53)
    anns = [C.ann(1, 1, 1, (10, 10, 40, 40)),
            C.ann(2, 1, 1, (10, 50, 90, 90), iscrowd=1, seg={"size": [100, 100], "counts": wire.rle_counts(crowd)})]
    ds = C.dataset({1: (100, 100)}, anns)
    inst = C.instances(100, 100, [[10, 10, 40, 40], [20, 50, 80, 53]], [0.5, 0.9])
    six = coco_eval.boundary_intersections_host(inst.pred_masks.numpy(), coco_eval.GroundTruth(ds).counts(1), 100, 100, d)
    three = coco_eval.intersections_host(inst.pred_masks.numpy(), coco_eval.GroundTruth(ds).counts(1), 100, 100)
    assert all(np.array_equal(a, b) and a.dtype == np.int32 for a, b in zip(six[:3], three))
    bc, bt = B.boundary_ref(crowd[None], d)[0], B.boundary_ref(thin[None], d)[0]
    assert np.array_equal(bt, thin) and int((bc & bt).sum()) == 180
    assert int(six[3][1, 1]) == 180 == int(six[4][1]) and int(six[5][1]) == int(bc.sum()) == 40 * 80 - 34 * 74
    iou = coco_eval.mask_iou_from_counts(six[3], six[4], six[5], [False, True])
    assert iou[1, 1] == 1.0 and iou[0, 1] == 0.0 and iou[0, 0] == 1.0
    ev = COCOEvaluator(ds, tasks=("segm", "boundary"))
    ev.process([{"image_id": 1}], [{"instances": inst}])
    res = ev.evaluate()
    assert res["boundary"]["AP"] == full(1010) and res["segm"]["AP"] == full(1010)
    # the same detection one band further in misses the crowd's boundary: not ignored any more, a false positive ahead of the match
    inst2 = C.instances(100, 100, [[10, 10, 40, 40], [20, 60, 80, 63]], [0.5, 0.9])
    ev = COCOEvaluator(ds, tasks=("segm", "boundary"))
    ev.process([{"image_id": 1}], [{"instances": inst2}])
    res = ev.evaluate()
    assert res["segm"]["AP"] == full(1010) and res["boundary"]["AP"] == 50.0          # 1 / (2 + eps) is 0.5 in float64


def test_defaults_are_unchanged():
    ds, per_image = C.mixed_case()
    ev = COCOEvaluator(ds)
    ev.process([{"image_id": i} for i, _ in per_image], [{"instances": inst} for _, inst in per_image])
    assert all("boundary_table" not in p and len(p["table"]) == 3 for p in ev._predictions)
    assert set(ev.evaluate()) == {"bbox", "segm"}
    ev = COCOEvaluator(ds, tasks=("bbox", "segm", "boundary"), boundary_dilation_ratio=0.02)
    ev.process([{"image_id": i} for i, _ in per_image], [{"instances": inst} for _, inst in per_image])
    res = ev.evaluate()
    assert set(res) == {"bbox", "segm", "boundary"} and set(res["boundary"]) == set(res["segm"])
    assert {"AP", "AP50", "AP75", "APs", "APm", "APl", "AP-c1", "AP-c3", "AP-c7"} <= set(res["boundary"])
    assert 0.0 <= res["boundary"]["AP"] <= res["segm"]["AP"]
    for p in ev._predictions:
        assert all(np.array_equal(a, b) for a, b in zip(p["table"], coco_eval.intersections_host(
            dict(per_image)[p["image_id"]].pred_masks.numpy(), coco_eval.GroundTruth(ds).counts(p["image_id"]), *ev._gt.size(p["image_id"]))))


def test_task_names_and_missing_masks():
    ds, inst = _square_case(0)
    with pytest.raises(NotImplementedError, match="keypoints"):
        COCOEvaluator(ds, tasks=("boundary", "keypoints"))
    with pytest.raises(ValueError, match="nope"):
        COCOEvaluator(ds, tasks=("nope",))
    with pytest.raises(ValueError, match="not built"):
        coco_eval.score(coco_eval.GroundTruth(ds), [], "keypoints")
    ev = COCOEvaluator(ds, tasks=("boundary",))
    ev.process([{"image_id": 1}], [{"instances": C.instances(100, 100, [[10, 10, 50, 50]], [0.9], masks=None)}])
    with pytest.raises(ValueError, match="no mask table"):
        ev.evaluate()


def test_device_entries_refuse_cpu_tensors():
    from centermask2_amd import _lib
    with pytest.raises(_lib.CmkError):
        ops.mask_boundary(torch.zeros((1, 4, 4), dtype=torch.bool))
    with pytest.raises(_lib.CmkError):
        ops.mask_boundary_bits(torch.zeros((1, 1), dtype=torch.int64), 4, 4, 1)
    with pytest.raises(_lib.CmkError):
        ops.mask_boundary_intersections(torch.zeros((1, 4, 4), dtype=torch.bool), [[16]], 4, 4, 1)
