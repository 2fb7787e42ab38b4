"""Sliced inference without a GPU: the TEST.SLICE defaults, the tile grid, the properties of the numpy restatement (tests/slice_ref.py) the
kernels are held to, the C ABI's argument checks (include/cmk.h: cmk_slice_boxes_to_image, cmk_nms_topk_metric), which run before any
launch, and the refusals and routing on the Python side."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from centermask2_amd import _lib, ops
from . import slice_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cmk_slice_boxes_to_image", "cmk_nms_topk_metric")


def _cpu_cfg(extra=()):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(extra))
    return cfg


def test_slice_defaults():
    from centermask2_amd.config import get_cfg
    sl = get_cfg().TEST.SLICE
    assert sl.ENABLED is False and tuple(sl.TILE) == (512, 512) and sl.OVERLAP == 0.2 and sl.FULL_IMAGE is True
    assert sl.MATCH_METRIC == "IOS" and sl.MATCH_THRESH == 0.5 and sl.BATCH == 8
    assert _cpu_cfg().TEST.SLICE.ENABLED is False                   # the shipped recipes leave it off


GRIDS = [(300, 420, 160, 200, 0.25), (1024, 2048, 512, 512, 0.2), (97, 131, 40, 50, 0.0), (64, 64, 64, 64, 0.5), (65, 64, 64, 64, 0.9),
         (200, 100, 7, 300, 0.99), (33, 1000, 32, 17, 0.3)]


@pytest.mark.parametrize("h,w,th,tw,ov", GRIDS)
def test_grid_properties(h, w, th, tw, ov):
    g = ops.slice_grid(h, w, th, tw, ov)
    assert g == slice_ref.grid(h, w, th, tw, ov) and len(set(g)) == len(g)
    eh, ew = min(th, h), min(tw, w)
    cover = np.zeros((h, w), dtype=bool)
    for y0, x0, a, b in g:
        assert (a, b) == (eh, ew) and 0 <= y0 and y0 + a <= h and 0 <= x0 and x0 + b <= w          # inside, equal size
        cover[y0:y0 + a, x0:x0 + b] = True
    assert cover.all()                                                                              # the union covers the image
    assert g == sorted(g)                                                                           # row-major
    for axis, (size, t) in enumerate(((h, eh), (w, ew))):
        starts = sorted({c[axis] for c in g})
        assert starts[0] == 0 and starts[-1] == size - t
        stride = max(1, int(t * (1 - ov)))
        for s0, s1 in zip(starts[:-2], starts[1:-1]):                                               # the regular part of the axis
            assert s1 - s0 == stride and s0 + t - s1 >= int(ov * t)
        if len(starts) > 1:                                                                         # the last tile is shifted back: it
            assert 0 < starts[-1] - starts[-2] <= stride                                            # overlaps its neighbour by no less
            assert starts[-2] + t - starts[-1] >= min(t - stride, int(ov * t))


def test_grid_known_answers():
    g = ops.slice_grid(300, 420, 160, 200, 0.25)
    assert len(g) == 9 and sorted({c[0] for c in g}) == [0, 120, 140] and sorted({c[1] for c in g}) == [0, 150, 220]
    assert g[0] == (0, 0, 160, 200) and g[1] == (0, 150, 160, 200) and g[-1] == (140, 220, 160, 200)
    assert ops.slice_grid(100, 90, 512, 512, 0.2) == [(0, 0, 100, 90)]                              # smaller than the tile: one tile
    assert ops.slice_grid(512, 512, 512, 512, 0.2) == [(0, 0, 512, 512)]
    assert ops.slice_grid(100, 600, 512, 512, 0.2) == [(0, 0, 100, 512), (0, 88, 100, 512)]
    part = ops.slice_grid(120, 200, 40, 50, 0.0)                                                    # overlap 0, sizes divide: a partition
    assert part == [(y, x, 40, 50) for y in (0, 40, 80) for x in (0, 50, 100, 150)]
    assert sum(a * b for _, _, a, b in part) == 120 * 200
    assert len(ops.slice_grid(1024, 2048, 512, 512, 0.2)) == 3 * 5
    for bad in (dict(overlap=1.0), dict(overlap=-0.1), dict(tile_h=0), dict(tile_w=-4), dict(h=0)):
        with pytest.raises(ValueError):
            ops.slice_grid(**dict(dict(h=10, w=10, tile_h=4, tile_w=4, overlap=0.2), **bad))


def test_restatement_map_identity_shift_and_clip():
    pss = [(0, 0, 40, 50, 40, 50), (10, 20, 40, 50, 80, 100), (0, 0, 100, 120, 50, 60)]
    t = slice_ref.table(pss)
    assert t.dtype == np.float32 and np.array_equal(t, np.array([[0, 0, 1, 1, 50, 40], [20, 10, 0.5, 0.5, 50, 40], [0, 0, 2, 2, 120, 100]], np.float32))
    assert np.array_equal(ops.slice_table(pss, "cpu").numpy(), t)
    box = np.zeros((3, 2, 4), np.float32)
    box[:, 0] = [4, 6, 30, 20]
    box[:, 1] = [-8, -8, 400, 400]
    loc = box[:, :, :2].copy()
    got = slice_ref.boxes_to_image(box, np.ones((3, 2)), np.full((3, 2), 7, np.int64), loc, [2, 1, 5], pss)
    assert got["cls"].dtype == np.int32 and got["src"].tolist() == [0, 1, 2, 4, 5]                  # counts clamp to K; slot a*K + k
    assert got["box"].tolist() == [[4, 6, 30, 20], [0, 0, 50, 40], [22, 13, 35, 20], [8, 12, 60, 40], [0, 0, 120, 100]]
    assert got["loc"].tolist() == [[4, 6], [-8, -8], [22, 13], [8, 12], [-16, -16]]                # the point is not clipped
    none = slice_ref.boxes_to_image(box, np.ones((3, 2)), np.zeros((3, 2), np.int64), loc, [0, -3, 0], pss)
    assert none["box"].shape == (0, 4) and none["src"].shape == (0,)


def test_restatement_nms_ios_nested_box_classwise_and_stable():
    box = np.array([[0, 0, 100, 100], [10, 10, 30, 30], [10, 10, 30, 30], [10, 10, 30, 30], [50, 50, 50, 80]], dtype=np.float32)
    score = np.array([0.9, 0.5, 0.5, 0.6, 0.95], dtype=np.float32)
    cls = np.array([1, 1, 1, 2, 1])
    assert slice_ref.iou(box[0], box[1]) == pytest.approx(0.04) and slice_ref.ios(box[0], box[1]) == 1.0
    assert np.isnan(slice_ref.ios(box[4], box[0]))
    # IoU leaves the nested box alone (0.04), IoS drops it; class 2 is left alone; the zero-area box neither suppresses nor is suppressed
    assert slice_ref.nms(box, score, cls, 0.5, 100, "iou") == [4, 0, 3, 1]                          # the tie 1/2: the earlier one stays
    assert slice_ref.nms(box, score, cls, 0.5, 100, "ios") == [4, 0, 3]
    assert slice_ref.nms(box[1:], score[1:], cls[1:], 0.5, 100, "ios") == [3, 2, 0]                 # without the large box: stable on the tie
    assert slice_ref.nms(box, score, cls, 0.5, 2, "ios") == [4, 0]
    assert slice_ref.nms_margin(box, score, cls, 0.5, 100, "ios") == ([4, 0, 3], 0.5)           # 1.0 and "no kept box of the class" decide
    assert slice_ref.nms_margin(box, score, cls, 0.5, 100, "iou") == ([4, 0, 3, 1], pytest.approx(0.46))      # the nested box at 0.04 is kept
    assert slice_ref.nms_margin(box, score, cls, 0.03, 100, "iou") == ([4, 0, 3], pytest.approx(0.01))
    m = slice_ref.pair_metric(box, cls, "ios")
    assert m[0, 1] == 1.0 and m[0, 3] == -1 and m[0, 4] == -1 and m[1, 2] == 1.0
    assert slice_ref.pair_metric(box, cls, "iou")[0, 1] == pytest.approx(0.04)


def test_slice_entries_are_declared_and_wrapped():
    header = open(os.path.join(ROOT, "include", "cmk.h")).read()
    declared = set(re.findall(r"\b(cmk_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES)
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
    assert len(_lib.SIGNATURES["cmk_nms_topk_metric"][1]) == len(_lib.SIGNATURES["cmk_nms_topk"][1]) + 1
    assert all(hasattr(ops, n) for n in ("slice_grid", "slice_table", "slice_boxes_to_image")) and ops.NMS_METRICS == {"iou": 0, "ios": 1}
    import centermask2_amd
    from centermask2_amd.modeling import sliced_inference as M
    assert centermask2_amd.SlicedInference is M.SlicedInference and "SlicedInference" in centermask2_amd.__all__


def test_slice_c_abi_argument_validation_without_gpu():
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def refused(rc, word=None):
        err = lib.cmk_last_error()
        return rc == -1 and err.strip() and (word is None or word in err)

    def to_image(box=p, score=p, cls=p, loc=p, counts=p, table=p, A=2, K=3, w=64, h=48, cbox=p, cscore=p, ccls=p, cloc=p, csrc=p, ccount=p):
        return lib.cmk_slice_boxes_to_image(box, score, cls, loc, counts, table, A, K, w, h, cbox, cscore, ccls, cloc, csrc, ccount, None)

    for name in ("box", "score", "cls", "loc", "counts", "table", "cbox", "cscore", "ccls", "cloc", "csrc", "ccount"):
        assert refused(to_image(**{name: None}), b"null"), name
    for bad in (dict(A=0), dict(A=-1), dict(A=4097), dict(K=0), dict(K=-5), dict(K=65536)):
        assert refused(to_image(**bad), b"need 1 <="), bad
    for bad in (dict(w=0), dict(h=0), dict(w=-3), dict(w=65536), dict(h=65536)):
        assert refused(to_image(**bad), b"image size"), bad
    assert refused(to_image(box=p + 4), b"aligned") and refused(to_image(cbox=p + 8), b"aligned")

    def nms(metric=1, topk=5, n=1, cap=8, **null):
        a = {k: null.get(k, p) for k in ("cand_box", "cand_score", "cand_cls", "cand_loc", "counts", "out_box", "out_score", "out_cls", "out_loc",
                                         "out_idx", "out_count", "sort_ws")}
        return lib.cmk_nms_topk_metric(a["cand_box"], a["cand_score"], a["cand_cls"], a["cand_loc"], a["counts"], n, cap, 0.5, metric, topk,
                                       a["out_box"], a["out_score"], a["out_cls"], a["out_loc"], a["out_idx"], a["out_count"], a["sort_ws"], None)

    for name in ("cand_box", "cand_score", "cand_cls", "cand_loc", "counts", "out_box", "out_score", "out_cls", "out_loc", "out_idx", "out_count",
                 "sort_ws"):
        assert refused(nms(**{name: None}), b"null"), name
    for metric in (0, 1):
        for bad in (dict(topk=0), dict(topk=1025), dict(n=0), dict(cap=0)):
            assert refused(nms(metric=metric, **bad), b"topk"), bad
    for metric in (2, -1, 7):
        assert refused(nms(metric=metric), b"metric"), metric


def test_ops_wrappers_refuse_host_tensors():
    a, k = 2, 3
    det = dict(box=torch.zeros((a, k, 4)), score=torch.zeros((a, k)), cls=torch.zeros((a, k), dtype=torch.int64), loc=torch.zeros((a, k, 2)),
               counts=torch.zeros(a, dtype=torch.int32))
    with pytest.raises(_lib.CmkError, match="no CPU fallback"):
        ops.slice_boxes_to_image(det, torch.zeros((a, 6)), 48, 64)
    with pytest.raises(_lib.CmkError, match="shape"):
        ops.slice_boxes_to_image(dict(det, box=torch.zeros((a, k, 5))), torch.zeros((a, 6)), 48, 64)
    with pytest.raises(_lib.CmkError, match="need \\(A,K\\) scores"):
        ops.slice_boxes_to_image(dict(det, score=torch.zeros((a * k,))), torch.zeros((a, 6)), 48, 64)
    cand = dict(box=torch.zeros((1, 8, 4)), score=torch.zeros((1, 8)), cls=torch.zeros((1, 8), dtype=torch.int32), loc=torch.zeros((1, 8, 2)),
                counts=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.CmkError, match="no CPU fallback"):
        ops.nms_topk(cand, 0.5, 4, metric="ios")
    with pytest.raises(_lib.CmkError, match="metric"):
        ops.nms_topk(cand, 0.5, 4, metric="giou")


def test_slice_refusals_name_their_keys():
    from centermask2_amd import Predictor, SlicedInference
    from centermask2_amd.modeling import build_model
    model = build_model(_cpu_cfg())
    for extra, exc, key in ((["TEST.SLICE.OVERLAP", 1.0], ValueError, "TEST.SLICE.OVERLAP"), (["TEST.SLICE.OVERLAP", -0.01], ValueError, "TEST.SLICE.OVERLAP"),
                            (["TEST.SLICE.TILE", (0, 512)], ValueError, "TEST.SLICE.TILE"), (["TEST.SLICE.TILE", (512, -1)], ValueError, "TEST.SLICE.TILE"),
                            (["TEST.SLICE.BATCH", 0], ValueError, "TEST.SLICE.BATCH"), (["TEST.SLICE.MATCH_METRIC", "GIOU"], ValueError, "TEST.SLICE.MATCH_METRIC"),
                            (["TEST.DETECTIONS_PER_IMAGE", 2000], NotImplementedError, "TEST.DETECTIONS_PER_IMAGE"),
                            (["TEST.DETECTIONS_PER_IMAGE", 0], NotImplementedError, "TEST.DETECTIONS_PER_IMAGE"),
                            (["MODEL.KEYPOINT_ON", True], NotImplementedError, "MODEL.KEYPOINT_ON"),
                            (["TEST.AUG.ENABLED", True], NotImplementedError, "TEST.AUG.ENABLED")):
        on = ["TEST.SLICE.ENABLED", True] + extra
        with pytest.raises(exc, match=re.escape(key)):
            SlicedInference(_cpu_cfg(on), model)
        with pytest.raises(exc, match=re.escape(key)):
            Predictor(_cpu_cfg(on), model=model)
    with pytest.raises(NotImplementedError, match="TEST.SLICE"):
        SlicedInference(_cpu_cfg(["TEST.SLICE.ENABLED", True, "MODEL.KEYPOINT_ON", True]), model)
    s = SlicedInference(_cpu_cfg(["TEST.SLICE.TILE", (160, 200), "TEST.SLICE.OVERLAP", 0.25, "TEST.SLICE.MATCH_METRIC", "IOU", "INPUT.MIN_SIZE_TEST", 192,
                                  "INPUT.MAX_SIZE_TEST", 333]), model)
    assert (s.tile, s.overlap, s.batch, s.metric, s.match_thresh, s.full_image, s.topk) == ((160, 200), 0.25, 8, "iou", 0.5, True, 100)
    pss = s.passes(300, 420)
    assert pss == slice_ref.passes(300, 420, 160, 200, 0.25, 192, 333, True) and len(pss) == 10
    assert len({p[2:] for p in pss[:-1]}) == 1 and pss[-1][:4] == (0, 0, 300, 420)                  # equal tiles, then the whole image
    with pytest.raises(_lib.CmkError):
        s([{"image": torch.zeros((8, 8, 3), dtype=torch.uint8)}])                            # HWC, not the mapper's CHW
    with pytest.raises(_lib.CmkError, match="no CPU fallback"):
        s([{"image": torch.zeros((3, 8, 8), dtype=torch.uint8)}])


def test_predictor_builds_the_sliced_object_only_when_enabled(monkeypatch):
    from centermask2_amd import Predictor
    from centermask2_amd.modeling import build_model, sliced_inference as M
    model = build_model(_cpu_cfg())
    built = []
    real = M.SlicedInference.__init__

    def spy(self, cfg, model):
        built.append(cfg)
        real(self, cfg, model)

    monkeypatch.setattr(M.SlicedInference, "__init__", spy)
    off = Predictor(_cpu_cfg(), model=model)
    assert off.sliced is None and off.tta is None and not built
    on = Predictor(_cpu_cfg(["TEST.SLICE.ENABLED", True]), model=model)
    assert isinstance(on.sliced, M.SlicedInference) and on.tta is None and len(built) == 1 and on.sliced.model is on.model
    assert on.sliced.tile == (512, 512) and on.sliced.metric == "ios"
