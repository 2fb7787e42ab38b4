"""not gpu: video mode's host side — hand-derived known answers for the NumPy restatement of the association rule (tests/video_ref.py) the
GPU tests compare the kernels with, the C ABI's argument validation on dummy aligned pointers (nothing is launched), the wrappers' and
classes' refusals, and the exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from centermask2_amd import video
from . import video_ref as V

A = [0, 0, 10, 10]
FAR = [[100, 100, 110, 110], [200, 200, 210, 210], [300, 300, 310, 310], [400, 400, 410, 410], [500, 500, 510, 510]]


def table(tr):
    return [(t["id"], t["ttl"]) for t in tr.tracks]


def test_first_frame_and_empty_frame():
    tr = V.RefTracker()
    assert tr.update(FAR[:3], [1, 1, 2]).tolist() == [0, 1, 2] and tr.next_id == 3 and table(tr) == [(0, 8), (1, 8), (2, 8)]
    assert tr.update(np.zeros((0, 4)), []).tolist() == [] and table(tr) == [(0, 7), (1, 7), (2, 7)] and tr.next_id == 3   # every track ages
    assert tr.update([FAR[1], FAR[0]], [1, 1]).tolist() == [1, 0] and table(tr) == [(1, 8), (0, 8), (2, 6)]           # new first, extras behind
    empty = V.RefTracker()
    assert empty.update(np.zeros((0, 4)), []).tolist() == [] and empty.tracks == [] and empty.next_id == 0


def test_class_mismatch_with_iou_one():
    tr = V.RefTracker()
    tr.update([A], [3])
    assert V.box_iou(A, A) == 1.0
    assert tr.update([A], [4]).tolist() == [1] and table(tr) == [(1, 8), (0, 7)]
    assert tr.update([A], [3]).tolist() == [0] and table(tr) == [(0, 8), (1, 7)]         # old row 1 (id 0) matches, old row 0 (id 1) ages


def test_two_old_tracks_claim_one_new_instance():
    """Both old rows have the new instance as their best above the threshold: the lower index wins, even with the smaller IoU."""
    tr = V.RefTracker()
    tr.update([[0, 0, 10, 9.5], A], [0, 0])
    assert V.box_iou([0, 0, 10, 9.5], A) == 0.95 and V.box_iou(A, A) == 1.0
    assert tr.update([A], [0]).tolist() == [0] and table(tr) == [(0, 8), (1, 7)]


def test_tie_in_a_row_takes_the_first_j():
    tr = V.RefTracker()
    tr.update([A], [0])
    assert tr.update([A, A], [0, 0]).tolist() == [0, 1] and table(tr) == [(0, 8), (1, 8)]
    # an all-zero row has its "maximum" at j = 0, which is not above the threshold
    assert tr.update([FAR[0]], [0]).tolist() == [2] and table(tr) == [(2, 8), (0, 7), (1, 7)]


def test_iou_exactly_at_the_threshold_is_not_matched():
    assert (V.BOX_THRESHOLD, V.MASK_THRESHOLD) == (video.BOX_IOU_THRESHOLD, video.MASK_IOU_THRESHOLD)      # the restatement's are the package's
    assert V.box_iou(A, [0, 0, 6, 10]) == 0.6 == V.BOX_THRESHOLD and V.box_iou(A, [0, 0, 6.25, 10]) == 0.625
    tr = V.RefTracker()
    tr.update([A], [0])
    assert tr.update([[0, 0, 6, 10]], [0]).tolist() == [1]
    tr = V.RefTracker()
    tr.update([A], [0])
    assert tr.update([[0, 0, 6.25, 10]], [0]).tolist() == [0]
    m = np.zeros((3, 2, 4), dtype=bool)
    m[0, 0, :] = True                       # 4 pixels
    m[1, 0, :2] = True                      # 2 of them: 2 / 4
    m[2, 0, :3] = True                      # 3 of them: 3 / 4
    assert V.mask_iou(m[0], m[1]) == 0.5 == V.MASK_THRESHOLD and V.mask_iou(m[0], m[2]) == 0.75 and V.mask_iou(m[0] & False, m[0] & False) == 0.0
    for new, want in ((1, [1]), (2, [0])):
        tr = V.RefTracker(match="mask")
        tr.update([A], [0], m[:1])
        assert tr.update([FAR[0]], [0], m[new:new + 1]).tolist() == want          # mask mode never looks at the boxes


def test_ttl_survives_the_seventh_miss_and_expires_on_the_eighth():
    tr = V.RefTracker(ttl=8)
    tr.update([A], [0])
    for miss in range(1, 8):
        tr.update(np.zeros((0, 4)), [])
        assert table(tr) == [(0, 8 - miss)], miss
    again = V.RefTracker(ttl=8)
    again.tracks, again.next_id = [dict(t) for t in tr.tracks], tr.next_id
    assert again.update([A], [0]).tolist() == [0] and table(again) == [(0, 8)]          # seen again after seven misses: the same id, fresh ttl
    tr.update(np.zeros((0, 4)), [])
    assert tr.tracks == [] and tr.dropped == 0                                            # expiry is not a drop
    assert tr.update([A], [0]).tolist() == [1]
    one = V.RefTracker(ttl=1)
    one.update([A], [0])
    assert one.update([FAR[0]], [0]).tolist() == [1] and table(one) == [(1, 1)]


def test_capacity_full_and_over_by_one():
    tr = V.RefTracker(max_tracks=4)
    tr.update(FAR[:2], [0, 0])
    assert tr.update(FAR[2:4], [0, 0]).tolist() == [2, 3] and table(tr) == [(2, 8), (3, 8), (0, 7), (1, 7)] and tr.dropped == 0
    tr = V.RefTracker(max_tracks=4)
    tr.update(FAR[:2], [0, 0])
    assert tr.update(FAR[2:5], [0, 0, 0]).tolist() == [2, 3, 4] and table(tr) == [(2, 8), (3, 8), (4, 8), (0, 7)] and tr.dropped == 1
    tr.update(FAR[:4], [0, 0, 0, 0])                                  # a full frame: FAR[0] is id 0 again, no room for any extra
    assert table(tr) == [(0, 8), (5, 8), (2, 8), (3, 8)] and tr.dropped == 2
    with pytest.raises(AssertionError):
        tr.update(FAR[:5], [0] * 5)


def test_nan_box():
    nan = [0, float("nan"), 10, 10]
    assert V.box_iou(nan, A) == 0.0 and V.box_iou(A, nan) == 0.0 and V.box_iou(nan, nan) == 0.0
    assert V.box_iou([0, 0, 0, 0], [0, 0, 0, 0]) == 0.0                       # a zero union
    assert V.box_iou([0, 0, float("inf"), 10], [0, 0, float("inf"), 10]) == 0.0       # inf / inf
    tr = V.RefTracker()
    tr.update([nan, A], [0, 0])
    assert tr.update([nan, A], [0, 0]).tolist() == [2, 1] and table(tr) == [(2, 8), (1, 8), (0, 7)]
    assert np.isnan(tr.arrays()["boxes"][2, 1])


@pytest.mark.parametrize("match,size,cap,ttl", [("box", (480, 640), 64, 8), ("box", (480, 640), 12, 2), ("mask", (37, 53), 64, 3), ("mask", (5, 7), 11, 8)])
def test_assign_tables_is_the_tracker_on_tables(match, size, cap, ttl):
    """video_ref.assign_tables (the rule on tables in plain loops, what the conformance rows of cmk_vis_track_assign are held to) against
    RefTracker.update over the frames of video_ref.sequence: the same table, src, ids and counters, frame for frame.  The table handed
    in is the ungated one (box_iou or the intersection counts of every pair): the class gate is assign_tables' own."""
    tr = V.RefTracker(match=match, ttl=ttl, max_tracks=cap)
    counters = np.array([0, 0, 0, 77], dtype=np.int32)
    old = dict(boxes=np.zeros((0, 4), np.float32), classes=np.zeros(0, np.int64), ids=np.zeros(0, np.int32), ttl=np.zeros(0, np.int32))
    old_masks = np.zeros((0,) + size, dtype=bool)
    matched = 0
    for f in V.sequence(9, frames=9, seed=4, size=size, with_masks=match == "mask"):
        n, rows = len(f["boxes"]), len(old["ids"])
        if match == "box":
            value = np.array([[V.box_iou(old["boxes"][i], f["boxes"][j]) for j in range(n)] for i in range(rows)], dtype=np.float64).reshape(rows, n)
        else:
            inter = np.array([[np.count_nonzero(old_masks[i] & f["masks"][j]) for j in range(n)] for i in range(rows)], dtype=np.int64).reshape(rows, n)
            value = V.mask_values(inter, [int(m.sum()) for m in old_masks], [int(m.sum()) for m in f["masks"]])
        new = dict(boxes=f["boxes"], classes=f["classes"])
        out, src, ids, counters = V.assign_tables(value, old, counters, new, n, cap, ttl, tr.threshold)
        want_ids = tr.update(f["boxes"], f["classes"], f["masks"])
        want = tr.arrays()
        assert ids.tolist() == want_ids.tolist() and counters.tolist() == [len(tr.tracks), tr.next_id, tr.dropped, 77]
        for k in ("classes", "ids", "ttl"):
            assert out[k].tolist() == want[k].tolist(), k
        assert np.array_equal(out["boxes"].view(np.uint32), want["boxes"].view(np.uint32))
        assert src[:n].tolist() == list(range(n)) and all(v >= n for v in src[n:]) and sorted(set(src.tolist())) == sorted(src.tolist())
        if match == "mask":
            both = np.concatenate([f["masks"], old_masks]) if n + rows else old_masks
            old_masks = both[src] if len(src) else old_masks[:0]
            assert np.array_equal(old_masks, want["masks"])
        matched += int(np.isin(ids, old["ids"]).sum())
        old = out
    assert matched > 0 and (cap > 12 or tr.dropped > 0)


@pytest.mark.parametrize("match,size", [("box", (480, 640)), ("mask", (37, 53)), ("mask", (5, 7))])
def test_array_form_of_the_table_equals_the_scalar_form(match, size):
    """RefTracker.iou_table (whole arrays, what the GPU tests' sequences run on) against box_iou / mask_iou pair by pair, bit for bit, on
    the sequences' own corner cases: duplicates, class mismatches, the NaN box, the empty box, an empty frame."""
    tr = V.RefTracker(match=match, max_tracks=64)
    seen = 0
    for f in V.sequence(9, frames=7, seed=4, size=size, with_masks=match == "mask"):
        a, b = tr.iou_table(f["boxes"], f["classes"], f["masks"]), tr.iou_table_scalar(f["boxes"], f["classes"], f["masks"])
        assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
        seen += int((a > tr.threshold).sum())
        tr.update(f["boxes"], f["classes"], f["masks"])
    assert seen > 0 and len({t["id"] for t in tr.tracks}) == len(tr.tracks)


def test_pack_words_by_hand():
    m = np.zeros((1, 5, 13), dtype=bool)                               # 65 pixels: one full word and one bit
    m[0, 0, 0] = m[0, 4, 11] = m[0, 4, 12] = True                      # pixels 0, 63, 64
    assert V.pack_words(m).tolist() == [[-2 ** 63 + 1, 1]]


# ---- the library -----------------------------------------------------------------------------------------------------------------------
NEW = ("cmk_vis_track_iou_boxes", "cmk_vis_track_assign", "cmk_vis_track_gather", "cmk_vis_prepare_ids")


def test_header_and_signatures_agree():
    from centermask2_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cmk.h")).read()
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), name
        for a, ct in zip(args, argtypes):
            want = ctypes.c_void_p if "*" in a else (ctypes.c_double if a.startswith("double") else ctypes.c_int)
            assert ct is want, (name, a)
        assert hasattr(lib, name)
    assert lib.cmk_version() == 5                                       # additive entries, as cmk_pack_records_kp was


def test_track_abi_argument_validation_without_gpu():
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 65536)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    q, r = p + 16384, p + 32768

    def iou(old=p, rows=2, new=p, n=2, out=q):
        return lib.cmk_vis_track_iou_boxes(old, rows, new, n, out, None), lib.cmk_last_error()

    for kw, msg in (({"old": None}, b"null"), ({"new": None}, b"null"), ({"out": None}, b"null"), ({"rows": -1}, b"rows"), ({"rows": 1025}, b"rows"),
                    ({"n": -1}, b"instances"), ({"n": 1025}, b"instances")):
        rc, err = iou(**kw)
        assert rc == -1 and msg in err and b"vis_track_iou_boxes" in err, (kw, rc, err)
    assert iou(rows=0, old=None)[0] == 0 and iou(n=0, new=None)[0] == 0             # nothing to compare: no launch

    def assign(iou=p, inter=None, oa=None, na=None, rows=2, ob=p, oc=p, oi=p, ot=p, nb=p, nc=p, n=2, cap=4, ttl=8, thr=0.6, xb=q, xc=q, xi=q, xt=q,
               src=r, ids=r, cnt=r):
        rc = lib.cmk_vis_track_assign(iou, inter, oa, na, rows, ob, oc, oi, ot, nb, nc, n, cap, ttl, thr, xb, xc, xi, xt, src, ids, cnt, None)
        return rc, lib.cmk_last_error()

    for kw, msg in (({"ob": None}, b"null"), ({"oc": None}, b"null"), ({"oi": None}, b"null"), ({"ot": None}, b"null"), ({"nb": None}, b"null"),
                    ({"nc": None}, b"null"), ({"xb": None}, b"null"), ({"xc": None}, b"null"), ({"xi": None}, b"null"), ({"xt": None}, b"null"),
                    ({"src": None}, b"null"), ({"ids": None}, b"null"), ({"cnt": None}, b"null"),
                    ({"iou": None}, b"exactly one"), ({"inter": p}, b"exactly one"), ({"iou": None, "inter": p}, b"null"),
                    ({"iou": None, "inter": p, "oa": p}, b"null"), ({"iou": None, "inter": p, "na": p}, b"null"),
                    ({"cap": 0}, b"max_tracks"), ({"cap": 1025, "n": 2}, b"max_tracks"), ({"n": 5}, b"instances"), ({"n": -1}, b"instances"),
                    ({"rows": 5}, b"rows"), ({"rows": -1}, b"rows"), ({"ttl": 0}, b"ttl"), ({"ttl": 256}, b"ttl"),
                    ({"thr": -0.1}, b"threshold"), ({"thr": 1.5}, b"threshold"), ({"thr": float("nan")}, b"threshold"),
                    ({"xb": p}, b"out of place"), ({"xc": p}, b"out of place"), ({"xi": p}, b"out of place"), ({"xt": p}, b"out of place")):
        rc, err = assign(**kw)
        assert rc == -1 and msg in err and b"vis_track_assign" in err, (kw, rc, err)

    def gather(src=r, cnt=r, ow=p, oa=p, nw=q, na=q, n=2, rows=4, cap=4, h=5, w=7, xw=r + 4096, xa=r + 8192):
        return lib.cmk_vis_track_gather(src, cnt, ow, oa, nw, na, n, rows, cap, h, w, xw, xa, None), lib.cmk_last_error()

    for kw, msg in (({"src": None}, b"null"), ({"cnt": None}, b"null"), ({"ow": None}, b"null"), ({"oa": None}, b"null"), ({"nw": None}, b"null"),
                    ({"na": None}, b"null"), ({"xw": None}, b"null"), ({"xa": None}, b"null"),
                    ({"h": 0}, b"at least 1"), ({"w": -2}, b"at least 1"), ({"h": 46341, "w": 46341}, b"int32"), ({"h": 1, "w": 2 ** 31 - 1}, b"int32"),
                    ({"cap": 0}, b"max_tracks"), ({"cap": 1025}, b"max_tracks"), ({"n": 5}, b"instances"), ({"rows": 5}, b"rows"),
                    ({"xw": p}, b"out of place"), ({"xw": p + 24}, b"out of place"), ({"xw": q + 8}, b"out of place"), ({"xa": p + 12}, b"out of place")):
        rc, err = gather(**kw)
        assert rc == -1 and msg in err and b"vis_track_gather" in err, (kw, rc, err)
    assert gather(rows=0)[0] == 0                                       # an empty table before and after: no launch

    def prepare_ids(boxes=p, scores=p, classes=p, order=p, names=p, lens=p, num_names=1, pal=p, n=1, h=4, w=4, fs=1, ids=p, rec=q):
        rc = lib.cmk_vis_prepare_ids(boxes, scores, classes, order, names, lens, num_names, pal, n, h, w, fs, 0, ids, rec, None)
        return rc, lib.cmk_last_error()

    for kw, msg in (({"boxes": None}, b"null"), ({"scores": None}, b"null"), ({"classes": None}, b"null"), ({"order": None}, b"null"),
                    ({"names": None}, b"null"), ({"lens": None}, b"null"), ({"pal": None}, b"null"), ({"rec": None}, b"null"),
                    ({"h": 0}, b"at least 1"), ({"h": 65536, "w": 65536}, b"int32"), ({"n": -1}, b"65535"), ({"n": 65536}, b"65535"),
                    ({"fs": 0}, b"font_scale"), ({"fs": 17}, b"font_scale"), ({"num_names": -1}, b"names")):
        rc, err = prepare_ids(**kw)
        assert rc == -1 and msg in err and b"vis_prepare_ids" in err, (kw, rc, err)
    assert prepare_ids(n=0, boxes=None, rec=None, ids=None)[0] == 0


def test_wrappers_and_classes_refuse_on_the_host():
    from centermask2_amd import ops
    from centermask2_amd._lib import CmkError
    from centermask2_amd.structures import Boxes, Instances
    from centermask2_amd.video import InstanceTracker, VideoVisualizer
    cap = 4
    half = lambda: dict(boxes=torch.zeros((cap, 4)), classes=torch.zeros(cap, dtype=torch.int64), ids=torch.zeros(cap, dtype=torch.int32),
                        ttl=torch.zeros(cap, dtype=torch.int32), words=torch.zeros((cap, 1), dtype=torch.int64), areas=torch.zeros(cap, dtype=torch.int32))
    nb, nc = torch.zeros((2, 4)), torch.zeros(2, dtype=torch.int64)
    src, cnt = torch.zeros(cap, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(CmkError, match="vis_track_iou_boxes.*old_boxes"):
        ops.vis_track_iou_boxes(torch.zeros((cap, 4)), 2, nb, torch.zeros(16, dtype=torch.float64))
    with pytest.raises(CmkError, match="rows = 5"):
        ops.vis_track_iou_boxes(torch.zeros((cap, 4)), 5, nb, torch.zeros(16, dtype=torch.float64))
    with pytest.raises(CmkError, match="vis_track_assign.*old.boxes"):
        ops.vis_track_assign(half(), half(), nb, nc, 2, 8, 0.6, src, cnt, iou=torch.zeros(16, dtype=torch.float64))
    with pytest.raises(CmkError, match=r"5 instances \(boxes \(5, 4\)\)"):
        ops.vis_track_assign(half(), half(), torch.zeros((5, 4)), torch.zeros(5, dtype=torch.int64), 2, 8, 0.6, src, cnt)
    with pytest.raises(CmkError, match="ttl = 0"):
        ops.vis_track_assign(half(), half(), nb, nc, 2, 0, 0.6, src, cnt)
    with pytest.raises(CmkError, match="vis_track_gather.*old.words"):
        ops.vis_track_gather(src, cnt, half(), half(), torch.zeros((2, 1), dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 4, 5, 7)
    with pytest.raises(CmkError, match="int32 positions"):
        ops.vis_track_gather(src, cnt, half(), half(), torch.zeros((2, 1), dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 4, 46341, 46341)
    with pytest.raises(CmkError, match="vis_prepare_ids.*boxes"):
        ops.vis_prepare_ids(nb, torch.zeros(2), nc, nc, torch.zeros((1, 32), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), 0,
                            torch.zeros((64, 3), dtype=torch.uint8), 6, 8, 1, False, torch.zeros(2, dtype=torch.int32))

    for kw in ({"match": "iou"}, {"iou_threshold": 1.5}, {"iou_threshold": -0.1}, {"ttl": 0}, {"ttl": 256}, {"ttl": 2.5}, {"max_tracks": 0},
               {"max_tracks": 1025}):
        with pytest.raises(CmkError):
            InstanceTracker(**kw)
        with pytest.raises(CmkError):
            VideoVisualizer(**kw)
    assert InstanceTracker().iou_threshold == 0.6 and InstanceTracker(match="mask").iou_threshold == 0.5 and InstanceTracker().ttl == 8
    assert InstanceTracker().max_tracks == 256 and InstanceTracker().dropped == 0 and InstanceTracker().table() == {}
    inst = Instances((6, 8), pred_boxes=Boxes(torch.tensor([[1.0, 1.0, 5.0, 4.0]] * 3)), scores=torch.ones(3), pred_classes=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(CmkError, match=r"cpu.*\(3, 4\)"):
        InstanceTracker().update(inst)
    with pytest.raises(CmkError, match="pred_masks"):
        InstanceTracker(match="mask").update(inst)
    with pytest.raises(CmkError, match=r"3 instances \(boxes \(3, 4\)\) but max_tracks = 2"):
        InstanceTracker(max_tracks=2).update(inst)
    with pytest.raises(CmkError, match="pred_boxes"):
        InstanceTracker().update(Instances((6, 8)))
    with pytest.raises(CmkError, match=r"cpu.*\(3, 4\)"):
        VideoVisualizer().draw(torch.zeros((6, 8, 3), dtype=torch.uint8), inst)
    tr = InstanceTracker()
    tr.reset()                                                          # a reset before the first frame is fine
    assert tr.n_tracks == 0 and tr.next_id == 0


def test_exports():
    import centermask2_amd
    from centermask2_amd import InstanceTracker, VideoVisualizer, Visualizer, video
    assert InstanceTracker is video.InstanceTracker and VideoVisualizer is video.VideoVisualizer and issubclass(VideoVisualizer, Visualizer)
    assert "InstanceTracker" in centermask2_amd.__all__ and "VideoVisualizer" in centermask2_amd.__all__
    assert isinstance(VideoVisualizer(match="mask", ttl=3, max_tracks=16, alpha=0.25).tracker, InstanceTracker)
