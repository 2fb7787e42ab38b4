"""Mask contours without a GPU: wire.mask_contours_host against the worked examples of DESIGN §3 "Contours" and against the serial edge
follower of tests/contour_ref.py, the properties of the contract on seeded masks, the round trip through the package's own polygon
rasteriser, the polygon form of the COCO results, and the argument checks of the C entries (the library loads without a device).
Everything is integer geometry: every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from centermask2_amd import coco_eval, wire
from centermask2_amd.structures import Boxes, Instances
from . import contour_ref as R

NEW = ("cmk_vis_contour_ws_bytes", "cmk_vis_contour_count", "cmk_vis_contour_trace_ws_bytes", "cmk_vis_contour_trace")


def host(mask):
    loops = wire.mask_contours_host(np.asarray(mask))
    for lp in loops:
        assert isinstance(lp, np.ndarray) and lp.dtype == np.int32 and lp.ndim == 2 and lp.shape[1] == 2
    return R.as_lists(loops)


@pytest.fixture(scope="module")
def seeded():
    """50 seeded masks of 1..40 x 1..40, blobs and noise in turn, each with the reference's loops: computed once."""
    masks = R.random_masks(20261020, 50, 1, 40)
    return [(m, R.contours(m)) for m in masks]


HOLE33 = np.ones((3, 3), dtype=int)
HOLE33[1, 1] = 0
HOLE44 = np.ones((4, 4), dtype=int)
HOLE44[1, 1] = HOLE44[2, 2] = 0
WORKED = [
    ([[1]], [[(0, 0), (1, 0), (1, 1), (0, 1)]]),
    ([[1, 0], [0, 1]], [[(0, 0), (1, 0), (1, 1), (0, 1)], [(1, 1), (2, 1), (2, 2), (1, 2)]]),
    ([[0, 1], [1, 0]], [[(1, 0), (2, 0), (2, 1), (1, 1)], [(0, 1), (1, 1), (1, 2), (0, 2)]]),
    (HOLE33, [[(0, 0), (3, 0), (3, 3), (0, 3)], [(1, 1), (1, 2), (2, 2), (2, 1)]]),
    (HOLE44, [[(0, 0), (4, 0), (4, 4), (0, 4)], [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 2), (2, 2), (2, 1)]]),
    (np.ones((2, 3), dtype=int), [[(0, 0), (3, 0), (3, 2), (0, 2)]]),
    (np.zeros((4, 5), dtype=int), []),
    ([[1, 0], [1, 1]], [[(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (0, 2)]]),           # an L: 6 corners
]


@pytest.mark.parametrize("k", range(len(WORKED)))
def test_worked_examples_by_hand(k):
    mask, want = WORKED[k]
    assert host(mask) == want
    assert R.contours(np.asarray(mask)) == want                    # the restatement gives the same: both are pinned by hand


def test_worked_areas():
    assert [R.area2(lp) for lp in host(HOLE33)] == [18, -2]
    assert [R.area2(lp) for lp in host(HOLE44)] == [32, -4]
    assert [wire.contour_area2(lp) for lp in wire.mask_contours_host(HOLE44)] == [32, -4]


def test_host_equals_the_serial_follower(seeded):
    for m, want in seeded:
        assert host(m) == want, m.shape
    board = (np.indices((8, 8)).sum(0) % 2).astype(bool)
    assert host(board) == R.contours(board) and len(host(board)) == 32
    t = torch.from_numpy(seeded[0][0])
    assert R.as_lists(wire.mask_contours_host(t)) == seeded[0][1]                   # CPU tensors take the same path


def test_properties_of_the_contract(seeded):
    for m, _ in seeded:
        h, w = m.shape
        loops = host(m)
        assert (R.fill_even_odd(loops, h, w) == m).all()
        assert sum(R.area2(lp) for lp in loops) == 2 * int(m.sum())
        starts = [(lp[0][1], lp[0][0]) for lp in loops]
        assert starts == sorted(starts) and len(set(starts)) == len(starts)
        for lp in loops:
            n = len(lp)
            assert n >= 4 and n % 2 == 0
            assert all(0 <= x <= w and 0 <= y <= h for x, y in lp)
            horiz = [lp[i][1] == lp[(i + 1) % n][1] for i in range(n)]
            for i in range(n):
                (x0, y0), (x1, y1) = lp[i], lp[(i + 1) % n]
                assert (x0 == x1) != (y0 == y1)                                      # exactly one coordinate changes
                assert horiz[i] != horiz[(i + 1) % n]                                # H and V alternate: no three collinear vertices
            assert min(range(n), key=lambda i: (lp[i][1], lp[i][0])) == 0
            assert (lp[0][1], lp[0][0]) < min((y, x) for x, y in lp[1:])            # the start is the minimum and is met once
            assert R.area2(lp) != 0


def test_polygons_round_trip_through_the_rasteriser():
    """Polygons drop holes: coco_eval's rleFrPoly restatement gives back the mask with its holes filled (background 8-connected)."""
    masks = [m for m in R.random_masks(7, 80, 5, 39)[::2]]                          # the 40 blob masks
    holes = 0
    for m in masks:
        h, w = m.shape
        loops = wire.mask_contours_host(m)
        polys = wire.contours_to_polygons(loops)
        assert len(polys) == sum(1 for lp in loops if R.area2(R.as_lists([lp])[0]) > 0)
        assert all(isinstance(v, float) for p in polys for v in p)
        filled = R.fill_holes(m)
        holes += int((filled != m).any())
        if not polys:
            assert not m.any()
            continue
        counts = coco_eval.segmentation_to_counts(polys, h, w)
        got = wire.rle_decode({"size": [h, w], "counts": wire.rle_to_string(counts)})
        assert (got == filled).all(), (h, w)
    assert holes > 0, "no mask of the set has a hole"


def test_polygon_batch_on_host_inputs():
    masks = np.stack([np.pad(np.ones((3, 4), dtype=bool), 2), np.zeros((7, 8), dtype=bool)])
    want = [[[2.0, 2.0, 6.0, 2.0, 6.0, 5.0, 2.0, 5.0]], []]
    assert wire.polygon_encode_batch(masks) == want
    assert wire.polygon_encode_batch(torch.from_numpy(masks)) == want


def instances(masks):
    n, h, w = masks.shape
    boxes = torch.tensor([[1.0, 2.0, 5.5, 7.0]] * n)
    return Instances((h, w), pred_boxes=Boxes(boxes), scores=torch.linspace(0.9, 0.5, n), pred_classes=torch.arange(n),
                     pred_masks=torch.from_numpy(masks), mask_scores=torch.linspace(0.8, 0.4, n))


def test_coco_json_segmentation_forms():
    m = np.zeros((3, 9, 11), dtype=bool)
    m[0, 2:6, 3:9] = True
    m[0, 3:5, 4:6] = False                                                          # a hole: not in the polygon
    m[2, 0, 0] = m[2, 8, 10] = True
    inst = instances(m)
    default = wire.instances_to_coco_json(inst, 7)
    assert default == wire.instances_to_coco_json(inst, 7, segmentation="rle")
    assert default[0]["segmentation"] == wire.rle_encode(m[0])
    poly = wire.instances_to_coco_json(inst, 7, segmentation="polygon")
    assert [r["segmentation"] for r in poly] == [[[3.0, 2.0, 9.0, 2.0, 9.0, 6.0, 3.0, 6.0]], [],
                                                 [[0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0], [10.0, 8.0, 11.0, 8.0, 11.0, 9.0, 10.0, 9.0]]]
    for a, b in zip(default, poly):
        assert {k: v for k, v in a.items() if k != "segmentation"} == {k: v for k, v in b.items() if k != "segmentation"}
        assert "mask_score" in b
    with pytest.raises(ValueError, match="'rle' and 'polygon'"):
        wire.instances_to_coco_json(inst, 7, segmentation="polygons")


def test_header_and_signatures_agree():
    from centermask2_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cmk.h")).read()
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"\b(int|int64_t) " + name + r"\s*\(([^;]*)\);", header)
        assert m, name
        args = [a.strip() for a in m.group(2).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else ctypes.c_int64) and len(argtypes) == len(args), name
        for a, ct in zip(args, argtypes):
            want = ctypes.c_void_p if "*" in a else (ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int)
            assert ct is want, (name, a)
        assert hasattr(lib, name)
    assert lib.cmk_version() == 5                                                   # additive entries


def test_contour_abi_argument_validation_without_gpu():
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * (1 << 20))()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    H, W, Rn = 5, 7, 2
    need = lib.cmk_vis_contour_ws_bytes(Rn, H, W)
    assert need == 8 * (Rn + 1) + 8 * Rn + 4 * Rn * (H + 1) * 1                    # offsets, block totals, one int32 per lattice row word
    assert lib.cmk_vis_contour_ws_bytes(Rn, 13, 130) == 8 * 3 + 8 * 2 + 4 * 2 * 14 * 3
    assert lib.cmk_vis_contour_ws_bytes(1, 800, 1280) == 8 * 2 + 8 * 17 + 4 * 801 * 21
    for bad in ((-1, H, W), (65536, H, W), (Rn, 0, W), (Rn, H, 0), (Rn, 65536, 32768)):
        assert lib.cmk_vis_contour_ws_bytes(*bad) == 0
    assert lib.cmk_vis_contour_trace_ws_bytes(-2) == 0 and lib.cmk_vis_contour_trace_ws_bytes(0) == 0
    assert lib.cmk_vis_contour_trace_ws_bytes(8) >= 8 * 16
    words, ws, nc, scratch, xy, head = p, p + 4096, p + 8192, p + 16384, p + 65536, p + 131072
    n_ok = (ctypes.c_int32 * Rn)(4, 8)
    sbytes = lib.cmk_vis_contour_trace_ws_bytes(12)

    def count(words=words, R=Rn, H=H, W=W, ws=ws, ws_bytes=need, nc=nc):
        return lib.cmk_vis_contour_count(words, R, H, W, ws, ws_bytes, nc, None), lib.cmk_last_error()

    for kw, msg in (({"words": None}, b"null"), ({"ws": None}, b"null"), ({"nc": None}, b"null"), ({"H": 0}, b"at least 1"),
                    ({"W": 0}, b"at least 1"), ({"H": 65536, "W": 32768}, b"int32"), ({"R": -1}, b"65535"), ({"R": 65536}, b"65535"),
                    ({"ws_bytes": need - 1}, b"workspace"), ({"ws": ws + 4}, b"aligned"), ({"nc": words}, b"overlaps"),
                    ({"ws": words + 8}, b"overlaps"), ({"nc": ws + 8}, b"overlaps")):
        rc, err = count(**kw)
        assert rc == -1 and msg in err and b"vis_contour_count" in err, (kw, rc, err)
    assert count(R=0, words=None, ws=None, nc=None)[0] == 0

    def trace(words=words, R=Rn, H=H, W=W, ws=ws, ws_bytes=need, n=n_ok, scratch=scratch, sbytes=sbytes, xy=xy, head=head):
        rc = lib.cmk_vis_contour_trace(words, R, H, W, ws, ws_bytes, ctypes.addressof(n) if n is not None else None, scratch, sbytes, xy, head, None)
        return rc, lib.cmk_last_error()

    i32 = ctypes.c_int32 * Rn
    for kw, msg in (({"words": None}, b"null"), ({"ws": None}, b"null"), ({"n": None}, b"null"), ({"scratch": None}, b"null"),
                    ({"xy": None}, b"null"), ({"head": None}, b"null"), ({"H": 0}, b"at least 1"), ({"W": -3}, b"at least 1"),
                    ({"H": 65536, "W": 32768}, b"int32"), ({"R": -1}, b"65535"), ({"R": 65536}, b"65535"),
                    ({"ws_bytes": need - 1}, b"workspace"), ({"n": i32(4, -2)}, b"negative or odd"), ({"n": i32(5, 7)}, b"negative or odd"),
                    ({"n": i32(2 ** 31 - 2, 2 ** 31 - 2)}, b"fit int32"), ({"sbytes": sbytes - 1}, b"scratch"),
                    ({"scratch": scratch + 8}, b"aligned"), ({"xy": words}, b"overlaps"), ({"head": ws + 16}, b"overlaps"),
                    ({"scratch": words}, b"overlaps"), ({"xy": head - 8}, b"overlap"), ({"head": scratch + 16}, b"overlap")):
        rc, err = trace(**kw)
        assert rc == -1 and msg in err and b"vis_contour_trace" in err, (kw, rc, err)
    assert trace(R=0, words=None, ws=None, n=None, scratch=None, xy=None, head=None)[0] == 0
    assert trace(n=i32(0, 0), scratch=None, xy=None, head=None)[0] == 0             # nothing to trace: no launch
