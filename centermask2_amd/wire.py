"""Result wire formats of the reference's tooling, host side, no third-party dependency.

* the six `.bin` files per image of the Ascend flow (postprocess_bin_outputs.py:36-45): `<name>_1.bin` .. `_6.bin` =
  locations f32 (-1,2), mask_scores f32 (-1), pred_boxes f32 (-1,4), pred_classes i64 (-1), pred_masks f32 (-1,1,28,28),
  scores f32 (-1) — the order of single_flatten_to_tuple (deploy_utils.py:117-126);
* COCO result json (evaluation/coco_evaluation.py:362-427): XYWH boxes, compressed RLE segmentation, `mask_score`, and the rule
  that segm AP is ranked by `mask_score` (:557-563).
pycocotools is absent here, so the RLE codec below restates its published algorithm (maskApi.c rleEncode / rleToString:
column-major runs starting with a zero run, 5-bit groups with a continuation bit, delta coding from the third count on);
it is checked by round trip only ("parity unpinned" for the exact bytes).  The same codec runs on the device for GPU bitmasks
(csrc/rle.hip through ops.mask_rle), held to byte equality with the host functions here, which stay the reference and the CPU path.
"""
import os
from typing import Dict, List, Tuple

import numpy as np
import torch

BIN_DTYPES = ("float32", "float32", "float32", "int64", "float32", "float32")
BIN_SHAPES = ((-1, 2), (-1,), (-1, 4), (-1,), (-1, 1, 28, 28), (-1,))


def to_bin(tuple6, prefix: str) -> List[str]:
    """tuple6 = (locations, mask_scores, pred_boxes, pred_classes, pred_masks, scores); writes prefix_1.bin .. prefix_6.bin."""
    paths = []
    for i, (t, dt) in enumerate(zip(tuple6, BIN_DTYPES)):
        path = "{}_{}.bin".format(prefix, i + 1)
        np.ascontiguousarray(t.detach().cpu().numpy().astype(dt)).tofile(path)
        paths.append(path)
    return paths


def from_bin(prefix: str) -> tuple:
    out = []
    for i, (dt, shp) in enumerate(zip(BIN_DTYPES, BIN_SHAPES)):
        out.append(torch.from_numpy(np.fromfile("{}_{}.bin".format(prefix, i + 1), dtype=dt).reshape(shp)))
    return tuple(out)


def rle_counts(mask: np.ndarray) -> List[int]:
    """Run lengths of the column-major flattening, starting with the zeros run (possibly 0 long)."""
    flat = np.asarray(mask, dtype=np.uint8).reshape(-1, order="F")
    if flat.size == 0:
        return []
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    bounds = np.concatenate(([0], change, [flat.size]))
    counts = np.diff(bounds).tolist()
    if flat[0] == 1:
        counts = [0] + counts
    return counts


def rle_to_string(counts: List[int]) -> str:
    s = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(chr(c + 48))
    return "".join(s)


def rle_from_string(s: str) -> List[int]:
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_encode(mask) -> Dict:
    m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": rle_to_string(rle_counts(m))}


def rle_encode_batch(masks) -> List[Dict]:
    """(n,H,W) bitmasks -> one RLE dict each.  Bool bitmasks on a GPU are encoded there (ops.mask_rle: the bitmaps are not downloaded);
    anything else (CPU tensors, NumPy arrays) goes through rle_encode mask by mask.  Both give the same bytes."""
    if torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.bool and masks.dim() == 3:
        from . import ops
        size = [int(masks.shape[1]), int(masks.shape[2])]
        return [{"size": list(size), "counts": s} for s in ops.mask_rle(masks)[1]]
    return [rle_encode(m) for m in masks]


def rle_decode(rle: Dict) -> np.ndarray:
    h, w = rle["size"]
    counts = rle_from_string(rle["counts"])
    flat = np.zeros(h * w, dtype=np.uint8)
    pos, val = 0, 0
    for c in counts:
        flat[pos:pos + c] = val
        pos += c
        val ^= 1
    return flat.reshape((h, w), order="F").astype(bool)


def mask_contours_host(mask) -> List[np.ndarray]:
    """One (H,W) binary mask -> its contours, the host reference of ops.mask_contours and the path for CPU tensors and arrays: a list
    of (k,2) int32 arrays of lattice vertices (x, y), 0 <= x <= W, 0 <= y <= H, pixel (r, c) being the square [c, c+1] x [r, r+1] and
    everything outside the image background (DESIGN §3 "Contours").  Every unit edge between a set and an unset pixel is walked once
    with the foreground on the right (y down: a set pixel's top edge runs +x, its right edge +y); foreground is 4-connected, at a
    saddle vertex the walk turns right.  Only corners are kept.  A loop starts at its smallest vertex in (y, x) order and the loops are
    sorted by start; outer boundaries have a positive doubled area (contour_area2), holes a negative one.  An empty mask has no loop.
    The same steps as the device: corner records in lattice row-major order, links along rows and columns, pointer jumping."""
    m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask_contours_host: expected one (H,W) mask, got shape {}".format(tuple(m.shape)))
    h, w = m.shape
    p = np.zeros((h + 2, w + 2), dtype=bool)
    p[1:-1, 1:-1] = m != 0
    nw, ne, sw, se = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]         # the 2x2 pixels around vertex [y, x]
    saddle = (ne ^ nw) & (se ^ sw) & (ne ^ se)
    cnt = (nw ^ ne ^ sw ^ se).astype(np.int64) + 2 * saddle
    ys, xs = np.nonzero(cnt)                                                # lattice row-major
    reps = cnt[ys, xs]
    t = int(reps.sum())
    if t == 0:
        return []
    y, x = np.repeat(ys, reps), np.repeat(xs, reps)
    sub = np.arange(t) - np.repeat(np.cumsum(reps) - reps, reps)            # 0, or 0 and 1 for the two passes of a saddle
    a, b, c, d, sad = nw[y, x], ne[y, x], sw[y, x], se[y, x], saddle[y, x]
    # out direction: 0 +x, 1 +y, 2 -x, 3 -y.  At a saddle the pass whose horizontal edge lies to the left comes first.
    out = np.select([d & ~b, c & ~d, a & ~c], [0, 1, 2], 3)
    out = np.where(sad, np.where(a, np.where(sub == 0, 2, 0), np.where(sub == 0, 1, 3)), out)
    idx = np.arange(t)
    # the corners of a lattice row pair up (2m, 2m+1) into its horizontal segments; those of a column, sorted by y with the pass of a
    # saddle whose vertical edge lies above first, into its vertical segments
    col_sub = np.where(sad & ~a, 1 - sub, sub)
    order = np.lexsort((col_sub, y, x))
    pos = np.empty(t, dtype=np.int64)
    pos[order] = idx
    succ = np.where((out == 0) | (out == 2), idx ^ 1, order[pos ^ 1])
    # pointer jumping: the smallest record of the loop (its canonical start) and the steps to it
    lab, dist, s, hop = idx.copy(), np.zeros(t, dtype=np.int64), succ.copy(), 1
    while hop < t:
        better = lab[s] < lab
        dist = np.where(better, hop + dist[s], dist)
        lab = np.where(better, lab[s], lab)
        s = s[s]
        hop *= 2
    length = np.zeros(t, dtype=np.int64)
    leaders = np.flatnonzero(lab == idx)
    length[leaders] = 1 + dist[succ[leaders]]
    lo = np.cumsum(length) - length
    place = lo[lab] + np.where(dist == 0, 0, length[lab] - dist)
    xy = np.empty((t, 2), dtype=np.int32)
    xy[place, 0], xy[place, 1] = x, y
    return [xy[o:o + n].copy() for o, n in zip(lo[leaders].tolist(), length[leaders].tolist())]


def contour_area2(loop) -> int:
    """Twice the signed area of a closed loop of (x, y) vertices: sum(x_i*y_{i+1} - x_{i+1}*y_i); positive for an outer boundary."""
    v = np.asarray(loop, dtype=np.int64).reshape(-1, 2)
    nx, ny = np.roll(v[:, 0], -1), np.roll(v[:, 1], -1)
    return int((v[:, 0] * ny - nx * v[:, 1]).sum())


def contours_to_polygons(loops) -> List[List[float]]:
    """The loops of one mask -> COCO polygons: the outer boundaries (positive area) as flat lists [x0, y0, x1, y1, ..] of floats, in
    the same order.  Holes are dropped, as a COCO polygon list and detectron2's mask_to_polygons cannot hold them: a mask with holes
    rasterises back with its holes filled."""
    return [np.asarray(lp, dtype=np.float64).reshape(-1).tolist() for lp in loops if contour_area2(lp) > 0]


def polygon_encode_batch(masks) -> List[List[List[float]]]:
    """(n,H,W) bitmasks -> the COCO polygon list of each (contours_to_polygons: no holes).  Bool bitmasks on a GPU are traced there
    (ops.mask_contours: the bitmaps are not downloaded); anything else (CPU tensors, NumPy arrays) goes through mask_contours_host
    mask by mask.  Both give the same lists."""
    if torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.bool and masks.dim() == 3:
        from . import ops
        return [contours_to_polygons(loops) for loops in ops.mask_contours(masks)]
    return [contours_to_polygons(mask_contours_host(m)) for m in masks]


def instances_to_coco_json(instances, img_id: int, segmentation: str = "rle") -> List[Dict]:
    """coco_evaluation.py:362-427 for post-processed Instances (pred_masks = (n,H,W) bool bitmasks).  segmentation: "rle" (the
    reference's compressed RLE dict) or "polygon" (COCO's other form: the list of outer-boundary polygons of polygon_encode_batch,
    [] for an empty mask; holes are not represented)."""
    if segmentation not in ("rle", "polygon"):
        raise ValueError("instances_to_coco_json: segmentation is {!r}; the choices are 'rle' and 'polygon'".format(segmentation))
    n = len(instances)
    if n == 0:
        return []
    boxes = instances.pred_boxes.tensor.detach().cpu().clone()
    boxes[:, 2] -= boxes[:, 0]          # XYXY_ABS -> XYWH_ABS
    boxes[:, 3] -= boxes[:, 1]
    boxes = boxes.tolist()
    scores = instances.scores.tolist()
    classes = instances.pred_classes.tolist()
    encode = rle_encode_batch if segmentation == "rle" else polygon_encode_batch
    rles = encode(instances.pred_masks) if instances.has("pred_masks") else None
    mask_scores = instances.mask_scores.tolist() if instances.has("mask_scores") else None
    keypoints = None
    if instances.has("pred_keypoints"):        # coco_evaluation.py:418-425: COCO's keypoint coordinates are pixel indices
        kp = instances.pred_keypoints.detach().cpu().clone()
        kp[:, :, :2] -= 0.5
        keypoints = kp.flatten(1).tolist()      # x, y, score per keypoint
    results = []
    for k in range(n):
        r = {"image_id": img_id, "category_id": classes[k], "bbox": boxes[k], "score": scores[k]}
        if rles is not None:
            r["segmentation"] = rles[k]
            if mask_scores is not None:
                r["mask_score"] = mask_scores[k]
        if keypoints is not None:
            r["keypoints"] = keypoints[k]
        results.append(r)
    return results


def segm_results_ranked_by_mask_score(coco_results: List[Dict]) -> List[Dict]:
    """coco_evaluation.py:551-563: for segm AP drop `bbox` and let `mask_score` replace `score`."""
    out = []
    for c in coco_results:
        c = dict(c)
        c.pop("bbox", None)
        if "mask_score" in c:
            c["score"] = c.pop("mask_score")
        out.append(c)
    return out
