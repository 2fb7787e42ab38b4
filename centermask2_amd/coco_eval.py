"""COCO detection scoring on the host (NumPy, float64): the protocol behind evaluation.COCOEvaluator.

pycocotools is absent here.  This module restates its published algorithm — COCOeval's evaluateImg / accumulate / summarize for
iouType "bbox" and "segm", and maskApi.c's rleFrPoly for polygon ground truth — from the published sources, as wire.py restates the RLE
codec.  It has never been run beside a real pycocotools: the numbers are checked against hand-computed cases, against
evaluation.average_precision where the two protocols coincide, and the rasteriser against properties of rectangles and a triangle
(tests/test_cpu_coco_eval.py).  "Parity unpinned" applies to every tie-breaking detail below.

The IoU of masks is formed here from integer counts (pixels in both, pixels in each); where those counts come from is the caller's
business: ops.mask_intersections for bitmasks on a GPU, intersections_host for bitmasks on the host.  Nothing here touches a bitmap
after the counts exist.

iouType "boundary" (Boundary AP; Cheng et al., "Boundary IoU", CVPR 2021) is the same protocol with IoU = min(mask IoU, IoU of the mask
boundaries).  boundary_host restates the rule from the publication and is unpinned against the real boundary-iou-api in the same way.
"""
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import wire

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))       # all, small, medium, large
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


# ---- ground-truth segmentations -> COCO run lengths -------------------------------------------------------------------------------

def counts_to_mask(counts: Sequence[int], h: int, w: int) -> np.ndarray:
    """(h,w) uint8 bitmask whose column-major runs are `counts` (zeros run first)."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.size == 0 or (counts < 0).any() or int(counts.sum()) != h * w:
        raise ValueError("runs add up to {}, not to {}x{}".format(int(counts.sum()), h, w))
    flat = np.repeat(np.arange(counts.size, dtype=np.int64) & 1, counts).astype(np.uint8)
    return flat.reshape((h, w), order="F")


def poly_to_counts(xy: Sequence[float], h: int, w: int) -> List[int]:
    """One polygon [x0, y0, x1, y1, ..] -> COCO run lengths of its (h,w) rasterisation: maskApi.c rleFrPoly restated.  The polygon is
    scaled by 5 and rounded, every edge walked densely along its longer axis, the points kept where the upsampled x changes and the
    change lands on a pixel-column boundary, y clamped to [0, h] and ceiled, the positions x*h + y sorted, their differences are the
    run lengths, and zero-length runs are merged away."""
    scale = 5.0
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    k = xy.shape[0]
    px = np.trunc(scale * xy[:, 0] + 0.5).astype(np.int64)        # (int)(scale*x + .5): C truncation
    py = np.trunc(scale * xy[:, 1] + 0.5).astype(np.int64)
    px, py = np.append(px, px[0]), np.append(py, py[0])
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = int(px[j]), int(px[j + 1]), int(py[j]), int(py[j + 1])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx == 0 and dy == 0:                                     # a repeated vertex: one point (the C code divides 0 by 0 here)
            us.append(np.array([xs], dtype=np.int64))
            vs.append(np.array([ys], dtype=np.int64))
            continue
        if dx >= dy:
            s = (ye - ys) / dx
            t = np.arange(dx + 1, dtype=np.int64)
            if flip:
                t = dx - t
            us.append(t + xs)
            vs.append(np.trunc(ys + s * t + 0.5).astype(np.int64))
        else:
            s = (xe - xs) / dy
            t = np.arange(dy + 1, dtype=np.int64)
            if flip:
                t = dy - t
            vs.append(t + ys)
            us.append(np.trunc(xs + s * t + 0.5).astype(np.int64))
    u, v = np.concatenate(us), np.concatenate(vs)
    # points along the y-boundary, downsampled
    j = np.flatnonzero(u[1:] != u[:-1]) + 1
    xd = np.where(u[j] < u[j - 1], u[j], u[j] - 1).astype(np.float64)
    xd = (xd + 0.5) / scale - 0.5
    yd = np.minimum(v[j], v[j - 1]).astype(np.float64)
    yd = (yd + 0.5) / scale - 0.5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    xd, yd = xd[keep], np.ceil(np.clip(yd[keep], 0.0, float(h)))
    a = np.sort(np.append(xd.astype(np.int64) * h + yd.astype(np.int64), h * w))
    a = np.diff(np.concatenate(([0], a))).tolist()
    # merge zero-length runs: a zero after the first run joins its two neighbours
    b, j = [a[0]], 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return b


def segmentation_to_counts(seg, h: int, w: int) -> List[int]:
    """A COCO annotation's `segmentation` -> uncompressed run lengths at (h,w): a list of polygons (rasterised, several OR-ed), an
    uncompressed RLE dict (counts a list) or a compressed one (counts a string)."""
    if isinstance(seg, dict):
        size = [int(v) for v in seg.get("size", (h, w))]
        if size != [h, w]:
            raise ValueError("RLE of size {} in an image of {}x{}".format(size, h, w))
        counts = seg["counts"]
        if isinstance(counts, bytes):
            counts = counts.decode("ascii")
        counts = wire.rle_from_string(counts) if isinstance(counts, str) else [int(c) for c in counts]
        if not counts or min(counts) < 0 or sum(counts) != h * w:
            raise ValueError("RLE runs add up to {}, not to {}x{}".format(sum(counts), h, w))
        return counts
    if isinstance(seg, (list, tuple)):
        polys = [p for p in seg if len(p) >= 6]
        if len(polys) == 1:
            return poly_to_counts(polys[0], h, w)
        m = np.zeros((h, w), dtype=np.uint8)
        for p in polys:
            m |= counts_to_mask(poly_to_counts(p, h, w), h, w)
        return wire.rle_counts(m) if m.size else []
    raise ValueError("segmentation of type {}".format(type(seg).__name__))


# ---- IoU ----------------------------------------------------------------------------------------------------------------------------

_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def intersections_host(det_masks: np.ndarray, gt_counts: Sequence[Sequence[int]], h: int, w: int):
    """The host path of ops.mask_intersections, on the same bits: (n,h,w) bitmasks and m run-length lists ->
    (inter (n,m), det_areas (n,), gt_areas (m,)) int32."""
    det = np.asarray(det_masks).astype(bool).reshape(len(det_masks), -1)
    if det.shape[1] != h * w:
        raise ValueError("detections of {} pixels against ground truth of {}x{}".format(det.shape[1], h, w))
    dp = np.packbits(det, axis=1)
    gp = [np.packbits(counts_to_mask(c, h, w).reshape(-1)) for c in gt_counts]
    inter = np.zeros((det.shape[0], len(gp)), dtype=np.int32)
    for j, g in enumerate(gp):
        inter[:, j] = _POP8[dp & g[None, :]].sum(axis=1, dtype=np.int64)
    det_areas = _POP8[dp].sum(axis=1, dtype=np.int64).astype(np.int32)
    gt_areas = np.array([int(_POP8[g].sum(dtype=np.int64)) for g in gp], dtype=np.int32)
    return inter, det_areas, gt_areas


def boundary_dilation(h: int, w: int, ratio: float = 0.02) -> int:
    """The erosion distance of Boundary IoU for an (h,w) image: ratio times the diagonal, rounded with Python's round, at least 1."""
    return max(1, int(round(float(ratio) * float(np.sqrt(int(h) * int(h) + int(w) * int(w))))))


def _all_set_in_window(a: np.ndarray, d: int, axis: int) -> np.ndarray:
    """out[i] = every element of a[i-d .. i+d] along `axis` is set and inside the array."""
    n, k = a.shape[axis], 2 * d + 1
    out = np.zeros(a.shape, dtype=bool)
    if k > n:
        return out
    a = np.moveaxis(a, axis, -1)
    c = np.concatenate([np.zeros(a.shape[:-1] + (1,), dtype=np.int32), np.cumsum(a, axis=-1, dtype=np.int32)], axis=-1)
    np.moveaxis(out, axis, -1)[..., d:n - d] = (c[..., k:] - c[..., :-k]) == k
    return out


def boundary_host(masks_np: np.ndarray, d: int) -> np.ndarray:
    """(R,h,w) 0/1 -> (R,h,w) bool, the boundary of Boundary IoU (Cheng et al., CVPR 2021): mask AND NOT eroded, where eroded is the
    mask zero-padded by one pixel and eroded d times with a 3x3 all-ones element, which is: every pixel of the (2d+1)x(2d+1) square
    around the pixel lies inside the image and is set.  The square is separable: a window of 2d+1 along x, then along y, each by one
    running sum.  The host path of ops.mask_boundary_bits, on the same bits."""
    m = np.asarray(masks_np).astype(bool)
    if m.ndim != 3:
        raise ValueError("boundary_host: expected (R,h,w) masks, got {}".format(m.shape))
    d = int(d)
    if d < 1:
        raise ValueError("boundary_host: erosion distance {} must be at least 1".format(d))
    if m.shape[0] == 0:
        return m
    return m & ~_all_set_in_window(_all_set_in_window(m, d, 2), d, 1)


def _pair_counts(dp: np.ndarray, gp: List[np.ndarray]):
    inter = np.zeros((dp.shape[0], len(gp)), dtype=np.int32)
    for j, g in enumerate(gp):
        inter[:, j] = _POP8[dp & g[None, :]].sum(axis=1, dtype=np.int64)
    det_areas = _POP8[dp].sum(axis=1, dtype=np.int64).astype(np.int32)
    gt_areas = np.array([int(_POP8[g].sum(dtype=np.int64)) for g in gp], dtype=np.int32)
    return inter, det_areas, gt_areas


def boundary_intersections_host(det_masks: np.ndarray, gt_counts: Sequence[Sequence[int]], h: int, w: int, d: int):
    """The host path of ops.mask_boundary_intersections, on the same bits: the three arrays of intersections_host for the masks, then
    the same three for their boundaries at erosion distance d."""
    det = np.asarray(det_masks).astype(bool).reshape(len(det_masks), -1)
    if det.shape[1] != h * w:
        raise ValueError("detections of {} pixels against ground truth of {}x{}".format(det.shape[1], h, w))
    det = det.reshape(-1, h, w)
    gts = [counts_to_mask(c, h, w).astype(bool) for c in gt_counts]
    out = _pair_counts(np.packbits(det.reshape(len(det), -1), axis=1), [np.packbits(g.reshape(-1)) for g in gts])
    bd = boundary_host(det, d)
    bg = boundary_host(np.stack(gts), d) if gts else np.zeros((0, h, w), dtype=bool)
    return out + _pair_counts(np.packbits(bd.reshape(len(bd), -1), axis=1), [np.packbits(g.reshape(-1)) for g in bg])


def mask_iou_from_counts(inter, det_areas, gt_areas, iscrowd) -> np.ndarray:
    """float64 IoU from integer counts: inter / (a_dt + a_gt - inter), for a crowd ground truth inter / a_dt; 0 where that is 0 / 0."""
    inter = np.asarray(inter, dtype=np.float64)
    a_dt = np.asarray(det_areas, dtype=np.float64)[:, None]
    a_gt = np.asarray(gt_areas, dtype=np.float64)[None, :]
    crowd = np.asarray(iscrowd, dtype=bool)[None, :]
    den = np.where(crowd, a_dt + 0.0 * a_gt, a_dt + a_gt - inter)
    return np.where(den > 0, inter / np.where(den > 0, den, 1.0), 0.0)


def box_iou_xywh(dt, gt, iscrowd) -> np.ndarray:
    """The same two rules on XYWH boxes, no +1 (maskApi.c bbIou)."""
    dt, gt = np.asarray(dt, dtype=np.float64).reshape(-1, 4), np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    a_dt, a_gt = (dt[:, 2] * dt[:, 3])[:, None], (gt[:, 2] * gt[:, 3])[None, :]
    iw = np.minimum(dt[:, None, 0] + dt[:, None, 2], gt[None, :, 0] + gt[None, :, 2]) - np.maximum(dt[:, None, 0], gt[None, :, 0])
    ih = np.minimum(dt[:, None, 1] + dt[:, None, 3], gt[None, :, 1] + gt[None, :, 3]) - np.maximum(dt[:, None, 1], gt[None, :, 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
    crowd = np.asarray(iscrowd, dtype=bool)[None, :]
    den = np.where(crowd, a_dt + 0.0 * a_gt, a_dt + a_gt - inter)
    return np.where(den > 0, inter / np.where(den > 0, den, 1.0), 0.0)


# ---- COCOeval: evaluateImg / accumulate / summarize -----------------------------------------------------------------------------------

def evaluate_img(ious: np.ndarray, dt_scores, dt_areas, gt_areas, gt_ignore, gt_crowd, area_rng, max_det: int) -> Optional[Dict]:
    """One (image, category, area range).  ious (D,G) with the detections ALREADY sorted by descending score (stable) and cut to the
    largest maxDet, ground truths in annotation order."""
    d_n, g_n = len(dt_scores), len(gt_areas)
    if d_n == 0 and g_n == 0:
        return None
    gt_areas = np.asarray(gt_areas, dtype=np.float64)
    g_ig = np.asarray(gt_ignore, dtype=bool) | (gt_areas < area_rng[0]) | (gt_areas > area_rng[1])
    order = np.argsort(g_ig, kind="mergesort")                         # non-ignored first, stable
    g_ig = g_ig[order]
    crowd = np.asarray(gt_crowd, dtype=bool)[order]
    d_n = min(d_n, max_det)
    ious = np.asarray(ious, dtype=np.float64).reshape(len(dt_scores), g_n)[:d_n][:, order]
    t_n = len(IOU_THRS)
    gtm = np.zeros((t_n, g_n), dtype=bool)
    dtm = np.zeros((t_n, d_n), dtype=bool)
    dt_ig = np.zeros((t_n, d_n), dtype=bool)
    if g_n and d_n:
        for ti, t in enumerate(IOU_THRS):
            for di in range(d_n):
                iou, m = min(float(t), 1 - 1e-10), -1
                row = ious[di]
                for gi in range(g_n):
                    if gtm[ti, gi] and not crowd[gi]:
                        continue
                    if m > -1 and not g_ig[m] and g_ig[gi]:
                        break
                    if row[gi] < iou:
                        continue
                    iou, m = row[gi], gi
                if m == -1:
                    continue
                dt_ig[ti, di] = g_ig[m]
                dtm[ti, di] = True
                gtm[ti, m] = True
    a = np.asarray(dt_areas, dtype=np.float64)[:d_n]
    outside = (a < area_rng[0]) | (a > area_rng[1])
    dt_ig |= (~dtm) & outside[None, :]
    return {"dt_scores": np.asarray(dt_scores, dtype=np.float64)[:d_n], "dtm": dtm, "dt_ig": dt_ig, "gt_ig": g_ig}


def accumulate(eval_imgs, n_cats: int) -> Dict[str, np.ndarray]:
    """eval_imgs[k][a] = list over images of evaluate_img results (None dropped by the caller or here) ->
    precision (T,R,K,A,M) and recall (T,K,A,M), -1 where there is no non-ignored ground truth."""
    t_n, r_n, a_n, m_n = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((t_n, r_n, n_cats, a_n, m_n))
    recall = -np.ones((t_n, n_cats, a_n, m_n))
    eps = np.spacing(1.0)
    for k in range(n_cats):
        for ai in range(a_n):
            es = [e for e in eval_imgs[k][ai] if e is not None]
            if not es:
                continue
            gt_ig = np.concatenate([e["gt_ig"] for e in es])
            npig = int(np.count_nonzero(~gt_ig))
            if npig == 0:
                continue
            for mi, max_det in enumerate(MAX_DETS):
                scores = np.concatenate([e["dt_scores"][:max_det] for e in es])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["dtm"][:, :max_det] for e in es], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ig"][:, :max_det] for e in es], axis=1)[:, inds]
                tp_sum = np.cumsum(dtm & ~dt_ig, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~dtm & ~dt_ig, axis=1).astype(np.float64)
                for ti in range(t_n):
                    tp, fp = tp_sum[ti], fp_sum[ti]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + eps)
                    recall[ti, k, ai, mi] = rc[-1] if nd else 0.0
                    if nd:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]        # right-to-left running maximum
                    pos = np.searchsorted(rc, REC_THRS, side="left")
                    q = np.zeros(r_n)
                    ok = pos < nd
                    q[ok] = pr[pos[ok]]
                    precision[ti, :, k, ai, mi] = q
    return {"precision": precision, "recall": recall}


def _mean_valid(x: np.ndarray) -> float:
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def summarize(acc: Dict[str, np.ndarray]) -> np.ndarray:
    """The twelve numbers of COCOeval.summarize for detection, in STAT_NAMES order; -1 where no cell has ground truth."""
    p, r = acc["precision"], acc["recall"]
    t50, t75 = int(np.flatnonzero(np.isclose(IOU_THRS, 0.5))[0]), int(np.flatnonzero(np.isclose(IOU_THRS, 0.75))[0])
    last = len(MAX_DETS) - 1
    return np.array([
        _mean_valid(p[:, :, :, 0, last]), _mean_valid(p[t50, :, :, 0, last]), _mean_valid(p[t75, :, :, 0, last]),
        _mean_valid(p[:, :, :, 1, last]), _mean_valid(p[:, :, :, 2, last]), _mean_valid(p[:, :, :, 3, last]),
        _mean_valid(r[:, :, 0, 0]), _mean_valid(r[:, :, 0, 1]), _mean_valid(r[:, :, 0, 2]),
        _mean_valid(r[:, :, 1, last]), _mean_valid(r[:, :, 2, last]), _mean_valid(r[:, :, 3, last])])


# ---- the dataset side -----------------------------------------------------------------------------------------------------------------

class GroundTruth:
    """A COCO annotation dict indexed for scoring: images, category ids (ascending), per image its annotations in file order, and per
    annotation the run lengths of its segmentation (rasterised on first use, once)."""

    def __init__(self, dataset: Dict):
        self.images = {im["id"]: im for im in dataset.get("images", [])}
        self.cat_ids = sorted(c["id"] for c in dataset.get("categories", []))
        self.cat_names = {c["id"]: c.get("name", str(c["id"])) for c in dataset.get("categories", [])}
        self.has_annotations = "annotations" in dataset
        self.anns: Dict = {i: [] for i in self.images}
        for a in dataset.get("annotations", []):
            self.anns.setdefault(a["image_id"], []).append(a)
        self._counts: Dict = {}

    def size(self, img_id):
        im = self.images[img_id]
        return int(im["height"]), int(im["width"])

    def counts(self, img_id) -> List[List[int]]:
        """Run lengths of every annotation of the image, in annotation order."""
        if img_id not in self._counts:
            h, w = self.size(img_id)
            out = []
            for a in self.anns.get(img_id, []):
                if "segmentation" not in a:
                    raise ValueError("annotation {} of image {} has no segmentation: segm cannot be scored".format(a.get("id"), img_id))
                out.append(segmentation_to_counts(a["segmentation"], h, w))
            self._counts[img_id] = out
        return self._counts[img_id]


def score(gt: GroundTruth, results: List[Dict], iou_type: str, tables: Optional[Dict] = None, img_ids=None,
          btables: Optional[Dict] = None) -> Dict:
    """COCOeval for one iouType.  results: COCO result dicts with dataset category ids; for "segm" each carries `_k`, its row in its
    image's table, and tables[img_id] = (inter (n, m), det_areas (n,), gt_areas (m,)) with the columns in gt.anns[img_id] order.
    "boundary" (Boundary AP) is "segm" with another IoU: btables[img_id] holds the same three arrays for the boundaries of the masks,
    and the IoU is the smaller of the mask IoU and the boundary IoU, a crowd ground truth taking the crowd rule in both; areas and
    everything else stay those of "segm".
    -> {"stats": the twelve numbers, "precision": ..., "recall": ...}."""
    if iou_type not in ("bbox", "segm", "boundary"):
        raise ValueError("iouType {!r} is not built: only bbox, segm and boundary".format(iou_type))
    imgs = sorted(gt.images) if img_ids is None else sorted(set(img_ids))
    cat_index = {c: k for k, c in enumerate(gt.cat_ids)}
    by_img_cat: Dict = {}
    for r in results:
        if r["category_id"] in cat_index:
            by_img_cat.setdefault((r["image_id"], r["category_id"]), []).append(r)
    eval_imgs = [[[] for _ in AREA_RNG] for _ in gt.cat_ids]
    for img in imgs:
        anns = gt.anns.get(img, [])
        for c in gt.cat_ids:
            g_idx = [j for j, a in enumerate(anns) if a["category_id"] == c]
            dts = by_img_cat.get((img, c), [])
            if not g_idx and not dts:
                continue
            order = np.argsort([-d["score"] for d in dts], kind="mergesort")[:MAX_DETS[-1]]
            dts = [dts[i] for i in order]
            g = [anns[j] for j in g_idx]
            crowd = [bool(a.get("iscrowd", 0)) for a in g]
            ignore = [bool(a.get("ignore", 0)) or cr for a, cr in zip(g, crowd)]
            g_area = [float(a["area"]) for a in g]
            if iou_type == "bbox":
                d_area = [float(d["bbox"][2]) * float(d["bbox"][3]) for d in dts]
                ious = box_iou_xywh([d["bbox"] for d in dts], [a["bbox"] for a in g], crowd)
            else:
                rows = [d["_k"] for d in dts]
                if dts:
                    inter, a_dt, a_gt = tables[img]
                    inter = np.asarray(inter).reshape(len(a_dt), len(a_gt))
                    d_area = [float(a_dt[k]) for k in rows]
                    ious = mask_iou_from_counts(inter[np.ix_(rows, g_idx)] if g_idx else np.zeros((len(rows), 0)),
                                                [a_dt[k] for k in rows], [a_gt[j] for j in g_idx], crowd)
                    if iou_type == "boundary":
                        b_inter, b_dt, b_gt = btables[img]
                        b_inter = np.asarray(b_inter).reshape(len(b_dt), len(b_gt))
                        ious = np.minimum(ious, mask_iou_from_counts(b_inter[np.ix_(rows, g_idx)] if g_idx else np.zeros((len(rows), 0)),
                                                                     [b_dt[k] for k in rows], [b_gt[j] for j in g_idx], crowd))
                else:
                    d_area, ious = [], np.zeros((0, len(g)))
            scores = [float(d["score"]) for d in dts]
            k = cat_index[c]
            for ai, rng in enumerate(AREA_RNG):
                eval_imgs[k][ai].append(evaluate_img(ious, scores, d_area, g_area, ignore, crowd, rng, MAX_DETS[-1]))
    acc = accumulate(eval_imgs, len(gt.cat_ids))
    acc["stats"] = summarize(acc)
    return acc
