"""numpy restatement of sliced inference (DESIGN §3 "Sliced inference"; include/cmk.h cmk_slice_boxes_to_image, cmk_nms_topk_metric): the
tile grid in plain integer loops, the map back into the image frame in float32 with one rounded operation per step and in the order the
kernel of csrc/slice/slice.hip must follow bit for bit, and a plain greedy class-wise NMS in float64 on IoU or on the intersection over
the smaller box.  Nothing here calls the code under test."""
import numpy as np

from centermask2_amd import ops
from .tta_ref import iou

F = np.float32


def axis_starts(size, t, overlap):
    """The tile starts along one axis of `size` pixels for tiles of t <= size: 0, stride, 2 * stride, .. while the tile ends before the
    border, then size - t (the tile shifted back onto the border)."""
    stride = max(1, int(t * (1 - overlap)))
    out = []
    s = 0
    while s + t < size:
        out.append(s)
        s += stride
    out.append(size - t)
    return sorted(set(out))


def grid(h, w, tile_h, tile_w, overlap):
    """[(y0, x0, th, tw)] in row-major order; every tile th x tw = min(tile_h, h) x min(tile_w, w)."""
    th, tw = min(tile_h, h), min(tile_w, w)
    return [(y0, x0, th, tw) for y0 in axis_starts(h, th, overlap) for x0 in axis_starts(w, tw, overlap)]


def passes(h, w, tile_h, tile_w, overlap, min_size, max_size, full_image):
    """[(y0, x0, th, tw, new_h, new_w)]: the tiles, each resized by ResizeShortestEdge(min_size, max_size), then the whole image."""
    out = [t + ops.resize_shortest_edge_shape(t[2], t[3], min_size, max_size) for t in grid(h, w, tile_h, tile_w, overlap)]
    if full_image:
        out.append((0, 0, h, w) + ops.resize_shortest_edge_shape(h, w, min_size, max_size))
    return out


def table(pss):
    """(A,6) float32 rows (x0, y0, rx, ry, tw, th): the ratios computed in double and rounded once."""
    return np.asarray([(x0, y0, F(tw / nw), F(th / nh), tw, th) for y0, x0, th, tw, nh, nw in pss], dtype=F)


def boxes_to_image(box, score, cls, loc, counts, pss):
    """box (A,K,4), score (A,K), cls (A,K), loc (A,K,2), counts (A) -> the candidate set: dict of box (M,4), score (M), cls (M) int32,
    loc (M,2), src (M) int32 with M = sum(min(max(counts, 0), K)), in pass order and the given order within a pass.  x * rx, then + x0,
    then clipped to [x0, x0 + tw]; y likewise; loc without the clip."""
    box, score, loc = np.asarray(box, dtype=F), np.asarray(score, dtype=F), np.asarray(loc, dtype=F)
    k = box.shape[1]
    ob, os_, oc, ol, osrc = [], [], [], [], []
    for a, row in enumerate(table(pss)):
        n = min(max(int(counts[a]), 0), k)
        x0, y0, rx, ry, tw, th = (F(v) for v in row)
        xhi, yhi = x0 + tw, y0 + th
        b, l = box[a, :n], loc[a, :n]
        clip = lambda v, lo, hi: np.fmin(np.fmax(v, lo), hi)           # fminf / fmaxf: a NaN coordinate clips to a bound
        mx = lambda v: (v * rx).astype(F) + x0
        my = lambda v: (v * ry).astype(F) + y0
        ob.append(np.stack([clip(mx(b[:, 0]), x0, xhi), clip(my(b[:, 1]), y0, yhi), clip(mx(b[:, 2]), x0, xhi), clip(my(b[:, 3]), y0, yhi)],
                           axis=1).astype(F))
        ol.append(np.stack([mx(l[:, 0]), my(l[:, 1])], axis=1).astype(F))
        os_.append(score[a, :n])
        oc.append(np.asarray(cls)[a, :n].astype(np.int32))
        osrc.append((a * k + np.arange(n)).astype(np.int32))
    out = dict(box=np.concatenate(ob), score=np.concatenate(os_), cls=np.concatenate(oc), loc=np.concatenate(ol), src=np.concatenate(osrc))
    assert out["box"].dtype == F and out["loc"].dtype == F
    return out


def ios(a, b):
    """Intersection over the smaller box, float64; NaN when the smaller area is zero (it then suppresses nothing)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    small = min((a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1]))
    return iw * ih / small if small != 0 else float("nan")


METRICS = {"iou": iou, "ios": ios}


def nms(box, score, cls, thr, topk, metric):
    """Greedy class-wise NMS in float64: candidates in stable descending-score order, one suppressed when its metric with a kept box of
    its class exceeds thr (a NaN does not); the indices of the first topk survivors."""
    f = METRICS[metric]
    order = np.argsort(-np.asarray(score, dtype=np.float64), kind="stable")
    keep = []
    for i in order:
        if all(cls[i] != cls[j] or not f(box[i], box[j]) > thr for j in keep):
            keep.append(int(i))
            if len(keep) == topk:
                break
    return keep


def nms_margin(box, score, cls, thr, topk, metric):
    """nms, and how far its decisions are from the threshold: per candidate reached, the largest metric with a kept box of its class
    (NaN aside) decides -- above thr it is suppressed, otherwise kept -- and its distance to thr is the decision's margin.  Returns (the
    kept indices, the smallest margin).  An NMS whose metric values differ from these by less than that margin takes the same
    decisions in the same order, by induction over the candidates: pairs that decide nothing may sit anywhere."""
    f = METRICS[metric]
    order = np.argsort(-np.asarray(score, dtype=np.float64), kind="stable")
    keep, margin = [], float("inf")
    for i in order:
        vals = [f(box[i], box[j]) for j in keep if cls[i] == cls[j]]
        best = max([v for v in vals if not np.isnan(v)], default=-float("inf"))
        margin = min(margin, abs(best - thr))
        if not best > thr:
            keep.append(int(i))
            if len(keep) == topk:
                break
    return keep, margin


def pair_metric(box, cls, metric):
    """The metric (float64) of every same-class pair i < j of boxes (n,4); other pairs, and NaN pairs, are -1."""
    b = np.asarray(box, dtype=np.float64)
    iw = np.clip(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), 0, None)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    den = np.minimum(area[:, None], area[None, :]) if metric == "ios" else area[:, None] + area[None, :] - iw * ih
    ok = den > 0
    m = np.where(ok, iw * ih / np.where(ok, den, 1), -1.0)
    same = (np.asarray(cls)[:, None] == np.asarray(cls)[None, :]) & np.triu(np.ones((len(b), len(b)), dtype=bool), 1)
    return np.where(same, m, -1.0)
