"""numpy restatement of the test-time augmentation geometry (DESIGN §3 "Test-time augmentation"; include/cmk.h cmk_tta_*): the
augmentation list, the two box maps and the mask average, in float32 with one rounded operation per step and in the order the kernels of
csrc/resize.hip must follow bit for bit; plus a plain greedy class-wise NMS in float64 for the merge."""
import numpy as np

from centermask2_amd import ops

F = np.float32


def augmentations(h, w, min_sizes, max_size, flip):
    """Step 1: [(new_h, new_w, flipped)], per scale the plain image and then its mirror; repeated shapes are kept."""
    out = []
    for s in min_sizes:
        nh, nw = ops.resize_shortest_edge_shape(h, w, s, max_size)
        out.append((nh, nw, False))
        if flip:
            out.append((nh, nw, True))
    return out


def ratios(aug, h, w, to_image):
    """(rx, ry) of one augmentation: computed in double, rounded once to float32."""
    nh, nw, _ = aug
    return (F(w / nw), F(h / nh)) if to_image else (F(nw / w), F(nh / h))


def _flip_x(nw, x0, x1):
    return F(nw) - x1, F(nw) - x0


def boxes_to_image(box, score, cls, loc, counts, augs, h, w):
    """Step 3.  box (A,K,4), score (A,K), cls (A,K), loc (A,K,2), counts (A) -> the candidate set: dict of box (M,4), score (M),
    cls (M) int32, loc (M,2) with M = sum(min(counts, K)), in augmentation order and the given order within an augmentation."""
    box, score, loc = np.asarray(box, dtype=F), np.asarray(score, dtype=F), np.asarray(loc, dtype=F)
    k = box.shape[1]
    ob, os_, oc, ol = [], [], [], []
    for a, aug in enumerate(augs):
        n = min(max(int(counts[a]), 0), k)
        rx, ry = ratios(aug, h, w, True)
        b, l = box[a, :n], loc[a, :n]
        x0, y0, x1, y1, lx, ly = b[:, 0], b[:, 1], b[:, 2], b[:, 3], l[:, 0], l[:, 1]
        if aug[2]:
            x0, x1 = _flip_x(aug[1], x0, x1)
            lx = F(aug[1]) - lx
        clip = lambda v, hi: np.fmin(np.fmax(v, F(0)), F(hi))          # fminf / fmaxf: a NaN coordinate clips to a bound
        ob.append(np.stack([clip(x0 * rx, w), clip(y0 * ry, h), clip(x1 * rx, w), clip(y1 * ry, h)], axis=1).astype(F))
        ol.append(np.stack([lx * rx, ly * ry], axis=1).astype(F))
        os_.append(score[a, :n])
        oc.append(np.asarray(cls)[a, :n].astype(np.int32))
    return dict(box=np.concatenate(ob), score=np.concatenate(os_), cls=np.concatenate(oc), loc=np.concatenate(ol))


def boxes_to_aug(box, count, augs, h, w):
    """Step 5.  box (K,4) in the image frame -> (A,K,4) in every augmentation's frame (scale, then flip), zero rows from `count` on."""
    box = np.asarray(box, dtype=F)
    k = box.shape[0]
    n = min(max(int(count), 0), k)
    out = np.zeros((len(augs), k, 4), dtype=F)
    for a, aug in enumerate(augs):
        rx, ry = ratios(aug, h, w, False)
        x0, y0, x1, y1 = box[:n, 0] * rx, box[:n, 1] * ry, box[:n, 2] * rx, box[:n, 3] * ry
        if aug[2]:
            x0, x1 = _flip_x(aug[1], x0, x1)
        out[a, :n] = np.stack([x0, y0, x1, y1], axis=1)
    return out


def reduce_masks(masks, flips, scores, count):
    """Step 6.  masks (A,K,S,S), flips (A), scores (A,K) or None -> ((K,S,S), (K) or None): added in augmentation order starting from 0,
    flipped augmentations mirrored along x, one division by float32(A); zero rows from `count` on."""
    masks = np.asarray(masks, dtype=F)
    a_n, k = masks.shape[0], masks.shape[1]
    n = min(max(int(count), 0), k)
    acc = np.zeros(masks.shape[1:], dtype=F)
    sacc = np.zeros((k,), dtype=F)
    for a in range(a_n):
        acc = acc + (masks[a, :, :, ::-1] if flips[a] else masks[a])
        if scores is not None:
            sacc = sacc + np.asarray(scores, dtype=F)[a]
    acc, sacc = acc / F(a_n), sacc / F(a_n)
    acc[n:] = 0
    sacc[n:] = 0
    assert acc.dtype == F and sacc.dtype == F
    return acc, (sacc if scores is not None else None)


def iou(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / union if union > 0 else 0.0


def nms(box, score, cls, thr, topk):
    """Greedy class-wise NMS in float64: candidates in stable descending-score order, one suppressed when its IoU with a kept box of its
    class exceeds thr; the indices of the first topk survivors."""
    order = np.argsort(-np.asarray(score, dtype=np.float64), kind="stable")
    keep = []
    for i in order:
        if all(cls[i] != cls[j] or iou(box[i], box[j]) <= thr for j in keep):
            keep.append(int(i))
            if len(keep) == topk:
                break
    return keep
