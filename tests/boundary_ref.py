"""The boundary of Boundary IoU (Cheng et al., CVPR 2021) as its definition reads, in NumPy, and the mask patterns shared by
tests/test_cpu_boundary.py and tests/test_gpu_boundary.py (no test in here).

boundary(m, d): pad m with one pixel of zeros on every side, erode d times with a 3x3 all-ones element (a pixel survives a step iff it
and its eight neighbours are set; what lies outside the padded array is background), strip the pad, and keep m AND NOT eroded.  Nothing
here is shared with coco_eval.boundary_host or the kernel: the iteration is literal, one 3x3 step at a time."""
import numpy as np


def erode3x3(a):
    """One step on a 2-D bool array, outside = background."""
    p = np.zeros((a.shape[0] + 2, a.shape[1] + 2), dtype=bool)
    p[1:-1, 1:-1] = a
    out = np.ones_like(a)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out &= p[dy:dy + a.shape[0], dx:dx + a.shape[1]]
    return out


def boundary_one(m, d):
    m = np.asarray(m).astype(bool)
    h, w = m.shape
    e = np.zeros((h + 2, w + 2), dtype=bool)
    e[1:-1, 1:-1] = m
    for _ in range(int(d)):
        if not e.any():
            break                                                       # nothing is left to erode: the remaining steps change nothing
        e = erode3x3(e)
    return m & ~e[1:-1, 1:-1]


def boundary_ref(masks, d):
    """(R,h,w) 0/1 -> (R,h,w) bool."""
    masks = np.asarray(masks)
    if masks.shape[0] == 0:
        return np.zeros(masks.shape, dtype=bool)
    return np.stack([boundary_one(m, d) for m in masks])


def packed(masks_np):
    """(R,H,W) 0/1 -> (R, ceil(HW/64)) uint64, bit p % 64 of word p / 64 = row-major pixel p, the unused high bits zero."""
    r = masks_np.shape[0]
    flat = np.asarray(masks_np).reshape(r, -1).astype(np.uint8)
    nw = (flat.shape[1] + 63) // 64
    pad = np.zeros((r, nw * 64), dtype=np.uint8)
    pad[:, :flat.shape[1]] = flat
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view(np.uint64)


def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), dtype=np.uint8)
    m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = 1
    return m


def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)


def mask_set(h, w, seed):
    """The patterns of tests/test_gpu_coco_eval.py::mask_set, and solid shapes: the thin and random patterns erode to nothing at d >= 1,
    rectangles and discs do not.  One rectangle touches the top and left edges, one the bottom and right, one spans every row."""
    z = np.zeros((h, w), dtype=np.uint8)
    out = [z.copy(), 1 - z]                                             # empty, full
    m = z.copy(); m[0, 0] = 1; out.append(m)                            # the first pixel
    m = z.copy(); m[h - 1, w - 1] = 1; out.append(m)                    # the last pixel
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(((yy + xx) & 1).astype(np.uint8))                        # checkerboard
    m = z.copy(); m[h // 2, :] = 1; out.append(m)                       # one row
    m = z.copy(); m[:, w // 2] = 1; out.append(m)                       # one column
    rng = np.random.RandomState(seed)
    for p in (0.02, 0.5, 0.98):
        out.append((rng.rand(h, w) < p).astype(np.uint8))
    out.append(rect(h, w, 0, (2 * h + 2) // 3, 0, (3 * w + 3) // 4))     # touches the top and left edges
    out.append(rect(h, w, h // 5, h, w // 3, w))                        # touches the bottom and right edges
    out.append(rect(h, w, h // 4, h - h // 4, w // 6, w - w // 6))       # interior
    out.append(rect(h, w, 0, h, w // 2 - min(w // 2, 3), w // 2 + 4))    # a band over every row
    out.append(disc(h, w, h / 2.0, w / 2.0, 0.45 * min(h, w)))
    out.append(disc(h, w, 0.2 * h, 0.85 * w, 0.4 * max(h, w)))           # a disc cut by two edges
    out.append(np.maximum(disc(h, w, 0.3 * h, 0.3 * w, 0.25 * min(h, w)), rect(h, w, h // 2, h - 1, 1, w - 1)) & (rng.rand(h, w) < 0.995))
    return np.stack(out).astype(np.uint8)
