"""The tests' own float64 restatement of the keypoint heatmap decode: the depth-to-space of the packed score_lowres output, the head's
bilinear x2 (keypoint_head.py:223, upsample_bilinear2d with align_corners=False) and detectron2's heatmaps_to_keypoints as
keypoint_rcnn_inference uses it (keypoint_head.py:89-116: bicubic resize to the box, first maximum, score normalised over the 4S x 4S
map, columns x, y, score).  Both resamplings are written out as explicit interpolation matrices — no F.interpolate — so this is
independent of the HIP kernel.  Box sizes are taken in fp32 as d2 takes them (a ceil of the fp32 width decides the map size)."""
import functools
import math

import torch

A = -0.75          # PyTorch's bicubic convolution parameter


def depth_to_space(packed: torch.Tensor, num_keypoints: int) -> torch.Tensor:
    """(R, S, S, 4K) with channel (2py+px)*K + k -> (R, K, 2S, 2S): out[2a+py, 2b+px] = packed[a, b, (2py+px)*K + k]."""
    r, s = packed.shape[0], packed.shape[1]
    return packed.reshape(r, s, s, 2, 2, num_keypoints).permute(0, 5, 1, 3, 2, 4).reshape(r, num_keypoints, 2 * s, 2 * s)


@functools.lru_cache(maxsize=None)
def bilinear_matrix(n_in: int) -> torch.Tensor:
    """(2 n_in, n_in): upsample_bilinear2d x2 along one axis, align_corners=False — source 0.5 (d + 0.5) - 0.5 clamped at 0, lower tap
    its floor, upper tap min(lower + 1, n_in - 1)."""
    m = torch.zeros((2 * n_in, n_in), dtype=torch.float64)
    for d in range(2 * n_in):
        src = max(0.5 * (d + 0.5) - 0.5, 0.0)
        lo = int(math.floor(src))
        hi = min(lo + 1, n_in - 1)
        m[d, lo] += 1.0 - (src - lo)
        m[d, hi] += src - lo
    return m


def _cubic(t: float):
    near = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1           # |x| <= 1
    far = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A       # 1 < |x| < 2
    return (far(t + 1), near(t), near(1 - t), far(2 - t))


@functools.lru_cache(maxsize=None)
def bicubic_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """(n_out, n_in): upsample_bicubic2d along one axis to n_out, align_corners=False — scale n_in / n_out, source scale (d + 0.5) - 0.5
    NOT clamped, taps floor(src) - 1 .. floor(src) + 2 clamped to [0, n_in - 1]."""
    m = torch.zeros((n_out, n_in), dtype=torch.float64)
    scale = n_in / n_out
    for d in range(n_out):
        src = scale * (d + 0.5) - 0.5
        f = math.floor(src)
        for j, w in enumerate(_cubic(src - f)):
            m[d, min(max(f - 1 + j, 0), n_in - 1)] += w
    return m


def heatmaps(logits28: torch.Tensor) -> torch.Tensor:
    """(..., 2S, 2S) -> (..., 4S, 4S) float64: the head's bilinear x2."""
    b = bilinear_matrix(logits28.shape[-1])
    return b @ logits28.double() @ b.t()


def box_geometry(box):
    """(x0, y0, w, h, Wc, Hc): w = max(x1 - x0, 1) in fp32 as d2 computes it, Wc = ceil(w)."""
    b = box.detach().float().cpu()
    w = float((b[2] - b[0]).clamp(min=1))
    h = float((b[3] - b[1]).clamp(min=1))
    return float(b[0]), float(b[1]), w, h, math.ceil(w), math.ceil(h)


def roi_map(map56_k: torch.Tensor, box) -> torch.Tensor:
    """One keypoint's (4S, 4S) float64 map resized to the box: (Hc, Wc)."""
    _, _, _, _, wc, hc = box_geometry(box)
    n = map56_k.shape[-1]
    return bicubic_matrix(n, hc) @ map56_k @ bicubic_matrix(n, wc).t()


def first_max(m: torch.Tensor):
    """(value, row, col, gap): the first maximum in row-major order and how far it lies above every other pixel."""
    flat = m.reshape(-1)
    pos = int(flat.argmax())
    top = float(flat[pos])
    rest = torch.cat([flat[:pos], flat[pos + 1:]])
    gap = top - float(rest.max()) if rest.numel() else math.inf
    return top, pos // m.shape[1], pos % m.shape[1], gap


def decode_one(logits28_r: torch.Tensor, box):
    """(K, 2S, 2S) logits of one RoI and its (4,) box -> list over keypoints of dict(xys = (x, y, score) float64, map, value, row, col,
    gap)."""
    x0, y0, w, h, wc, hc = box_geometry(box)
    m56 = heatmaps(logits28_r)
    out = []
    for k in range(m56.shape[0]):
        rm = roi_map(m56[k], box)
        top, yi, xi, gap = first_max(rm)
        score = 1.0 / float(torch.exp(m56[k] - top).sum())
        out.append(dict(xys=((xi + 0.5) * (w / wc) + x0, (yi + 0.5) * (h / hc) + y0, score), map=rm, value=top, row=yi, col=xi, gap=gap))
    return out


def pixel_of(x: float, y: float, box):
    """The (row, col) of the resized map that an (x, y) names: the inverse of x = (xi + 0.5) * (w / Wc) + x0."""
    x0, y0, w, h, wc, hc = box_geometry(box)
    return int(round((y - y0) / (h / hc) - 0.5)), int(round((x - x0) / (w / wc) - 0.5))
