"""The tests' own float64 restatements of the deformable 3x3 conv (d2 DeformConv / ModulatedDeformConv, stride 1, pad 1).
deform_conv3x3_ref is written with grid_sample (align_corners=True, zero padding): a sample outside the map and every out-of-map bilinear
corner count as 0, as in d2; it needs H, W >= 2.  deform_conv3x3_ref_corners follows the rule of include/cmk.h corner by corner, says what
is READ as well, and is valid for H or W = 1: it is the arbiter where an input holds an Inf or NaN.  Both are independent of the HIP kernel
and of the per-corner stand-in tests/golden/make_golden_dcn.py feeds the reference.  make_offsets: the offset tensors of the tests."""
import torch
import torch.nn.functional as F


def deform_conv3x3_ref(x, offsets, weight, dg, modulated, scale=None, shift=None, relu=False):
    """x (N,C,H,W), offsets (N,>=18*dg | 27*dg,H,W) raw (mask LOGITS in channels [18*dg, 27*dg) when modulated), weight (Cout,C,3,3)
    -> (N,Cout,H,W) float64.  H, W >= 2."""
    x, offsets, weight = x.double(), offsets.double(), weight.double()
    n, c, h, w = x.shape
    cpg = c // dg
    hs = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    ws = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    cols = torch.zeros((n, c, 9, h, w), dtype=torch.float64)
    for g in range(dg):
        for k in range(9):
            i, j = divmod(k, 3)
            py = hs - 1 + i + offsets[:, g * 18 + 2 * k]
            px = ws - 1 + j + offsets[:, g * 18 + 2 * k + 1]
            grid = torch.stack((2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1), dim=-1)
            s = F.grid_sample(x[:, g * cpg:(g + 1) * cpg], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            if modulated:
                s = s * torch.sigmoid(offsets[:, 18 * dg + g * 9 + k])[:, None]
            cols[:, g * cpg:(g + 1) * cpg, k] = s
    y = torch.einsum("nckhw,ock->nohw", cols, weight.reshape(weight.shape[0], c, 9))
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return y.clamp_min(0) if relu else y


def deform_conv3x3_ref_corners(x, offsets, weight, dg, modulated, scale=None, shift=None, relu=False):
    """The same operation by the rule of include/cmk.h, literally: a sample outside (-1,H) x (-1,W) is 0 and reads nothing, an out-of-map
    corner reads nothing, an in-map corner is read and multiplied by its weight even where that weight is 0 (so 0 * Inf = NaN there and
    only there).  Arguments and result as deform_conv3x3_ref; any H, W >= 1.  The ReLU keeps a NaN."""
    x, offsets, weight = x.double(), offsets.double(), weight.double()
    n, c, h, w = x.shape
    cpg = c // dg
    hs = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    ws = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    flat = x.reshape(n, c, h * w)
    zero = torch.zeros((), dtype=torch.float64)
    cols = torch.zeros((n, c, 9, h, w), dtype=torch.float64)
    for g in range(dg):
        xg = flat[:, g * cpg:(g + 1) * cpg]
        for k in range(9):
            i, j = divmod(k, 3)
            py = hs - 1 + i + offsets[:, g * 18 + 2 * k]
            px = ws - 1 + j + offsets[:, g * 18 + 2 * k + 1]
            inside = (py > -1) & (px > -1) & (py < h) & (px < w)
            y0, x0 = torch.floor(py), torch.floor(px)
            ly, lx = py - y0, px - x0
            s = torch.zeros((n, cpg, h, w), dtype=torch.float64)
            for cy, cx, wt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx), (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
                read = inside & (cy >= 0) & (cy <= h - 1) & (cx >= 0) & (cx <= w - 1)
                idx = (cy.clamp(0, h - 1) * w + cx.clamp(0, w - 1)).long().reshape(n, 1, h * w).expand(n, cpg, h * w)
                v = torch.gather(xg, 2, idx).reshape(n, cpg, h, w)
                s = s + torch.where(read[:, None], v * wt[:, None], zero)          # where, not a product with 0: an unread value is dropped
            if modulated:
                s = s * torch.sigmoid(offsets[:, 18 * dg + g * 9 + k])[:, None]
            cols[:, g * cpg:(g + 1) * cpg, k] = s
    y = torch.einsum("nckhw,ock->nohw", cols, weight.reshape(weight.shape[0], c, 9))
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def make_offsets(kind, mask, n, h, w, dg, modulated, seed):
    """(N, 18*dg | 27*dg, H, W) offsets (+ mask logits).  kind frac | int | far | edge: the generators of tests/test_gpu_deform_conv.py
    (far: with pixel (0, H/2, W/2) given nine taps that all lie outside the map); zero: no offset at all.  mask randn: logits of order one
    and nothing else; saturated: +-60 on two thirds of the taps."""
    from tests.test_gpu_deform_conv import _offsets
    off = _offsets("frac" if kind == "zero" else kind, n, h, w, dg, modulated, seed)
    if kind == "zero":
        off[:, :18 * dg] = 0.0
    if kind == "far":
        off[0, :18 * dg, h // 2, w // 2] = max(h, w) + 5.5
    if modulated:
        g = torch.Generator().manual_seed(seed + 1000)
        m = torch.randn((n, 9 * dg, h, w), generator=g)
        if mask == "saturated":
            u = torch.rand(m.shape, generator=g)
            m[u < 1 / 3] = 60.0
            m[u > 2 / 3] = -60.0
        off[:, 18 * dg:] = m
    return off
