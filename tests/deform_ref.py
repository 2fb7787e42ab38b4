"""The tests' own float64 restatement of the deformable 3x3 conv (d2 DeformConv / ModulatedDeformConv, stride 1, pad 1), written
with grid_sample (align_corners=True, zero padding): a sample outside the map and every out-of-map bilinear corner count as 0, as in
d2.  Independent of the HIP kernel and of the per-corner stand-in tests/golden/make_golden_dcn.py feeds the reference."""
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
