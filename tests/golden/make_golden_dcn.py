"""Golden vectors for the deformable VoVNet stages (MODEL.VOVNET.STAGE_WITH_DCN), produced by the REFERENCE's own VoVNet/FPN.

    python tests/golden/make_golden_dcn.py        # needs /root/reference; writes tests/golden/vovnet_dcn.pt

The reference's vovnet.py binds detectron2.layers.DeformConv / ModulatedDeformConv at import time, so the stand-ins below are put
on the stub module BEFORE make_golden (which imports the reference package) is imported.  They are written from d2's public
behaviour in float64 as an explicit per-corner gather — independent of the HIP kernel and of the restatement in the tests:
sample (h-1+i+dy, w-1+j+dx) for tap k = 3i+j, offsets [g][k][dy, dx] per deformable group g, bilinear with each corner outside
the map counted as 0, and 0 when the point lies outside (-1,H) x (-1,W); the modulated form multiplies by mask[g][k].
d2's own source is not available, so this stays parity-unpinned against a real detectron2 (as the FPN stand-in already is).

Per case: (1) the reference's state-dict keys/shapes must equal synthetic.model_param_shapes(body, dcn...), (2) the reference runs on
seeded weights: stage3-5 on a small odd-sized input, p3-p7 on a /32 input (the smallest sizes whose stage-4 maps still cover the
3x3 pooling window), (3) the same network again with the offset conv zeroed and the mask logits at +40 (mask 1) must differ
by far more than 1e-3 (the deformation is not trivial; the GPU test repeats this on the package's own plain path rather than
storing a second set of outputs, which would push the file past the 1 MiB limit of a committed file).  The depth-wise body with the
DCN flags set must reproduce the plain depth-wise body bit for bit; its fixture is the key listing only, and the GPU test compares
it with vovnet_bodies.pt.  Data only — no reference source.
"""
import os
import sys

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import d2_stub  # noqa: E402

d2_stub.install()


def _deform_f64(x, offset, weight, dg, mask=None):
    """(N,C,H,W) x, (N,18*dg,H,W) offset, (Cout,C,3,3) weight, optional (N,9*dg,H,W) mask -> (N,Cout,H,W), computed in float64."""
    n, c, h, w = x.shape
    cpg = c // dg
    x64, off64 = x.double(), offset.double()
    cols = torch.zeros((n, c, 9, h, w), dtype=torch.float64)
    hs = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    ws = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    for g in range(dg):
        flat = x64[:, g * cpg:(g + 1) * cpg].reshape(n, cpg, h * w)
        for k in range(9):
            i, j = divmod(k, 3)
            py = hs - 1 + i + off64[:, g * 18 + 2 * k]
            px = ws - 1 + j + off64[:, g * 18 + 2 * k + 1]
            inside = (py > -1) & (px > -1) & (py < h) & (px < w)
            y0, x0 = torch.floor(py), torch.floor(px)
            ly, lx = py - y0, px - x0
            val = torch.zeros((n, cpg, h, w), dtype=torch.float64)
            for cy, cx, wt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx),
                               (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
                ok = inside & (cy >= 0) & (cy <= h - 1) & (cx >= 0) & (cx <= w - 1)
                idx = (cy.clamp(0, h - 1) * w + cx.clamp(0, w - 1)).long().reshape(n, 1, h * w).expand(n, cpg, h * w)
                val += torch.gather(flat, 2, idx).reshape(n, cpg, h, w) * (wt * ok)[:, None]
            if mask is not None:
                val = val * mask[:, g * 9 + k].double()[:, None]
            cols[:, g * cpg:(g + 1) * cpg, k] = val
    return torch.einsum("nckhw,ock->nohw", cols, weight.double().reshape(weight.shape[0], c, 9))


class DeformConv(nn.Module):
    """Stand-in for d2 DeformConv as the reference constructs it (3x3, stride 1, pad 1, dilation 1, groups 1, bias=False)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1,
                 bias=False, norm=None, activation=None):
        super().__init__()
        assert kernel_size == 3 and stride == 1 and padding == 1 and dilation == 1 and groups == 1 and not bias
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        nn.init.kaiming_uniform_(self.weight, nonlinearity="relu")

    def forward(self, x, offset):
        return _deform_f64(x, offset, self.weight, self.deformable_groups).to(x.dtype)


class ModulatedDeformConv(DeformConv):
    def forward(self, x, offset, mask):
        return _deform_f64(x, offset, self.weight, self.deformable_groups, mask).to(x.dtype)


sys.modules["detectron2.layers"].DeformConv = DeformConv
sys.modules["detectron2.layers"].ModulatedDeformConv = ModulatedDeformConv

import make_golden as G  # noqa: E402  (imports the reference package, which binds the two names above)

S = G.S
# name -> (body, STAGE_WITH_DCN, WITH_MODULATED_DCN, DEFORMABLE_GROUPS)
CASES = {
    "v39_v1_dg1": ("V-39-eSE", (False, True, True, True), False, 1),
    "v39_mod_dg2": ("V-39-eSE", (True, True, True, True), True, 2),
    "v19slim_mod_dg2": ("V-19-slim-eSE", (True, True, True, True), True, 2),
    "v19slimdw_flags": ("V-19-slim-dw-eSE", (True, True, True, True), True, 2),
}
ODD = (1, 58, 58)        # bottom-up only (stage3-5: 7x7, 3x3, 1x1)
P32 = (1, 64, 64)        # VoVNet + FPN + P6/P7


def build_reference(body, stage_with_dcn, modulated, dg):
    cfg = G.ref_get_cfg()
    cfg.merge_from_file(os.path.join("/root/reference/centermask2/configs/centermask/zy_model_config.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.VOVNET.CONV_BODY", body, "MODEL.VOVNET.STAGE_WITH_DCN", stage_with_dcn,
                         "MODEL.VOVNET.WITH_MODULATED_DCN", modulated, "MODEL.VOVNET.DEFORMABLE_GROUPS", dg])
    cfg.freeze()
    backbone = G.BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, G.ShapeSpec(channels=3))
    backbone.eval()
    return backbone


def run(backbone, x, x32):
    with torch.no_grad():
        bu = backbone.bottom_up(x)
        p = backbone(x32)
    out = {k: bu[k].clone() for k in ("stage3", "stage4", "stage5")}
    out.update({k: p[k].clone() for k in ("p3", "p4", "p5", "p6", "p7")})
    return out


def main():
    x = S.make_synthetic_images(*ODD, seed0=311)
    x32 = S.make_synthetic_images(*P32, seed0=312)
    out = dict(x=x, x32=x32)
    for name, (body, flags, modulated, dg) in CASES.items():
        backbone = build_reference(body, flags, modulated, dg)
        ref_sd = {"backbone." + k: v for k, v in backbone.state_dict().items()}
        dcn = dict(stage_with_dcn=flags, with_modulated_dcn=modulated, deformable_groups=dg)
        shapes = {k: v for k, v in S.model_param_shapes(body, **dcn).items() if k.startswith("backbone.")}
        assert set(ref_sd) == set(shapes), (name, sorted(set(ref_sd) ^ set(shapes))[:8])
        for k, v in ref_sd.items():
            assert tuple(v.shape) == tuple(shapes[k]), (name, k, tuple(v.shape), shapes[k])
        n_off = sum(1 for k in shapes if "/conv_offset." in k)
        print("{}: {} backbone keys match ({} offset-conv tensors)".format(name, len(shapes), n_off))
        sd = {k[len("backbone."):]: v for k, v in S.make_synthetic_state_dict(body, 0, **dcn).items() if k.startswith("backbone.")}
        backbone.load_state_dict(sd, strict=True)
        case = dict(body=body, stage_with_dcn=torch.tensor(flags), modulated=torch.tensor(modulated), dg=torch.tensor(dg),
                    keys=sorted(shapes), shapes=[list(shapes[k]) for k in sorted(shapes)])
        if not n_off:                           # depth-wise body: the flags are ignored (vovnet.py:292-298)
            plain = build_reference(body, (False,) * 4, False, 1)
            plain.load_state_dict(sd, strict=True)
            a, b = run(backbone, x, x32), run(plain, x, x32)
            assert all(torch.equal(a[k], b[k]) for k in a)
            print("  {}: identical to the plain {} body".format(name, body))
            out[name] = case
            continue
        case["out"] = run(backbone, x, x32)
        if n_off:
            offs = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("/conv_offset.bias")])
            print("  offset-conv biases: mean |b| %.3f" % float(offs.abs().mean()))
            for k, v in sd.items():              # offsets 0, mask logits +40 (sigmoid 1): the deformable convs become plain 3x3 convs
                if "/conv_offset." in k:
                    z = torch.zeros_like(v)
                    if modulated and k.endswith(".bias"):
                        z[18 * dg:] = 40.0
                    sd[k] = z
            backbone.load_state_dict(sd, strict=True)
            plain = run(backbone, x, x32)
            for k in case["out"]:
                d = float((case["out"][k] - plain[k]).abs().max())
                assert d > 0.05, (name, k, d)
                print("  {} {} absmax {:.3f}, |deformed - plain| max {:.3f}".format(name, k, float(case["out"][k].abs().max()), d))
        out[name] = case
    path = os.path.join(HERE, "vovnet_dcn.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
