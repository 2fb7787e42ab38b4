"""The mask head's four 3x3 convs on the RoI features of a real (synthetic-weight V-99) forward pass, layer by layer, on the direct form (2/16/4)
and on F(2x2,3x3) (5/16/2), each against a float64 convolution of the same input: post-ReLU sparsity and trained-scale weights, which the seeded
N(0,1) data of conv_probe.py check does not have.  python tools/diag_mask.py"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, torch.nn.functional as F
from centermask2_amd import ops, synthetic as S
from centermask2_amd.ops import View
from tests.helpers import build_gpu_model
model, sd = build_gpu_model("V-99-eSE")
x = S.make_synthetic_images(1, 128, 192, seed0=555)
with torch.no_grad():
    out = model.inference_padded(x.cuda(), [(128, 192)], want=("roi_feat",))
roi = out["roi_feat"]          # (50,14,14,256)
print("roi", tuple(roi.shape), float(roi.abs().max()), float(roi.abs().mean()), "zeros frac", float((roi == 0).float().mean()))
xin = View(roi.contiguous())
for k in range(1, 5):
    w = sd["roi_heads.mask_head.mask_fcn%d.weight" % k]; b = sd["roi_heads.mask_head.mask_fcn%d.bias" % k]
    pc = ops.PackedConv(w, None, b, "cuda")
    ref = F.relu(F.conv2d(xin.t.permute(0, 3, 1, 2).cpu().double(), w.double(), b.double(), padding=1)).float()
    res = {}
    for name, tv in (("direct", (2, 16, 4)), ("wino", (5, 16, 2))):
        y = View(torch.empty((50, 14, 14, 256), device="cuda"))
        launch = ops._ConvLaunch([xin], [pc], [y], relu=True, single=True)
        launch.set(tv)
        launch.launch()
        torch.cuda.synchronize()
        got = y.t.permute(0, 3, 1, 2).cpu()
        err = (got - ref).abs()
        res[name] = y
        print("layer", k, name, "max ref %.3g max err %.3g rms rel %.2e  worst idx %s" % (ref.abs().max(), err.max(), err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt(), tuple(int(v) for v in torch.nonzero(err == err.max())[0])))
    xin = res["direct"]
