"""The ResNeXt path, measured at the bench shape (batch 8, 3 x 800 x 1280, STRIDE_IN_1X1 False):
  * the conv2 layers of X-101-32x8d, one problem per distinct shape: ops.group_conv3x3 (csrc/conv_group3.hip) beside the only way to run the
    same layer without it, a dense conv through ops.conv2d on the block-diagonal expansion of the weight (zeros outside the groups, 32x the
    multiplies), and beside the compulsory-traffic floor: input + output + weight bytes over the float4-copy rate measured in this
    session.  The two results are compared on the same input;
  * the X-101-32x8d CenterMask model as a graph-replayed inference_padded step beside R-101 (tools/bench_resnet.py's bench_model).
HIP-event times, best and worst of several interleaved rounds.  A tool only: bench.py does not run it.

    python tools/bench_resnext.py [--reps 10] [--rounds 3] [--out profiles/bench_resnext.json] [--no-models]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_resnet as BR  # noqa: E402  (the timing helpers and bench_model)
from centermask2_amd import ops  # noqa: E402
from centermask2_amd import synthetic as S  # noqa: E402
from centermask2_amd.ops import View  # noqa: E402

B = 8
GROUPS = 32
# (C, input map, stride) of the distinct conv2 problems of X-101-32x8d at 800 x 1280 with the stride on the 3x3
SHAPES = [(256, (200, 320), 1), (512, (200, 320), 2), (512, (100, 160), 1), (1024, (100, 160), 2), (1024, (50, 80), 1), (2048, (50, 80), 2),
          (2048, (25, 40), 1)]
FP32_TFLOPS = 157.3


def copy_rate(dev, reps, rounds):
    """TB/s of a device-to-device float4 copy (read + write) of 1 GiB."""
    src = torch.empty(1 << 28, device=dev).normal_()
    dst = torch.empty_like(src)
    us = BR._rounds({"copy": lambda: dst.copy_(src)}, reps, rounds)["copy"]
    return 2 * src.numel() * 4 / (us["best"] * 1e-6) / 1e12, us


def bench_layer(dev, c, hw, stride, reps, rounds, tbs):
    cg = c // GROUPS
    h, wd = hw
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    key = "backbone.bottom_up.res{}.1.conv2.".format({8: 2, 16: 3, 32: 4, 64: 5}[cg])
    w = S.synthetic_tensor(key + "weight", (c, cg, 3, 3))
    scale, shift = ops.fold_frozen_bn(*[S.synthetic_tensor(key + "norm." + n, (c,)) for n in ("weight", "bias", "running_mean", "running_var")])
    dense_w = torch.zeros((c, c, 3, 3))
    for g in range(GROUPS):
        dense_w[g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
    pg = ops.PackedGroupConv(w, scale, shift, dev, GROUPS, stride=stride)
    pd = ops.PackedConv(dense_w, scale, shift, dev, stride=stride)
    del dense_w
    x = View(torch.relu(torch.randn((B, h, wd, c), device=dev)))
    yg = View(torch.empty((B, ho, wo, c), device=dev))
    yd = View(torch.empty((B, ho, wo, c), device=dev))
    us = BR._rounds({"grouped": lambda: ops.group_conv3x3(x, pg, yg, relu=True), "block_diagonal_dense": lambda: ops.conv2d(x, pd, yd, relu=True)}, reps, rounds)
    torch.cuda.synchronize()
    diff = float((yg.t - yd.t).abs().max())
    nbytes = 4 * (B * h * wd * c + B * ho * wo * c + 9 * cg * c)
    flops = 2.0 * 9 * cg * c * B * ho * wo
    floor_us = nbytes / (tbs * 1e12) * 1e6
    best = us["grouped"]["best"]
    res = dict(C=c, Cg=cg, input_map=[h, wd], stride=stride, us=us, max_abs_diff_grouped_vs_dense=diff, max_abs_out=float(yd.t.abs().max()),
               compulsory_bytes=nbytes, traffic_floor_us=round(floor_us, 1), floor_over_time=round(floor_us / best, 3), flops=flops,
               achieved_tflops=round(flops / (best * 1e-6) / 1e12, 2), compute_floor_us=round(flops / (FP32_TFLOPS * 1e12) * 1e6, 1),
               achieved_tb_per_s=round(nbytes / (best * 1e-6) / 1e12, 2), dense_over_grouped=round(us["block_diagonal_dense"]["best"] / best, 2))
    del pg, pd, x, yg, yd
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-models", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_autotune(False)
    with torch.no_grad():
        tbs, copy_us = copy_rate(dev, a.reps, a.rounds)
        layers = []
        for c, hw, stride in SHAPES:
            layers.append(bench_layer(dev, c, hw, stride, a.reps, a.rounds, tbs))
            print(json.dumps(layers[-1]), flush=True)
        models = []
        if not a.no_models:
            mreps = max(a.reps // 2, 1)
            models = [BR.bench_model("centermask_X_101_32x8d_FPN_ms_3x.yaml", "X-101-32x8d", dev, mreps, a.rounds),
                      BR.bench_model("centermask_R_101_FPN_ms_3x.yaml", "R-101", dev, mreps, a.rounds)]
            for m in models:
                m["variants"] = "library defaults"
    res = dict(layers=layers, grouped_faster_at_every_shape=all(l["us"]["grouped"]["best"] < l["us"]["block_diagonal_dense"]["best"] for l in layers),
               models=models, rates=dict(float4_copy_tb_per_s_this_session=round(tbs, 3), copy_us=copy_us, fp32_tflops_peak=FP32_TFLOPS),
               batch=B, groups=GROUPS, reps=a.reps, rounds=a.rounds)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
