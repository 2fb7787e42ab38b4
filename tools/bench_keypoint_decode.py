"""The keypoint heatmap decode (cmk_keypoint_decode) at the size a keypoint model would run it — bs 8 x 50 detections of an 800 x 1280
image, K = 17 — beside the convs that would feed it in the keypoint head (KRCNNConvDeconvUpsampleHead: eight 512-channel 3x3 convs on the
14 x 14 RoI maps, and score_lowres as a 3x3 conv with 4K outputs) on the existing conv library.  Device events, warm-up, interleaved,
best of `rounds`.  Reports the decode's work sum(Hc * Wc * K) over the valid detections and its rate.  A tool only: bench.py does not
run it.

    python tools/bench_keypoint_decode.py [--reps 20] [--rounds 3] [--out profiles/bench_keypoint_decode.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from centermask2_amd import ops  # noqa: E402
from centermask2_amd.ops import View  # noqa: E402

B, TOPK, K, S = 8, 50, 17, 14


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def boxes_like_detections(g):
    """(B, TOPK, 4): sides log-uniform over 16 .. 800 px, aspect within 1/2 .. 2, centres inside the 1280 x 800 image, clipped to it."""
    side = torch.empty(B, TOPK).uniform_(math.log(16.0), math.log(800.0), generator=g).exp()
    aspect = torch.empty(B, TOPK).uniform_(math.log(0.5), math.log(2.0), generator=g).exp()
    w, h = side * aspect.sqrt(), side / aspect.sqrt()
    cx, cy = torch.rand(B, TOPK, generator=g) * 1280, torch.rand(B, TOPK, generator=g) * 800
    b = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 2)
    b[..., 0::2] = b[..., 0::2].clamp(0, 1280)
    b[..., 1::2] = b[..., 1::2].clamp(0, 800)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    r = B * TOPK
    boxes = boxes_like_detections(g)
    counts = torch.full((B,), TOPK, dtype=torch.int32)
    w = (boxes[..., 2] - boxes[..., 0]).clamp(min=1).ceil()
    h = (boxes[..., 3] - boxes[..., 1]).clamp(min=1).ceil()
    pixels = float((w * h).sum()) * K

    x = View(torch.randn((r, S, S, 256), generator=g).to(dev))
    trunk = [ops.PackedConv(torch.randn((512, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5, None, torch.zeros(512), dev)
             for cin in [256] + [512] * 7]
    score = ops.PackedConv(torch.randn((4 * K, 512, 3, 3), generator=g) * (1.0 / 2048) ** 0.5, None, torch.zeros(4 * K), dev)
    ys = [View(torch.empty((r, S, S, 512), device=dev)) for _ in range(2)]
    dec = View(torch.empty((r, S, S, 4 * K), device=dev))
    bd, cd = boxes.to(dev), counts.to(dev)

    def run_trunk():
        src = x
        for i, pc in enumerate(trunk):
            ops.conv2d(src, pc, ys[i % 2], relu=True)
            src = ys[i % 2]

    fns = {"trunk_8_convs": run_trunk, "score_lowres_as_3x3": lambda: ops.conv2d(ys[1], score, dec),
           "decode": lambda: ops.keypoint_decode(dec, bd, cd, K)}
    for f in fns.values():
        f(); f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            ms[k].append(_timed(f, a.reps))
    best = {k: min(v) for k, v in ms.items()}
    branch = sum(best.values())
    trunk_flops = 2.0 * r * S * S * 9 * 512 * (256 + 7 * 512)
    res = dict(rois=r, keypoints=K, resolution=S, ms={k: round(v, 4) for k, v in best.items()},
               decode_share_of_branch=round(best["decode"] / branch, 4),
               decode_work_pixels=int(pixels), decode_gpix_per_s=round(pixels / best["decode"] / 1e6, 2),
               trunk_alg_tflops=round(trunk_flops / best["trunk_8_convs"] / 1e9, 1),
               box_side_px=dict(min=round(float(torch.minimum(w, h).min()), 1), max=round(float(torch.maximum(w, h).max()), 1)),
               variants={"trunk": list(ops._TUNED.values())} if ops._TUNED else "library defaults (cmk_conv_resolve), no tuned table")
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
