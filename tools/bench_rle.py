"""COCO RLE of pasted bitmasks: the host codec against the device encoder at the bench shape — 8 images x 50 detections at 800 x 1280,
box sides between 20 px and the image size, soft masks that are smooth blobs (so the run counts are those of real masks).  The paste runs
once and is not timed.  A tool only: bench.py does not run it.

  (A) masks.cpu() followed by wire.rle_encode per mask        — the host path (CPU inputs still take it)
  (B) wire.rle_encode_batch on the GPU tensor                  — csrc/rle.hip through ops.mask_rle

The strings of the two paths are asserted equal on every mask before anything is timed.  A and B alternate in one process after a
warm-up of both; each round is timed with a host clock around work that ends in the device-to-host copy.  Reported per image: median,
minimum and maximum over the rounds, and the device-to-host bytes of each path.

    python tools/bench_rle.py [--rounds 10] [--out profiles/bench_rle.json]

Kernel times come from a run of their own, with no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o rle -- python tools/bench_rle.py --trace-body
    python tools/bench_rle.py --kernel-stats DIR/.../rle_kernel_stats.csv --out profiles/bench_rle.json

The second command adds the kernels' time per image to the json, against the memory bound of reading every bitmap byte twice,
2 * R * H * W bytes at the 6.3 TB/s an MI355X achieves from HBM, and names the result as a share of that bound.
"""
import argparse
import csv
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from centermask2_amd import ops, wire  # noqa: E402

B, TOPK, H, W, S = 8, 50, 800, 1280, 28
HBM_BYTES_PER_S = 6.3e12            # achievable HBM bandwidth of an MI355X
TRACE_CALLS = 5                     # --trace-body: encodes of every image under the profiler
KERNELS = ("rle_count_kernel", "rle_scan_kernel", "rle_offsets_kernel", "rle_starts_kernel", "rle_string_kernel")


def workload(dev):
    """Per image (TOPK, H, W) bool bitmasks on the device, pasted from seeded boxes and blobs."""
    g = torch.Generator().manual_seed(7)
    n = B * TOPK
    bw = torch.empty(n).uniform_(math.log(20.0), math.log(float(W)), generator=g).exp()
    bh = torch.empty(n).uniform_(math.log(20.0), math.log(float(H)), generator=g).exp()
    x0, y0 = torch.rand(n, generator=g) * (W - bw), torch.rand(n, generator=g) * (H - bh)
    boxes = torch.stack([x0, y0, x0 + bw, y0 + bh], 1)
    u = torch.linspace(-1, 1, S)
    vv, uu = torch.meshgrid(u, u, indexing="ij")
    r = lambda lo, hi: (torch.rand(n, 1, 1, generator=g) * (hi - lo) + lo)  # noqa: E731
    cx, cy, sx, sy = r(-0.3, 0.3), r(-0.3, 0.3), r(0.4, 0.9), r(0.4, 0.9)
    a, b, ph = r(-4, 4), r(-4, 4), r(0, 6.28)
    soft = torch.exp(-(((uu - cx) / sx) ** 2 + ((vv - cy) / sy) ** 2)) * (1.0 + 0.3 * torch.sin(a * uu + b * vv + ph))
    soft = soft.clamp(0, 1).float()
    return [ops.paste_masks(soft[i * TOPK:(i + 1) * TOPK].to(dev), boxes[i * TOPK:(i + 1) * TOPK].to(dev), H, W) for i in range(B)]


def path_a(masks):
    return [wire.rle_encode(m) for m in masks.cpu()]


def path_b(masks):
    return wire.rle_encode_batch(masks)


def _round(fn, images):
    t0 = time.perf_counter()
    for m in images:
        fn(m)
    return (time.perf_counter() - t0) * 1e3 / len(images)


def _spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "rounds": len(ms)}


def kernel_stats(path):
    """rocprofv3's kernel_stats.csv of a --trace-body run -> the RLE kernels' time per image and its share of the memory bound."""
    per_kernel = {}
    for row in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in row["Name"]:
                per_kernel[k] = {"calls": int(row["Calls"]), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 2)}
    missing = [k for k in KERNELS if k not in per_kernel]
    if missing:
        raise SystemExit("{}: no row for {}".format(path, missing))
    calls = per_kernel["rle_count_kernel"]["calls"]
    if calls != B * TRACE_CALLS:
        raise SystemExit("{}: {} count launches, a --trace-body run makes {}".format(path, calls, B * TRACE_CALLS))
    us_per_image = sum(v["total_us"] for v in per_kernel.values()) / calls
    walk_us = (per_kernel["rle_count_kernel"]["total_us"] + per_kernel["rle_starts_kernel"]["total_us"]) / calls
    bound_us = 2.0 * TOPK * H * W / HBM_BYTES_PER_S * 1e6
    return {"source": "rocprofv3 --kernel-trace --stats, {} encodes of each of the {} images".format(TRACE_CALLS, B),
            "per_kernel": per_kernel, "kernels_us_per_image": round(us_per_image, 2),
            "count_plus_starts_us_per_image": round(walk_us, 2),
            "memory_bound_us_per_image": round(bound_us, 2), "memory_bound": "2 * R * H * W bytes at 6.3 TB/s",
            "share_of_memory_bound_all_kernels": round(bound_us / us_per_image, 3),
            "share_of_memory_bound_count_plus_starts": round(bound_us / walk_us, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-body", action="store_true", help="only run the device path a few times (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --trace-body run; merged into --out")
    a = ap.parse_args()

    if a.kernel_stats:
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        res["kernels"] = kernel_stats(a.kernel_stats)
        print(json.dumps(res["kernels"]))
        if a.out:
            json.dump(res, open(a.out, "w"), indent=1)
        return

    if not torch.cuda.is_available():
        raise SystemExit("bench_rle needs the MI355X: nothing about speed is stated from a CPU run")
    if a.rounds < 10 and not a.trace_body:
        raise SystemExit("at least 10 rounds of each path")
    dev = torch.device("cuda:0")
    images = workload(dev)
    torch.cuda.synchronize()

    if a.trace_body:
        for _ in range(TRACE_CALLS):
            for m in images:
                path_b(m)
        torch.cuda.synchronize()
        return

    runs, chars = [], []
    for m in images:                                    # equality first; this is also the warm-up of both paths
        ra, rb = path_a(m), path_b(m)
        assert ra == rb, "device and host RLE differ"
        runs += [len(c) for c in ops.mask_rle(m)[0]]
        chars += [len(r["counts"]) for r in rb]
    _round(path_a, images), _round(path_b, images)
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(_round(path_a, images))
        tb.append(_round(path_b, images))
    total_runs = sum(runs)
    res = {
        "workload": "{} images x {} masks of {}x{}, seeded boxes (sides 20 px .. image) and blob masks; paste not timed".format(B, TOPK, H, W),
        "runs_per_mask": {"min": min(runs), "median": statistics.median(runs), "max": max(runs)},
        "string_chars_per_mask": {"min": min(chars), "median": statistics.median(chars), "max": max(chars)},
        "strings_equal": True,
        "host_ms_per_image": _spread(ta),
        "device_ms_per_image": _spread(tb),
        "host_over_device_median": round(statistics.median(ta) / statistics.median(tb), 2),
        "device_faster_beyond_spread": max(tb) < min(ta),
        "d2h_bytes_per_image": {"host": TOPK * H * W, "device": round((12 * B * TOPK + 11 * total_runs) / B)},
        "timing": "host clock around each round of {} images, A and B alternating, {} rounds after a warm-up of both".format(B, a.rounds),
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(res))
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        if "kernels" in old:
            res["kernels"] = old["kernels"]
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
