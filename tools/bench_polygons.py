"""Contours of pasted bitmasks: the host path against the device tracer at the bench shape — the workload of tools/bench_rle.py, 8 images
x 50 detections at 800 x 1280, seeded boxes and blob masks.  The paste runs once and is not timed.  A tool only: bench.py does not run it,
and none of its numbers is a gate.

  (A) masks.cpu() followed by wire.mask_contours_host per mask — the host path (CPU inputs still take it): the reference, there is no
                                                                  earlier polygon path to compare with
  (B) ops.mask_contours on the GPU tensor                       — the vis_contour_* kernels of csrc/visualize.hip
  (C) ops.mask_rle on the same masks                            — the yardstick: a two-pass encoder over the same masks

The loops of A and B are asserted equal on every mask before anything is timed.  A, B and C alternate in one process after a warm-up of
all; each round is timed with a host clock around work that ends in the device-to-host copy.  B is also timed phase by phase, each phase
closed by a device synchronise: pack, count (with the read of the totals), trace, download with the split into loops.  Reported per
image: median, minimum and maximum over the rounds, and the device-to-host bytes of each path.

    python tools/bench_polygons.py [--rounds 10] [--out profiles/bench_polygons.json]

Kernel times come from a run of their own, with no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o poly -- python tools/bench_polygons.py --trace-body
    python tools/bench_polygons.py --kernel-stats DIR/.../poly_kernel_stats.csv --out profiles/bench_polygons.json

The second command adds the kernels' time per image to the json and states the count kernel's share of its read-once memory floor,
R * ceil(H*W/64) * 8 bytes at the 6.3 TB/s an MI355X achieves from HBM.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_rle  # noqa: E402  the workload
from bench_rle import B, H, HBM_BYTES_PER_S, TOPK, W, _round, _spread  # noqa: E402
from centermask2_amd import ops, wire  # noqa: E402

TRACE_CALLS = 5
KERNELS = ("vis_contour_count_kernel", "vis_contour_offsets_kernel", "vis_contour_emit_kernel", "vis_contour_link_kernel",
           "vis_contour_jump_kernel", "vis_contour_lens_kernel", "vis_contour_blocks_kernel", "vis_contour_place_kernel",
           "vis_contour_write_kernel")


def path_a(masks):
    return [wire.mask_contours_host(m) for m in masks.cpu().numpy()]


def path_b(masks):
    return ops.mask_contours(masks)


def path_c(masks):
    return ops.mask_rle(masks)


def phases(masks):
    """One ops.mask_contours, phase by phase -> milliseconds of (pack, count, trace, download)."""
    sync = torch.cuda.synchronize
    sync()
    t0 = time.perf_counter()
    words, _ = ops.mask_pack_bits(masks)
    sync()
    t1 = time.perf_counter()
    ws, ws_bytes, n_dev = ops._contour_count(words, H, W)
    n_host = np.ascontiguousarray(n_dev.cpu().numpy(), dtype=np.int32)
    t2 = time.perf_counter()
    out = ops._contour_trace(words, H, W, ws, ws_bytes, n_host)
    sync()
    t3 = time.perf_counter()
    ops._contour_split(out.cpu().numpy(), n_host)
    t4 = time.perf_counter()
    return [(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4))]


def kernel_stats(path):
    """rocprofv3's kernel_stats.csv of a --trace-body run -> the contour kernels' time per image, the count kernel against its floor."""
    per_kernel = {}
    for row in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in row["Name"]:
                per_kernel[k] = {"calls": int(row["Calls"]), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 2)}
    missing = [k for k in KERNELS if k not in per_kernel]
    if missing:
        raise SystemExit("{}: no row for {}".format(path, missing))
    calls = per_kernel["vis_contour_count_kernel"]["calls"]
    if calls != B * TRACE_CALLS:
        raise SystemExit("{}: {} count launches, a --trace-body run makes {}".format(path, calls, B * TRACE_CALLS))
    us_per_image = sum(v["total_us"] for v in per_kernel.values()) / calls
    count_us = per_kernel["vis_contour_count_kernel"]["total_us"] / calls
    floor_us = TOPK * ((H * W + 63) // 64) * 8 / HBM_BYTES_PER_S * 1e6
    return {"source": "rocprofv3 --kernel-trace --stats, {} traces of each of the {} images".format(TRACE_CALLS, B),
            "per_kernel": per_kernel, "kernels_us_per_image": round(us_per_image, 2),
            "jump_launches_per_image": round(per_kernel["vis_contour_jump_kernel"]["calls"] / calls, 1),
            "count_kernel_us_per_image": round(count_us, 2),
            "memory_floor_us_per_image": round(floor_us, 3), "memory_floor": "R * ceil(H*W/64) * 8 bytes read once at 6.3 TB/s",
            "count_kernel_share_of_memory_floor": round(floor_us / count_us, 4)}


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
        raise SystemExit("bench_polygons needs the MI355X: nothing about speed is stated from a CPU run")
    if a.rounds < 10 and not a.trace_body:
        raise SystemExit("at least 10 rounds of each path")
    dev = torch.device("cuda:0")
    images = bench_rle.workload(dev)
    torch.cuda.synchronize()

    if a.trace_body:
        for _ in range(TRACE_CALLS):
            for m in images:
                path_b(m)
        torch.cuda.synchronize()
        return

    corners, loops = [], []
    for m in images:                                    # equality first; this is also the warm-up of all paths
        ra, rb = path_a(m), path_b(m)
        assert len(ra) == len(rb) and all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(ra, rb)), \
            "device and host contours differ"
        corners += [sum(len(lp) for lp in x) for x in rb]
        loops += [len(x) for x in rb]
        path_c(m), phases(m)
    ta, tb, tc, tp = [], [], [], []
    for _ in range(a.rounds):
        ta.append(_round(path_a, images))
        tb.append(_round(path_b, images))
        tc.append(_round(path_c, images))
        tp.append([sum(v) / len(images) for v in zip(*[phases(m) for m in images])])
    total = sum(corners)
    nw = (H * W + 63) // 64
    res = {
        "workload": "{} images x {} masks of {}x{}, seeded boxes (sides 20 px .. image) and blob masks; paste not timed".format(B, TOPK, H, W),
        "corners_per_mask": {"min": min(corners), "median": statistics.median(corners), "max": max(corners)},
        "loops_per_mask": {"min": min(loops), "median": statistics.median(loops), "max": max(loops)},
        "loops_equal": True,
        "host_ms_per_image": _spread(ta),
        "device_ms_per_image": _spread(tb),
        "device_phase_ms_per_image": {k: _spread([r[i] for r in tp]) for i, k in enumerate(("pack", "count", "trace", "download_split"))},
        "rle_device_ms_per_image": _spread(tc),
        "host_over_device_median": round(statistics.median(ta) / statistics.median(tb), 2),
        "device_faster_beyond_spread": max(tb) < min(ta),
        "d2h_bytes_per_image": {"host": TOPK * H * W, "device": round((4 * B * TOPK + 12 * total) / B)},
        "count_read_once_floor_bytes_per_image": TOPK * nw * 8,
        "timing": "host clock around each round of {} images, A, B and C alternating, {} rounds after a warm-up of all; "
                  "phases in rounds of their own, each closed by a synchronise".format(B, a.rounds),
        "gate": "none: no number here is asserted anywhere",
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(res))
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        if "kernels" in old:
            res["kernels"] = old["kernels"]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
