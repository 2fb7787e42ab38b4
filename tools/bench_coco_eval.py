"""COCOEvaluator.process() per image: Instances on the GPU against the same Instances on the host, at the bench shape — 8 images x 50
detections at 800 x 1280 against 10 ground truths per image (compressed RLE in the annotation dict), masks pasted from seeded boxes and
smooth blobs as in tools/bench_rle.py.  A tool only: bench.py does not run it.

  (A) process() on the CPU copies of the Instances  — wire.rle_encode per mask + coco_eval.intersections_host; the copies are made
                                                      beforehand, so the 51 MB download per image is NOT in A's time (it is reported
                                                      on its own line: a user whose model runs on the GPU pays it on top)
  (B) process() on the GPU Instances                — ops.mask_rle + ops.mask_intersections (csrc/rle.hip, csrc/mask_iou.hip)

The intersection tables and both area vectors of the two paths are asserted equal on every image before anything is timed.  A and B
alternate in one process after a warm-up of both (which also rasterises the ground truth once); each round is timed with a host clock
around work that ends in the device-to-host copy of the table.

    python tools/bench_coco_eval.py [--rounds 10] [--out profiles/bench_coco_eval.json]

Kernel times come from a run of their own, with no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o coco -- python tools/bench_coco_eval.py --trace-body
    python tools/bench_coco_eval.py --kernel-stats DIR/.../coco_kernel_stats.csv --out profiles/bench_coco_eval.json

The second command adds the mask IoU kernels' time per image to the json beside their memory bounds at the 6.3 TB/s an MI355X achieves
from HBM: the pack kernel reads R*H*W bytes, the intersection kernel (N + M)*H*W/8 bytes.

The Boundary AP leg is a run of its own (boundary_leg below; written to the key "boundary" of --out, the rest of the file kept):

    python tools/bench_coco_eval.py --boundary [--rounds 10] [--host-rounds 3] [--out profiles/bench_coco_eval.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bnd -- python tools/bench_coco_eval.py --boundary --trace-body
    python tools/bench_coco_eval.py --boundary --kernel-stats DIR/.../bnd_kernel_stats.csv --out profiles/bench_coco_eval.json
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

from centermask2_amd import ops, wire  # noqa: E402
from centermask2_amd.evaluation import COCOEvaluator  # noqa: E402
from centermask2_amd.structures import Boxes, Instances  # noqa: E402

B, TOPK, NGT, H, W, S = 8, 50, 10, 800, 1280, 28
NCAT = 3
HBM_BYTES_PER_S = 6.3e12            # achievable HBM bandwidth of an MI355X
TRACE_CALLS = 5                     # --trace-body: process() of every image under the profiler
KERNELS = ("mask_pack_kernel", "rle_decode_pack_kernel", "words_area_kernel", "mask_inter_kernel")


def _paste(dev, n, g):
    """n (H,W) bool bitmasks on the device and their boxes, pasted from seeded boxes and blobs."""
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
    return ops.paste_masks(soft.clamp(0, 1).float().to(dev), boxes.to(dev), H, W), boxes


def workload(dev):
    """-> (annotation dict, [(image id, Instances on the device)])."""
    g = torch.Generator().manual_seed(7)
    images, anns, per_image = [], [], []
    for i in range(B):
        img = i + 1
        images.append({"id": img, "height": H, "width": W})
        gt_masks, gt_boxes = _paste(dev, NGT, g)
        for k, (m, bx) in enumerate(zip(gt_masks.cpu().numpy(), gt_boxes.tolist())):
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1 + k % NCAT, "iscrowd": int(k == NGT - 1), "area": float(m.sum()),
                         "bbox": [bx[0], bx[1], bx[2] - bx[0], bx[3] - bx[1]], "segmentation": wire.rle_encode(m)})
        masks, boxes = _paste(dev, TOPK, g)
        inst = Instances((H, W), pred_boxes=Boxes(boxes.to(dev)), scores=torch.rand(TOPK, generator=g).to(dev),
                         pred_classes=torch.randint(0, NCAT, (TOPK,), generator=g).to(dev), pred_masks=masks,
                         mask_scores=torch.rand(TOPK, generator=g).to(dev))
        per_image.append((img, inst))
    ds = {"images": images, "categories": [{"id": c + 1, "name": "c{}".format(c + 1)} for c in range(NCAT)], "annotations": anns}
    return ds, per_image


def _round(ev, per_image):
    ev.reset()
    t0 = time.perf_counter()
    for img, inst in per_image:
        ev.process([{"image_id": img}], [{"instances": inst}])
    return (time.perf_counter() - t0) * 1e3 / len(per_image)


def _spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "rounds": len(ms)}


def kernel_stats(path):
    """rocprofv3's kernel_stats.csv of a --trace-body run -> the mask IoU kernels' time per image beside their memory bounds."""
    per_kernel = {}
    for row in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in row["Name"]:
                per_kernel[k] = {"calls": int(row["Calls"]), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 2)}
    missing = [k for k in KERNELS if k not in per_kernel]
    if missing:
        raise SystemExit("{}: no row for {}".format(path, missing))
    calls = per_kernel["mask_pack_kernel"]["calls"]
    if calls != B * TRACE_CALLS:
        raise SystemExit("{}: {} pack launches, a --trace-body run makes {}".format(path, calls, B * TRACE_CALLS))
    us = {k: round(v["total_us"] / calls, 2) for k, v in per_kernel.items()}
    pack_bound = TOPK * H * W / HBM_BYTES_PER_S * 1e6
    inter_bound = (TOPK + NGT) * H * W / 8 / HBM_BYTES_PER_S * 1e6
    return {"source": "rocprofv3 --kernel-trace --stats, {} process() calls on each of the {} images".format(TRACE_CALLS, B),
            "per_kernel": per_kernel, "us_per_image": us, "kernels_us_per_image": round(sum(us.values()), 2),
            "pack_memory_bound_us_per_image": round(pack_bound, 2), "pack_memory_bound": "R * H * W bytes at 6.3 TB/s",
            "pack_share_of_memory_bound": round(pack_bound / us["mask_pack_kernel"], 3),
            "intersections_memory_bound_us_per_image": round(inter_bound, 2), "intersections_memory_bound": "(N + M) * H * W / 8 bytes at 6.3 TB/s",
            "intersections_share_of_memory_bound": round(inter_bound / us["mask_inter_kernel"], 3)}


def boundary_leg(a, dev):
    """--boundary: what the task "boundary" (Boundary AP) adds to process() at the same shape, erosion distance 30.  Three timings in
    alternating rounds after a warm-up of all: process() on GPU Instances without and with the task, and with it on the CPU copies (fewer
    rounds: a host round takes seconds).  Both tables of the two paths are asserted equal first.  The entry cmk_mask_boundary_bits on the
    60 packed masks of one image is timed on its own with device events (the zeroing of words and areas and the boundary kernel together)
    beside the memory floor of the boundary kernel: the words read once and written once."""
    ds, gpu_images = workload(dev)
    torch.cuda.synchronize()
    plain, with_b = COCOEvaluator(ds), COCOEvaluator(ds, tasks=("bbox", "segm", "boundary"))
    d = ops.boundary_dilation(H, W)
    cpu_images = [(img, inst.to("cpu")) for img, inst in gpu_images]
    _round(plain, gpu_images)
    _round(with_b, gpu_images)
    on_gpu = [p["table"] + p["boundary_table"] for p in with_b._predictions]
    _round(with_b, cpu_images)
    on_cpu = [p["table"] + p["boundary_table"] for p in with_b._predictions]
    for ta, tb in zip(on_gpu, on_cpu):
        assert len(ta) == 6 and all(np.array_equal(x, y) for x, y in zip(ta, tb)), "mask or boundary tables of the two paths differ"
    t_plain, t_b, t_host = [], [], []
    for k in range(a.rounds):
        t_plain.append(_round(plain, gpu_images))
        t_b.append(_round(with_b, gpu_images))
        if k < a.host_rounds:
            t_host.append(_round(with_b, cpu_images))
    # the entry alone, on the packed masks of one image
    inst = gpu_images[0][1]
    words = torch.cat([ops.mask_pack_bits(inst.pred_masks)[0], ops.mask_rle_decode(with_b._gt.counts(gpu_images[0][0]), H, W, want_bitmasks=False)[0]])
    for _ in range(5):
        ops.mask_boundary_bits(words, H, W, d)
    torch.cuda.synchronize()
    us = []
    for _ in range(max(a.rounds, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.mask_boundary_bits(words, H, W, d)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    floor_us = 2 * words.numel() * 8 / HBM_BYTES_PER_S * 1e6
    return {
        "workload": "{} images x {} detections against {} ground truths of {}x{}, erosion distance {}".format(B, TOPK, NGT, H, W, d),
        "tables_equal": True,
        "device_ms_per_image_without_boundary": _spread(t_plain),
        "device_ms_per_image_with_boundary": _spread(t_b),
        "host_ms_per_image_with_boundary": _spread(t_host),
        "host_over_device_median": round(statistics.median(t_host) / statistics.median(t_b), 2),
        "boundary_entry_us": {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2), "calls": len(us),
                              "masks": int(words.shape[0]),
                              "what": "cmk_mask_boundary_bits between two device events: zeroing of words and areas, mask_boundary_kernel"},
        "boundary_memory_floor_us": round(floor_us, 2),
        "boundary_memory_floor": "2 * R * ceil(H*W/64) * 8 bytes (words read once, written once) at 6.3 TB/s",
        "boundary_entry_share_of_memory_floor": round(floor_us / statistics.median(us), 3),
        "timing": "host clock around each round of {} process() calls, the three alternating, {} device and {} host rounds after a warm-up "
                  "of all".format(B, a.rounds, len(t_host)),
        "device": torch.cuda.get_device_name(0),
    }


BOUNDARY_TRACE_CALLS = 20


def boundary_trace_body(dev):
    """--boundary --trace-body: the entry alone on the 60 packed masks of the first image, for rocprofv3 --kernel-trace."""
    ds, gpu_images = workload(dev)
    img, inst = gpu_images[0]
    gt = COCOEvaluator(ds)._gt.counts(img)
    words = torch.cat([ops.mask_pack_bits(inst.pred_masks)[0], ops.mask_rle_decode(gt, H, W, want_bitmasks=False)[0]])
    for _ in range(BOUNDARY_TRACE_CALLS):
        ops.mask_boundary_bits(words, H, W, ops.boundary_dilation(H, W))
    torch.cuda.synchronize()


def boundary_kernel_stats(path):
    """kernel_stats.csv of a --boundary --trace-body run -> the boundary kernel's time per call beside its memory floor."""
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}
    name = [n for n in rows if "mask_boundary_kernel" in n]
    if not name or int(rows[name[0]]["Calls"]) != BOUNDARY_TRACE_CALLS:
        raise SystemExit("{}: not the {} mask_boundary_kernel launches of a --boundary --trace-body run".format(path, BOUNDARY_TRACE_CALLS))
    us = float(rows[name[0]]["TotalDurationNs"]) / 1e3 / BOUNDARY_TRACE_CALLS
    floor_us = 2 * (TOPK + NGT) * ((H * W + 63) // 64) * 8 / HBM_BYTES_PER_S * 1e6
    return {"source": "rocprofv3 --kernel-trace --stats, {} calls of the entry on {} masks".format(BOUNDARY_TRACE_CALLS, TOPK + NGT),
            "mask_boundary_kernel_us": round(us, 2), "memory_floor_us": round(floor_us, 2),
            "share_of_memory_floor": round(floor_us / us, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--boundary", action="store_true", help="the Boundary AP leg; written to the key \"boundary\" of --out")
    ap.add_argument("--host-rounds", type=int, default=3, help="--boundary: rounds of the host path")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-body", action="store_true", help="only run the device path a few times (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --trace-body run; merged into --out")
    a = ap.parse_args()

    if a.kernel_stats and a.boundary:
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        res.setdefault("boundary", {})["kernel"] = boundary_kernel_stats(a.kernel_stats)
        print(json.dumps(res["boundary"]["kernel"]))
        if a.out:
            json.dump(res, open(a.out, "w"), indent=1)
        return
    if a.kernel_stats:
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        res["kernels"] = kernel_stats(a.kernel_stats)
        print(json.dumps(res["kernels"]))
        if a.out:
            json.dump(res, open(a.out, "w"), indent=1)
        return

    if not torch.cuda.is_available():
        raise SystemExit("bench_coco_eval needs the MI355X: nothing about speed is stated from a CPU run")
    if a.rounds < 10 and not a.trace_body:
        raise SystemExit("at least 10 rounds of each path")
    dev = torch.device("cuda:0")
    if a.boundary and a.trace_body:
        boundary_trace_body(dev)
        return
    if a.boundary:
        if a.host_rounds < 3:
            raise SystemExit("at least 3 rounds of the host path")
        res = boundary_leg(a, dev)
        print(json.dumps(res))
        if a.out:
            old = json.load(open(a.out)) if os.path.exists(a.out) else {}
            if "kernel" in old.get("boundary", {}):
                res["kernel"] = old["boundary"]["kernel"]
            old["boundary"] = res
            json.dump(old, open(a.out, "w"), indent=1)
        return
    ds, gpu_images = workload(dev)
    torch.cuda.synchronize()
    ev = COCOEvaluator(ds)

    if a.trace_body:
        for _ in range(TRACE_CALLS):
            _round(ev, gpu_images)
        torch.cuda.synchronize()
        return

    t0 = time.perf_counter()
    cpu_images = [(img, inst.to("cpu")) for img, inst in gpu_images]
    download_ms = (time.perf_counter() - t0) * 1e3 / B
    # equality first; this is also the warm-up of both paths and rasterises the ground truth
    _round(ev, gpu_images)
    on_gpu = [(p["instances"], p["table"]) for p in ev._predictions]
    _round(ev, cpu_images)
    on_cpu = [(p["instances"], p["table"]) for p in ev._predictions]
    for (ra, ta), (rb, tb) in zip(on_gpu, on_cpu):
        assert ra == rb, "result records of the two paths differ"
        assert all(np.array_equal(x, y) for x, y in zip(ta, tb)), "intersection tables of the two paths differ"
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(_round(ev, cpu_images))
        tb.append(_round(ev, gpu_images))
    res = {
        "workload": "{} images x {} detections against {} ground truths of {}x{}, seeded boxes (sides 20 px .. image) and blob masks; paste "
                    "not timed".format(B, TOPK, NGT, H, W),
        "tables_equal": True,
        "host_ms_per_image": _spread(ta),
        "device_ms_per_image": _spread(tb),
        "host_over_device_median": round(statistics.median(ta) / statistics.median(tb), 2),
        "device_faster_beyond_spread": max(tb) < min(ta),
        "instances_to_cpu_ms_per_image": round(download_ms, 3),
        "instances_to_cpu_note": "one untimed-path measurement of Instances.to('cpu') per image; not part of host_ms_per_image",
        "d2h_bytes_per_image": {"host": TOPK * H * W, "device_table": 4 * (TOPK * NGT + TOPK + NGT)},
        "timing": "host clock around each round of {} process() calls, A and B alternating, {} rounds after a warm-up of both".format(B, a.rounds),
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
