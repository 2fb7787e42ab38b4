"""CityscapesInstanceEvaluator.process() per image: Instances on the GPU against the same Instances on the host, at the size of a
Cityscapes frame — 1024 x 2048, a synthetic label image of about 60 ground-truth regions (elliptic instances of the eight classes, a few
group regions, void strips), and 50 and 100 elliptic blob predictions (half of them jittered copies of ground-truth regions).  A tool
only: bench.py does not run it.  Every number is reported, none is gated.

  (A) process() on the CPU copies of the Instances  — cityscapes_eval.label_counts_host; the copies are made beforehand, so the
                                                      download of the bitmaps is NOT in A's time (reported on its own line)
  (B) process() on the GPU Instances                — ops.mask_label_counts (csrc/mask_iou.hip pack, csrc/eval/label_counts.hip)

Both build the columns of the label image on the host (cityscapes_eval.columns, timed on its own line too).  The tables and areas of
the two paths are asserted equal before anything is timed.  A and B alternate in one process after a warm-up of both; each round is
timed with a host clock around work that ends in the device-to-host copy of the table.  The entry cmk_mask_label_counts alone (the
zeroing of the table and the kernel) is timed between two device events.  The default loader read_label_png is timed per image on two
files of the same label image, one written with the Up filter (undone by NumPy) and one with Paeth (undone in a Python loop).

    python tools/bench_cityscapes_eval.py [--rounds 10] [--out profiles/bench_cityscapes_eval.json]

The kernel's own time comes from a run of its own, with no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o city -- python tools/bench_cityscapes_eval.py --trace-body
    python tools/bench_cityscapes_eval.py --kernel-stats DIR/.../city_kernel_stats.csv --out profiles/bench_cityscapes_eval.json

The second command adds the kernel's time per call at 100 predictions beside its read-once floor, N*H*W/8 + 2*H*W bytes (every packed
word and every label once) at the 6.3 TB/s an MI355X achieves from HBM."""
import argparse
import csv
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from centermask2_amd import cityscapes_eval as ce, ops  # noqa: E402
from centermask2_amd.evaluation import CityscapesInstanceEvaluator  # noqa: E402
from centermask2_amd.structures import Instances  # noqa: E402

H, W = 1024, 2048
COUNTS = (50, 100)
NAME = "bench_000000_000019"
HBM_BYTES_PER_S = 6.3e12            # achievable HBM bandwidth of an MI355X
TRACE_N, TRACE_CALLS = 100, 20


def label_image(rng):
    """-> ((H,W) uint16 label image, [(cy, cx, ry, rx, class index)] of its instance regions)."""
    g = np.full((H, W), 7, dtype=np.uint16)
    g[:300] = 23                                                       # sky
    g[300:450] = 11                                                    # building
    g[940:] = 1                                                        # ego vehicle: void
    g[:, :12] = 3                                                      # out of roi: void
    yy, xx = np.mgrid[0:H, 0:W]
    ellipses, serial = [], {}
    for k in range(56):
        ci = int(rng.randint(0, len(ce.CLASSES)))
        label = ce.CLASSES[ci][1]
        ry, rx = float(np.exp(rng.uniform(np.log(8), np.log(120)))), float(np.exp(rng.uniform(np.log(8), np.log(160))))
        cy, cx = float(rng.uniform(420, 930)), float(rng.uniform(30, W - 30))
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        if k % 14 == 13:
            g[inside] = label                                          # a group region
        else:
            serial[label] = serial.get(label, 0) + 1
            g[inside] = label * 1000 + serial[label]
            ellipses.append((cy, cx, ry, rx, ci))
    return g, ellipses


def predictions(n, ellipses, rng, dev):
    """n elliptic blobs on the device: every second one a jittered copy of a ground-truth ellipse."""
    yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    masks = torch.empty((n, H, W), dtype=torch.bool, device=dev)
    classes = []
    for k in range(n):
        if k % 2 == 0:
            cy, cx, ry, rx, ci = ellipses[(k // 2) % len(ellipses)]
            cy, cx, ry, rx = cy + rng.uniform(-0.15, 0.15) * ry, cx + rng.uniform(-0.15, 0.15) * rx, ry * rng.uniform(0.85, 1.15), rx * rng.uniform(0.85, 1.15)
        else:
            ci = int(rng.randint(0, len(ce.CLASSES)))
            ry, rx = float(np.exp(rng.uniform(np.log(8), np.log(120)))), float(np.exp(rng.uniform(np.log(8), np.log(160))))
            cy, cx = float(rng.uniform(300, 1000)), float(rng.uniform(0, W))
        masks[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        classes.append(ci)
    return Instances((H, W), pred_masks=masks, pred_classes=torch.tensor(classes, device=dev),
                     scores=torch.from_numpy(rng.rand(n).astype(np.float32)).to(dev), mask_scores=torch.from_numpy(rng.rand(n).astype(np.float32)).to(dev))


def write_png16(path, img, ft):
    """(H,W) uint16 -> a 16-bit greyscale PNG whose rows all use filter type ft (2 Up or 4 Paeth)."""
    rows = img.astype(">u2").view(np.uint8).reshape(img.shape[0], -1).astype(np.int64)
    up = np.concatenate([np.zeros_like(rows[:1]), rows[:-1]])
    if ft == 2:
        pred = up
    else:
        a = np.concatenate([np.zeros_like(rows[:, :2]), rows[:, :-2]], axis=1)
        c = np.concatenate([np.zeros_like(up[:, :2]), up[:, :-2]], axis=1)
        p = a + up - c
        pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    body = np.concatenate([np.full((rows.shape[0], 1), ft, dtype=np.uint8), ((rows - pred) & 255).astype(np.uint8)], axis=1).tobytes()
    chunk = lambda k, b: struct.pack(">I", len(b)) + k + b + struct.pack(">I", zlib.crc32(k + b) & 0xffffffff)  # noqa: E731
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", img.shape[1], img.shape[0], 16, 0, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(body, 6)) + chunk(b"IEND", b""))


def _spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "rounds": len(ms)}


def _process(ev, inst):
    ev.reset()
    t0 = time.perf_counter()
    ev.process([{"file_name": NAME + "_leftImg8bit.png"}], [{"instances": inst}])
    return (time.perf_counter() - t0) * 1e3


def floor_us(n):
    return (n * H * W / 8 + 2 * H * W) / HBM_BYTES_PER_S * 1e6


def kernel_stats(path):
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}
    name = [k for k in rows if "label_counts_kernel" in k]
    if not name or int(rows[name[0]]["Calls"]) != TRACE_CALLS:
        raise SystemExit("{}: not the {} label_counts_kernel launches of a --trace-body run".format(path, TRACE_CALLS))
    us = float(rows[name[0]]["TotalDurationNs"]) / 1e3 / TRACE_CALLS
    return {"source": "rocprofv3 --kernel-trace --stats, {} calls of ops.mask_label_counts on {} predictions".format(TRACE_CALLS, TRACE_N),
            "label_counts_kernel_us": round(us, 2), "read_once_floor_us": round(floor_us(TRACE_N), 2),
            "read_once_floor": "N*H*W/8 + 2*H*W bytes at 6.3 TB/s", "floor_over_kernel": round(floor_us(TRACE_N) / us, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-body", action="store_true", help="only run the device table a few times (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --trace-body run; merged into --out")
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        res["kernel"] = kernel_stats(a.kernel_stats)
        print(json.dumps(res["kernel"]))
        if a.out:
            json.dump(res, open(a.out, "w"), indent=1)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_cityscapes_eval needs the MI355X: nothing about speed is stated from a CPU run")
    if a.rounds < 10 and not a.trace_body:
        raise SystemExit("at least 10 rounds of each path")
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(11)
    gt, ellipses = label_image(rng)
    cols, regions = ce.columns(gt)
    num_cols = 2 + len(regions)

    if a.trace_body:
        inst = predictions(TRACE_N, ellipses, rng, dev)
        for _ in range(TRACE_CALLS):
            ops.mask_label_counts(inst.pred_masks, cols, num_cols)
        torch.cuda.synchronize()
        return

    t_cols = []
    for _ in range(5):
        t0 = time.perf_counter()
        ce.columns(gt)
        t_cols.append((time.perf_counter() - t0) * 1e3)
    loader = {}
    with tempfile.TemporaryDirectory() as tmp:
        for ft, what in ((2, "up_filter_numpy"), (4, "paeth_filter_python_loop")):
            path = os.path.join(tmp, "{}_gtFine_instanceIds.png".format(what))
            write_png16(path, gt, ft)
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                back = ce.read_label_png(path)
                ms.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(back, gt), "read_label_png does not give the label image back"
            loader[what] = dict(_spread(ms), file_bytes=os.path.getsize(path))

    ev = CityscapesInstanceEvaluator(ground_truth={NAME: gt})
    res = {"workload": "{}x{} label image with {} ground-truth regions ({} columns); {} elliptic blob predictions, every second one a jittered "
                       "ground-truth ellipse; mask generation not timed".format(H, W, len(regions), num_cols, " and ".join(map(str, COUNTS))),
           "columns_ms_per_image": _spread(t_cols), "columns_note": "cityscapes_eval.columns on the host, part of both paths' process()",
           "read_label_png_ms_per_image": loader, "per_count": {}}
    for n in COUNTS:
        gpu = predictions(n, ellipses, rng, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cpu = gpu.to("cpu")
        download_ms = (time.perf_counter() - t0) * 1e3
        # equality first; this is also the warm-up of both paths
        tg, ag = ops.mask_label_counts(gpu.pred_masks, cols, num_cols)
        th, ah = ce.label_counts_host(cpu.pred_masks.numpy(), cols, num_cols)
        assert np.array_equal(tg.numpy(), th) and np.array_equal(ag.numpy(), ah), "tables of the two paths differ"
        _process(ev, gpu)
        on_gpu = ev._predictions
        _process(ev, cpu)
        assert on_gpu == ev._predictions, "records of the two paths differ"
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(_process(ev, cpu))
            tb.append(_process(ev, gpu))
        # the entry alone: zeroing of the table and the kernel, between two device events
        words, _ = ops.mask_pack_bits(gpu.pred_masks)
        cols_dev = torch.from_numpy(cols.view(np.int16)).to(dev)
        table = torch.empty((n, num_cols), dtype=torch.int32, device=dev)
        from centermask2_amd import _lib
        lib, us = _lib.load(), []
        for k in range(5 + max(a.rounds, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.cmk_mask_label_counts(words.data_ptr(), n, cols_dev.data_ptr(), H, W, num_cols, table.data_ptr(), ops._stream()))
            e1.record()
            e1.synchronize()
            if k >= 5:
                us.append(e0.elapsed_time(e1) * 1e3)
        assert np.array_equal(table.cpu().numpy(), th)
        covered = float(ah.sum()) / (n * H * W)
        res["per_count"][str(n)] = {
            "tables_equal": True,
            "mask_pixels_share": round(covered, 5),
            "host_ms_per_image": _spread(ta),
            "device_ms_per_image": _spread(tb),
            "host_over_device_median": round(statistics.median(ta) / statistics.median(tb), 2),
            "device_faster_beyond_spread": max(tb) < min(ta),
            "instances_to_cpu_ms": round(download_ms, 3),
            "d2h_bytes_per_image": {"host": n * H * W, "device_table": 4 * (n * num_cols + n)},
            "entry_us": {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2), "calls": len(us),
                         "what": "cmk_mask_label_counts between two device events: zeroing of the table, label_counts_kernel"},
            "read_once_floor_us": round(floor_us(n), 2),
        }
    res["read_once_floor"] = "N*H*W/8 + 2*H*W bytes at 6.3 TB/s"
    res["instances_to_cpu_note"] = "one measurement of Instances.to('cpu') per count; not part of host_ms_per_image"
    res["timing"] = "host clock around each process() call, A and B alternating, {} rounds after a warm-up of both".format(a.rounds)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        if "kernel" in old:
            res["kernel"] = old["kernel"]
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
