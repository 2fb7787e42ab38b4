"""The device-side visualizer at the bench shape: one 800 x 1280 image with 50 and with 100 instances whose masks are pasted blobs (as
tools/bench_rle.py makes them), 17 keypoints each with the COCO skeleton.  A tool only: bench.py does not run it.

Timed with device events after a warm-up, each over a window of at least half a second:
  draw      Visualizer.draw as a whole (sort, prepare, pack, compose, keypoints; the allocations included)
  pack      ops.mask_pack_bits           (n,H,W) byte masks -> 64-bit words
  prepare   ops.vis_prepare              per-instance records
  compose   ops.vis_compose              the hot kernel: boxes, fills, outlines, labels
  keypoints ops.vis_keypoints            winner map + colour pass

The bytes model, stated in `bytes_model` below: the image is read once and written once and the packed words are read once
(compose); the pack reads the byte masks once and writes the words.  compose and the whole draw are reported as a share of the time these
bytes take at the HBM bandwidth an MI355X achieves (6.29 TB/s measured of 8.0 TB/s peak); the bound is memory, there is no arithmetic to
speak of.  The host comparison is the download of the same Instances plus the tests' NumPy restatement (tests/visualize_ref.py) on them:
the tests' restatement, not detectron2's matplotlib renderer, which is not available here.  The two pictures are asserted equal first.

    python tools/bench_visualize.py [--out profiles/bench_visualize.json]

Per-kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -- python tools/bench_visualize.py --trace-body
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from centermask2_amd import ops  # noqa: E402
from centermask2_amd.structures import Boxes, Instances  # noqa: E402
from centermask2_amd.visualize import COCO_CLASSES, COCO_PERSON_SKELETON, Visualizer  # noqa: E402

H, W, S, K = 800, 1280, 28, 17
HBM_BYTES_PER_S = 6.29e12           # achieved HBM bandwidth of an MI355X (float4 copy); the spec peak is 8.0e12
WINDOW_S = 0.5


def bytes_model(n, with_pack):
    """Least bytes a draw moves: image in + image out + the packed words once (+ the byte masks and the words' write for the pack)."""
    words = n * ops.mask_words(H, W) * 8
    compose = 2 * 3 * H * W + words
    return compose + (n * H * W + words if with_pack else 0)


def workload(n, dev):
    g = torch.Generator().manual_seed(11)
    bw = torch.empty(n).uniform_(math.log(20.0), math.log(float(W)), generator=g).exp()
    bh = torch.empty(n).uniform_(math.log(20.0), math.log(float(H)), generator=g).exp()
    x0, y0 = torch.rand(n, generator=g) * (W - bw), torch.rand(n, generator=g) * (H - bh)
    boxes = torch.stack([x0, y0, x0 + bw, y0 + bh], 1)
    u = torch.linspace(-1, 1, S)
    vv, uu = torch.meshgrid(u, u, indexing="ij")
    r = lambda lo, hi: (torch.rand(n, 1, 1, generator=g) * (hi - lo) + lo)  # noqa: E731
    cx, cy, sx, sy = r(-0.3, 0.3), r(-0.3, 0.3), r(0.4, 0.9), r(0.4, 0.9)
    soft = torch.exp(-(((uu - cx) / sx) ** 2 + ((vv - cy) / sy) ** 2)).clamp(0, 1).float()
    masks = ops.paste_masks(soft.to(dev), boxes.to(dev), H, W).bool()
    kp = torch.rand(n, K, 3, generator=g)
    kp[:, :, 0] = x0[:, None] + kp[:, :, 0] * bw[:, None]
    kp[:, :, 1] = y0[:, None] + kp[:, :, 1] * bh[:, None]
    image = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    inst = Instances((H, W), pred_boxes=Boxes(boxes.to(dev)), scores=torch.rand(n, generator=g).to(dev),
                     pred_classes=torch.randint(0, 80, (n,), generator=g).to(dev), pred_masks=masks, pred_keypoints=kp.to(dev))
    return image.to(dev), inst


def timed(fn):
    """ms per call by device events: warm up, size the window to at least WINDOW_S, time it."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps, a, b = 4, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= WINDOW_S * 1e3:
            return ms / reps, reps
        reps = max(reps * 2, int(reps * WINDOW_S * 1.2e3 / max(ms, 1e-3)))


def host_path(image, inst, kw):
    from tests import visualize_ref as R
    t0 = time.perf_counter()
    host = inst.to("cpu")
    img = image.cpu()
    t1 = time.perf_counter()
    out = R.render_instances(img, host, skeleton=COCO_PERSON_SKELETON, **kw)
    t2 = time.perf_counter()
    return out, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-body", action="store_true", help="only a few draws of each size (for rocprofv3 --kernel-trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visualize needs the MI355X: nothing about speed is stated from a CPU run")
    dev = torch.device("cuda:0")
    kw = {"class_names": COCO_CLASSES}
    vis = Visualizer(**kw)
    res = {"shape": "{}x{} image, pasted blob masks, {} keypoints with the COCO skeleton".format(H, W, K),
           "timing": "device events after a warm-up, windows of at least {} s".format(WINDOW_S),
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "device": torch.cuda.get_device_name(0), "runs": {}}
    for n in (50, 100):
        image, inst = workload(n, dev)
        if a.trace_body:
            for _ in range(5):
                vis.draw(image, inst)
            torch.cuda.synchronize()
            continue
        got = vis.draw(image, inst)
        want, dl_ms, render_ms = host_path(image, inst, kw)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), "device picture and restatement differ"
        lw, fs = vis.line_width or 2, vis.font_scale or 2            # the defaults at 800 x 1280: round(800/400), round(800/500)
        t = vis._device_tables(dev)
        boxes, scores, classes = inst.pred_boxes.tensor, inst.scores, inst.pred_classes
        area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        order = torch.sort(area, descending=True, stable=True).indices
        prep = lambda: ops.vis_prepare(boxes, scores, classes, order, t["names"], t["name_lens"], t["num_names"], t["palette"], H, W, fs, False)  # noqa: E731
        records = prep()
        words, _ = ops.mask_pack_bits(inst.pred_masks)
        skel, _ = vis._device_skeleton(t, K, dev)
        composed = ops.vis_compose(image, words, records, n, t["font"], lw, fs, vis.alpha256)
        kps = inst.pred_keypoints.contiguous()
        stages = {"draw": lambda: vis.draw(image, inst), "pack": lambda: ops.mask_pack_bits(inst.pred_masks), "prepare": prep,
                  "compose": lambda: ops.vis_compose(image, words, records, n, t["font"], lw, fs, vis.alpha256),
                  "keypoints": lambda: ops.vis_keypoints(composed, kps, records, skel, vis.keypoint_threshold, lw, 255 << 16)}
        run = {"ms": {}, "calls": {}}
        for name, fn in stages.items():
            run["ms"][name], run["calls"][name] = timed(fn)
            run["ms"][name] = round(run["ms"][name], 4)
        b_compose, b_draw = bytes_model(n, False), bytes_model(n, True)
        run["bytes_model"] = {"compose": b_compose, "draw": b_draw, "stated": "image in + image out + packed words once (+ byte masks and words for the pack)"}
        run["memory_bound_ms"] = {"compose": round(b_compose / HBM_BYTES_PER_S * 1e3, 4), "draw": round(b_draw / HBM_BYTES_PER_S * 1e3, 4)}
        run["share_of_memory_bound"] = {k: round(run["memory_bound_ms"][k] / run["ms"][k], 4) for k in ("compose", "draw")}
        run["host"] = {"what": "download of the Instances + the tests' NumPy restatement (not detectron2)", "download_ms": round(dl_ms, 2),
                       "restatement_ms": round(render_ms, 2), "download_bytes": n * H * W, "pictures_equal": True}
        run["host_over_device"] = round((dl_ms + render_ms) / run["ms"]["draw"], 1)
        res["runs"][str(n)] = run
    if a.trace_body:
        return
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
