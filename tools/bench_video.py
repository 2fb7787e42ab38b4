"""Video mode at the sizes a user runs: what a frame's association costs beside the picture.  A tool only: bench.py does not run it.

Per size (480 x 640 and 800 x 1333) and instance count (50 and 100): a clip of 4 frames of the same objects, pasted blob masks as
tools/bench_visualize.py makes them, every frame with its own jitter and its own output order, cycled.  Timed with device events after a
warm-up, each over a window of at least half a second, ms per frame:
  update_box          InstanceTracker(match="box").update: IoU table, assign (3 launches at most)
  update_mask         InstanceTracker(match="mask").update on packed words: intersections, assign, gather
  update_mask_pack    the same with ops.mask_pack_bits of the frame's bitmasks in front (what a caller without packed words pays)
  draw                Visualizer.draw
  draw_video_box      VideoVisualizer(match="box").draw on the same instances
  draw_video_mask     VideoVisualizer(match="mask").draw (the masks are packed once for tracker and picture)
The gather's bytes (rows read and written once, stated in `gather_bytes`) are given with the time they take at the HBM bandwidth an
MI355X achieves; beside it the box update is three small launches, the mask update the all-pairs table of cmk_mask_intersections over
the host's bound on the table's rows (DESIGN §3 "Video" has the per-kernel figures).

    python tools/bench_video.py [--out profiles/bench_video.json]

Per-kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -- python tools/bench_video.py --trace-body
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
from centermask2_amd.structures import Boxes, Instances  # noqa: E402
from centermask2_amd.video import InstanceTracker, VideoVisualizer  # noqa: E402
from centermask2_amd.visualize import COCO_CLASSES, Visualizer  # noqa: E402

SIZES = ((480, 640), (800, 1333))
COUNTS = (50, 100)
CLIP, S = 4, 28
HBM_BYTES_PER_S = 6.29e12           # achieved HBM bandwidth of an MI355X (float4 copy); the spec peak is 8.0e12
WINDOW_S = 0.5


def clip(n, h, w, dev):
    """CLIP frames of the same n objects: boxes jittered by up to 2 % of their size, the output order shuffled."""
    g = torch.Generator().manual_seed(17)
    bw = torch.empty(n).uniform_(math.log(20.0), math.log(float(w)), generator=g).exp()
    bh = torch.empty(n).uniform_(math.log(20.0), math.log(float(h)), generator=g).exp()
    x0, y0 = torch.rand(n, generator=g) * (w - bw), torch.rand(n, generator=g) * (h - bh)
    u = torch.linspace(-1, 1, S)
    vv, uu = torch.meshgrid(u, u, indexing="ij")
    r = lambda lo, hi: (torch.rand(n, 1, 1, generator=g) * (hi - lo) + lo)  # noqa: E731
    cx, cy, sx, sy = r(-0.3, 0.3), r(-0.3, 0.3), r(0.4, 0.9), r(0.4, 0.9)
    soft = torch.exp(-(((uu - cx) / sx) ** 2 + ((vv - cy) / sy) ** 2)).clamp(0, 1).float()
    classes, scores = torch.randint(0, 80, (n,), generator=g), torch.rand(n, generator=g)
    image = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    frames = []
    for _ in range(CLIP):
        perm = torch.randperm(n, generator=g)
        jit = (torch.rand(n, 4, generator=g) - 0.5) * 0.04 * torch.stack([bw, bh, bw, bh], 1)
        boxes = (torch.stack([x0, y0, x0 + bw, y0 + bh], 1) + jit)[perm]
        masks = ops.paste_masks(soft[perm].to(dev), boxes.to(dev), h, w).bool()
        frames.append(Instances((h, w), pred_boxes=Boxes(boxes.to(dev)), scores=scores[perm].to(dev), pred_classes=classes[perm].to(dev),
                                pred_masks=masks))
    return image, frames


def timed(fn):
    """ms per call by device events: warm up (two rounds of the clip), size the window to at least WINDOW_S, time it."""
    for _ in range(2 * CLIP):
        fn()
    torch.cuda.synchronize()
    reps, a, b = 4 * CLIP, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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


def cycle(frames, fn):
    state = {"k": 0}

    def step():
        fn(state["k"] % len(frames))
        state["k"] += 1
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-body", action="store_true", help="only a few frames of each stage at the largest size (for rocprofv3 --kernel-trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_video needs the MI355X: nothing about speed is stated from a CPU run")
    dev = torch.device("cuda:0")
    res = {"clip": "{} frames of the same objects, jittered and reordered, pasted blob masks".format(CLIP),
           "timing": "ms per frame, device events after a warm-up, windows of at least {} s".format(WINDOW_S),
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "device": torch.cuda.get_device_name(0), "runs": {}}
    for h, w in (SIZES[-1:] if a.trace_body else SIZES):
        for n in (COUNTS[-1:] if a.trace_body else COUNTS):
            image, frames = clip(n, h, w, dev)
            packed = [ops.mask_pack_bits(f.pred_masks) for f in frames]
            box, mask, mask_pack = InstanceTracker(match="box"), InstanceTracker(match="mask"), InstanceTracker(match="mask")
            kw = {"class_names": COCO_CLASSES}
            plain, vbox, vmask = Visualizer(**kw), VideoVisualizer(match="box", **kw), VideoVisualizer(match="mask", **kw)
            # is the clip what it says: after two rounds n ids are out and n tracks live if every instance of every frame was matched
            tracked = {}
            for tr, args in ((box, lambda k: (frames[k],)), (mask, lambda k: (frames[k],) + packed[k])):
                for k in range(2 * CLIP):
                    tr.update(*args(k % CLIP))
                tracked[tr.match] = {"ids_given": tr.next_id, "tracks": tr.n_tracks, "dropped": tr.dropped}
            stages = {"update_box": lambda k: box.update(frames[k]),
                      "update_mask": lambda k: mask.update(frames[k], *packed[k]),
                      "update_mask_pack": lambda k: mask_pack.update(frames[k]),
                      "draw": lambda k: plain.draw(image, frames[k]),
                      "draw_video_box": lambda k: vbox.draw(image, frames[k]),
                      "draw_video_mask": lambda k: vmask.draw(image, frames[k])}
            if a.trace_body:
                for fn in stages.values():
                    for k in range(2 * CLIP):
                        fn(k % CLIP)
                torch.cuda.synchronize()
                continue
            run = {"ms": {}, "calls": {}, "after_two_rounds": tracked}
            for name, fn in stages.items():
                ms, reps = timed(cycle(frames, fn))
                run["ms"][name], run["calls"][name] = round(ms, 4), reps
            gather = 2 * n * ops.mask_words(h, w) * 8
            run["gather_bytes"] = {"bytes": gather, "stated": "n rows of ceil(h*w/64) words read once and written once",
                                   "memory_bound_ms": round(gather / HBM_BYTES_PER_S * 1e3, 4)}
            run["update_over_draw"] = {"box": round(run["ms"]["update_box"] / run["ms"]["draw"], 3),
                                       "mask": round(run["ms"]["update_mask"] / run["ms"]["draw"], 3)}
            run["video_draw_over_draw"] = {"box": round(run["ms"]["draw_video_box"] / run["ms"]["draw"], 3),
                                           "mask": round(run["ms"]["draw_video_mask"] / run["ms"]["draw"], 3)}
            res["runs"]["{}x{}_{}".format(h, w, n)] = run
            del frames, packed, box, mask, mask_pack, vbox, vmask
            torch.cuda.empty_cache()
    if a.trace_body:
        return
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
