"""Sliced inference at a Cityscapes frame: one raw 1024 x 2048 image, TEST.SLICE with tiles of 512 x 512, overlap 0.2 (15 tiles) and the
full-image pass, on V-39 with synthetic weights and the recipe's test size (every tile runs at 800 x 800).  A tool only: bench.py does
not run it.

Two schedules on the same code, same kernels (the untuned conv defaults), timed in one session, alternating, each with device events
around whole steps after a warm-up of every shape:
  sliced     the Predictor with TEST.SLICE.ENABLED: tiles in batches of TEST.SLICE.BATCH, merged on the device
  separate   the same tiles and the whole image as separate plain Predictor calls, the boxes read back, shifted and merged on the host
             by a NumPy greedy NMS on the same metric, the survivors' bitmasks placed into the frame: what a user without TEST.SLICE
             would have to run
Reported per schedule: the median over the rounds with the smallest and the largest round.  Then the pieces the sliced step adds, each
in a window of its own and as a share of the median step: the crop copies (T slices made contiguous), the map kernel, the metric NMS,
and the gather of the survivors' masks and mask scores.  The wrappers' allocations are inside those times.

    python tools/bench_slice.py [--out profiles/bench_slice.json] [--rounds 5]

The AP gain on small objects is not measured here: there is no dataset and no trained checkpoint where this runs.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from centermask2_amd import Predictor, ops, synthetic as S  # noqa: E402
from centermask2_amd.config import config_path, get_cfg  # noqa: E402
from centermask2_amd.modeling import build_model  # noqa: E402

H, W = 1024, 2048
WINDOW_S = 0.5


def raw_image(seed):
    x = S.make_synthetic_images(1, H, W, seed0=seed)[0] + torch.tensor(S.PIXEL_MEAN).view(3, 1, 1)
    return x.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def step_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def timed(fn):
    """ms per call of a short piece: warm up, size the window to at least WINDOW_S, time it."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = 16
    while True:
        ms = step_ms(fn, reps) * reps
        if ms >= WINDOW_S * 1e3:
            return ms / reps
        reps = max(reps * 2, int(reps * WINDOW_S * 1.2e3 / max(ms, 1e-3)))


def host_merge(box, score, cls, thr, topk, ios):
    """Greedy class-wise NMS in NumPy on IoS (or IoU): the indices of the first topk survivors in descending-score order."""
    order = np.argsort(-score, kind="stable")
    box, cls = box[order].astype(np.float64), cls[order]
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    alive = np.ones(len(order), dtype=bool)
    keep = []
    for i in range(len(order)):
        if not alive[i]:
            continue
        keep.append(int(order[i]))
        if len(keep) == topk:
            break
        iw = np.clip(np.minimum(box[i, 2], box[i + 1:, 2]) - np.maximum(box[i, 0], box[i + 1:, 0]), 0, None)
        ih = np.clip(np.minimum(box[i, 3], box[i + 1:, 3]) - np.maximum(box[i, 1], box[i + 1:, 1]), 0, None)
        inter = iw * ih
        den = np.minimum(area[i], area[i + 1:]) if ios else area[i] + area[i + 1:] - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            alive[i + 1:] &= ~((inter / den > thr) & (cls[i + 1:] == cls[i]))
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of the two schedules")
    ap.add_argument("--steps", type=int, default=2, help="steps per schedule and round")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_slice needs the MI355X: nothing about speed is stated from a CPU run")
    dev = torch.device("cuda:0")
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda:0", "TEST.SLICE.ENABLED", True, "TEST.SLICE.TILE", (512, 512), "TEST.SLICE.OVERLAP", 0.2,
                         "TEST.SLICE.FULL_IMAGE", True])
    cfg.freeze()
    model = build_model(cfg).eval()
    model.load_state_dict(S.make_synthetic_state_dict("V-39-eSE", 0))
    raw = raw_image(4321).to(dev)
    pred = Predictor(cfg, model=model)
    sliced = pred.sliced
    single = Predictor(cfg, model=model)
    single.sliced = None                                      # the plain path of the same Predictor
    passes = sliced.passes(H, W)
    tiles = passes[:-1]
    ios = sliced.metric == "ios"

    def crop_all():
        return [raw[y0:y0 + th, x0:x0 + tw].contiguous() for y0, x0, th, tw, _, _ in tiles]

    def separate():
        results = [single(c)["instances"] for c in crop_all()] + [single(raw)["instances"]]
        offs = [(x0, y0) for y0, x0, _, _, _, _ in passes]
        box = np.concatenate([r.pred_boxes.tensor.cpu().numpy() + np.array([x0, y0, x0, y0], np.float32) for r, (x0, y0) in zip(results, offs)])
        score = np.concatenate([r.scores.cpu().numpy() for r in results])
        cls = np.concatenate([r.pred_classes.cpu().numpy() for r in results])
        keep = host_merge(box, score, cls, sliced.match_thresh, sliced.topk, ios)
        ends = np.cumsum([len(r) for r in results])
        masks = torch.zeros((len(keep), H, W), dtype=torch.bool, device=dev)
        for j, i in enumerate(keep):                          # the survivor's bitmask, placed at its pass's corner
            p = int(np.searchsorted(ends, i, side="right"))
            y0, x0, th, tw, _, _ = passes[p]
            masks[j, y0:y0 + th, x0:x0 + tw] = results[p].pred_masks[i - (ends[p - 1] if p else 0)]
        return len(keep), masks

    schedules = {"sliced": lambda: pred(raw), "separate": separate}
    got = pred(raw)["instances"]
    n_sep, _ = separate()
    for fn in schedules.values():                             # every shape of every schedule once more before a clock starts
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in schedules}
    for _ in range(a.rounds):
        for k, fn in schedules.items():
            rounds[k].append(round(step_ms(fn, a.steps), 3))
    ms = {k: {"median": round(statistics.median(v), 3), "min": min(v), "max": max(v)} for k, v in rounds.items()}
    step = ms["sliced"]["median"]
    res = {"shape": "one raw {}x{} image, V-39-eSE, synthetic weights, {} tiles of {}x{} at overlap {} resized to {}x{}, batch {}, and the whole "
                    "image at {}x{}".format(H, W, len(tiles), tiles[0][2], tiles[0][3], sliced.overlap, tiles[0][4], tiles[0][5], sliced.batch,
                                            passes[-1][4], passes[-1][5]),
           "timing": "device events around {} whole steps, {} alternating rounds after a warm-up of every shape; median, smallest and largest "
                     "round".format(a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "metric": sliced.metric, "match_thresh": sliced.match_thresh,
           "detections": {"sliced": len(got), "separate": n_sep}, "ms_per_image": ms, "ms_rounds": rounds,
           "sliced_over_separate": round(step / ms["separate"]["median"], 4),
           "ap_gain": "not measured (no dataset, no trained checkpoint)"}

    # ---- the pieces the sliced step adds, at the shapes of this step -------------------------------------------------------------
    na, k, topk, s = len(passes), int(cfg.MODEL.FCOS.POST_NMS_TOPK_TEST), sliced.topk, 28
    g = torch.Generator().manual_seed(3)
    lo = torch.rand((na, k, 2), generator=g) * 600
    det = dict(box=torch.cat([lo, lo + torch.rand((na, k, 2), generator=g) * 200], dim=2).to(dev), score=torch.rand((na, k), generator=g).to(dev),
               cls=torch.randint(0, 80, (na, k), generator=g).to(dev), loc=(lo + 50).to(dev),
               counts=torch.full((na,), k, dtype=torch.int32, device=dev))
    table = sliced._geometry(H, W, dev)[1]
    cand = ops.slice_boxes_to_image(det, table, H, W)
    merged = ops.nms_topk(cand, sliced.match_thresh, topk, metric=sliced.metric)
    n = int(merged["counts"][0])
    masks, scores = torch.rand((na * k, 1, s, s), generator=g).to(dev), torch.rand((na * k,), generator=g).to(dev)

    def gather():
        src = cand["src"].index_select(0, merged["idx"][0, :n].long()).long()
        return masks.index_select(0, src), scores.index_select(0, src)

    pieces = {"crop_copies": {"ms": timed(crop_all), "what": "{} slices of {}x{}x3 bytes made contiguous".format(len(tiles), tiles[0][2], tiles[0][3])},
              "slice_boxes_to_image": {"ms": timed(lambda: ops.slice_boxes_to_image(det, table, H, W)), "what": "A {} x K {} rows, all valid".format(na, k)},
              "nms_topk_metric": {"ms": timed(lambda: ops.nms_topk(cand, sliced.match_thresh, topk, metric=sliced.metric)),
                                  "what": "{} random candidates, {} kept of top {}".format(na * k, n, topk)},
              "gather": {"ms": timed(gather), "what": "{} survivors' {}x{} masks and mask scores by index_select".format(n, s, s)}}
    for v in pieces.values():
        v["ms"] = round(v["ms"], 4)
        v["share_of_step"] = round(v["ms"] / step, 5)
    res["pieces"] = pieces
    res["pieces_share_of_step"] = round(sum(v["ms"] for v in pieces.values()) / step, 5)
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
