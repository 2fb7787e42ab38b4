"""Test-time augmentation at the bench shape: one raw 800 x 1280 image, detectron2's default TEST.AUG (nine scales 400..1200, MAX_SIZE
4000, FLIP: 18 augmentations) on V-39 with synthetic weights.  A tool only: bench.py does not run it.

Three schedules on the same code, same kernels (the untuned conv defaults), timed in one session, alternating, each with device events
around whole steps after a warm-up of every shape:
  tta        GeneralizedRCNNWithTTA: one backbone pass per scale batch of two, its feature maps kept for the mask pass
  d2         the same step with detectron2's schedule: the backbone run again per scale batch for the mask pass
  separate   len(augs) single-scale Predictor calls (one per augmentation, the mirrored ones on the mirrored image): what a user
             without TEST.AUG would have to run, and still without the merge
Then the three new kernels at the shapes of that step, each in a window of its own: time, the least bytes it must move (stated in
`bytes_model`), that over the achieved HBM bandwidth of an MI355X as its memory bound, and their sum as a share of the step.  The box
maps move a few kilobytes: their time is a launch, not bandwidth, and is reported as such.

    python tools/bench_tta.py [--out profiles/bench_tta.json] [--rounds 3]

The AP gain of TTA is not measured here: there is no COCO and no trained checkpoint where this runs.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from centermask2_amd import GeneralizedRCNNWithTTA, Predictor, _lib, ops, synthetic as S  # noqa: E402
from centermask2_amd.config import config_path, get_cfg  # noqa: E402
from centermask2_amd.modeling import build_model  # noqa: E402

H, W = 800, 1280
HBM_BYTES_PER_S = 6.29e12           # achieved HBM bandwidth of an MI355X (float4 copy); the spec peak is 8.0e12
WINDOW_S = 0.5


class D2Schedule(GeneralizedRCNNWithTTA):
    """detectron2's schedule: the mask pass computes the features of every augmentation again."""

    def _mask_features(self, i, canvases, feats):
        return self.model.backbone(canvases[i])


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
    """ms per call of a short launch: warm up, size the window to at least WINDOW_S, time it."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = 16
    while True:
        ms = step_ms(fn, reps) * reps
        if ms >= WINDOW_S * 1e3:
            return ms / reps
        reps = max(reps * 2, int(reps * WINDOW_S * 1.2e3 / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of the three schedules")
    ap.add_argument("--steps", type=int, default=2, help="steps per schedule and round")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta needs the MI355X: nothing about speed is stated from a CPU run")
    dev = torch.device("cuda:0")
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda:0", "TEST.AUG.ENABLED", True])
    cfg.freeze()
    model = build_model(cfg).eval()
    model.load_state_dict(S.make_synthetic_state_dict("V-39-eSE", 0))
    raw = raw_image(4321).to(dev)
    mirrored = torch.flip(raw, dims=[1]).contiguous()
    tta, d2 = GeneralizedRCNNWithTTA(cfg, model), D2Schedule(cfg, model)
    single = Predictor(cfg, model=model)
    single.tta = None                                         # the single-scale path of the same Predictor
    augs = tta._geometry(H, W, dev)[0]

    def separate():
        for (nh, nw, flip), s in zip(augs, [s for s in tta.min_sizes for _ in range(2 if tta.flip else 1)]):
            single.min_size, single.max_size = s, tta.max_size
            single(mirrored if flip else raw)

    schedules = {"tta": lambda: tta.inference_one_image(raw, H, W), "d2": lambda: d2.inference_one_image(raw, H, W), "separate": separate}
    got, again = tta.inference_one_image(raw, H, W), d2.inference_one_image(raw, H, W)
    torch.cuda.synchronize()
    assert len(got) == len(again) and torch.equal(got.scores, again.scores) and torch.equal(got.pred_masks, again.pred_masks)
    for fn in schedules.values():                             # every shape of every schedule once more before a clock starts
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in schedules}
    for _ in range(a.rounds):
        for k, fn in schedules.items():
            rounds[k].append(round(step_ms(fn, a.steps), 3))
    ms = {k: min(v) for k, v in rounds.items()}
    res = {"shape": "one raw {}x{} image, V-39-eSE, synthetic weights, {} augmentations {}".format(H, W, len(augs), [(nh, nw) for nh, nw, _ in augs[::2]]),
           "timing": "device events around {} whole steps, {} alternating rounds after a warm-up of every shape; ms is the best round".format(a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "detections": len(got), "ms_per_image": ms, "ms_rounds": rounds,
           "tta_over_d2": round(ms["tta"] / ms["d2"], 4), "tta_over_separate": round(ms["tta"] / ms["separate"], 4),
           "ap_gain": "not measured (no COCO, no trained checkpoint)", "hbm_bytes_per_s": HBM_BYTES_PER_S}

    # ---- the new kernels at the shapes of this step -----------------------------------------------------------------------------
    lib = _lib.load()
    d = model.backbone.size_divisibility
    m3 = (ctypes.c_float * 3)(*model.pixel_mean.flatten().tolist())
    s3 = (ctypes.c_float * 3)(*model.pixel_std.flatten().tolist())
    kern = {"hflip": {"ms": 0.0, "bytes": 0, "per_scale_ms": {}}}
    for nh, nw, _ in augs[::2]:
        hp, wp = (nh + d - 1) // d * d, (nw + d - 1) // d * d
        ws = torch.empty((H * nw * 3 + 3,), dtype=torch.uint8, device=dev)
        mid = ops._resize_h(lib, raw, nw, ws)
        by, ky, ksy, keep = ops._resize_v_args(H, nh, dev)
        dst = torch.empty((3, hp, wp), dtype=torch.float32, device=dev)
        t = timed(lambda: ops.check(lib.cmk_resize_v_preprocess_hflip(mid.data_ptr(), H, nh, nw, by, ky, ksy, dst.data_ptr(), hp, wp, m3, s3, 0,
                                                                      ops._stream()), "hflip"))
        kern["hflip"]["per_scale_ms"]["{}x{}".format(nh, nw)] = round(t, 4)
        kern["hflip"]["ms"] += t
        kern["hflip"]["bytes"] += 12 * hp * wp + 3 * H * nw       # the float canvas written once, the h-pass output read once
        del keep
    k, topk, s, na = int(cfg.MODEL.FCOS.POST_NMS_TOPK_TEST), tta.topk, 28, len(augs)
    g = torch.Generator().manual_seed(3)
    det = dict(box=(torch.rand((na, k, 4), generator=g) * 400).to(dev), score=torch.rand((na, k), generator=g).to(dev),
               cls=torch.randint(0, 80, (na, k), generator=g).to(dev), loc=(torch.rand((na, k, 2), generator=g) * 400).to(dev),
               counts=torch.full((na,), k, dtype=torch.int32, device=dev))
    _, to_image, to_aug, flips = tta._geometry(H, W, dev)
    count = torch.tensor([len(got)], dtype=torch.int32, device=dev)
    box = (torch.rand((topk, 4), generator=g) * 400).to(dev)
    masks, scores = torch.rand((na, topk, s, s), generator=g).to(dev), torch.rand((na, topk), generator=g).to(dev)
    kern["boxes_to_image"] = {"ms": timed(lambda: ops.tta_boxes_to_image(det, to_image, H, W)), "bytes": na * k * (36 + 36) + na * 24}
    kern["boxes_to_aug"] = {"ms": timed(lambda: ops.tta_boxes_to_aug(box, count, to_aug)), "bytes": topk * 16 + na * topk * 16}
    n = len(got)
    kern["reduce_masks"] = {"ms": timed(lambda: ops.tta_reduce_masks(masks, flips, scores, count)),
                            "bytes": (na * n + topk) * (s * s + 1) * 4}
    for v in kern.values():
        v["memory_bound_ms"] = round(v["bytes"] / HBM_BYTES_PER_S * 1e3, 5)
        v["ms"] = round(v["ms"], 4)
        v["share_of_memory_bound"] = round(v["memory_bound_ms"] / v["ms"], 4)
        v["share_of_step"] = round(v["ms"] / ms["tta"], 5)
    res["kernels"] = kern
    res["bytes_model"] = ("hflip: float canvas written once + h-pass bytes read once, summed over the scales; box maps: every input and output "
                          "once (kilobytes: their time is a launch); reduce: the A soft masks and scores of the rows below the count read "
                          "once, the K output rows written once.  The wrapper's allocations are inside the box-map and reduce times.")
    res["new_kernels_share_of_step"] = round(sum(v["ms"] for v in kern.values()) / ms["tta"], 5)
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
