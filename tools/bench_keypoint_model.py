"""The keypoint branch inside the model: the graph-replayed step of bench.py (bs 8, 3 x 800 x 1280, V-39, synthetic weights, the shipped
conv variant table, inference_padded + the result record) with MODEL.KEYPOINT_ON and IN_FEATURES p3-p5, K = 17, beside the same step
without it, interleaved in one session.  The keypoint head's convs are not in the variant table and run on the library's defaults.
Reports ms per step of both, the difference, and the detections the synthetic weights give (the decode's work grows with the box area).
A tool only: bench.py does not run it.

    python tools/bench_keypoint_model.py [--reps 10] [--rounds 5] [--topk 50] [--out profiles/bench_keypoint_model.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from centermask2_amd import ops  # noqa: E402
from centermask2_amd import synthetic as S  # noqa: E402
from centermask2_amd.config import config_path, get_cfg  # noqa: E402
from centermask2_amd.dist import pack_records  # noqa: E402
from centermask2_amd.modeling import build_model  # noqa: E402

B, H, W, BODY = 8, 800, 1280, "V-39-eSE"


def build(keypoint_on, topk, dev):
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", str(dev), "MODEL.KEYPOINT_ON", keypoint_on, "MODEL.ROI_KEYPOINT_HEAD.IN_FEATURES", ["p3", "p4", "p5"],
                         "MODEL.FCOS.POST_NMS_TOPK_TEST", topk])
    cfg.freeze()
    model = build_model(cfg).eval()
    model.load_state_dict(S.make_synthetic_state_dict(BODY, 0, keypoint_on=keypoint_on))
    return model


def capture(model, x, sizes):
    def step():
        out = model.inference_padded(x, sizes)
        return out, pack_records(out)
    step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, rec = step()
    torch.cuda.synchronize()
    return graph, out, rec


def _timed(graph, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--topk", type=int, default=50, help="MODEL.FCOS.POST_NMS_TOPK_TEST: slots per image of the padded layout (the yaml's 50)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    table = os.path.join(ROOT, "centermask2_amd", "tuned", "mi355x_{}_b{}_800x1280.json".format(BODY, B))
    n_loaded = ops.load_tuned(table) if os.path.exists(table) else 0
    x = S.make_synthetic_images(B, H, W, seed0=1234).to(dev)
    sizes = [(H, W)] * B
    runs = {}
    with torch.no_grad():
        for name, on in (("keypoint_off", False), ("keypoint_on", True)):
            runs[name] = capture(build(on, a.topk, dev), x, sizes)
        for g, _, _ in runs.values():
            _timed(g, 3)
        ms = {name: [] for name in runs}
        for _ in range(a.rounds):
            for name, (g, _, _) in runs.items():
                ms[name].append(_timed(g, a.reps))
    out_on, out_off = runs["keypoint_on"][1], runs["keypoint_off"][1]
    counts = out_on["counts"].cpu()
    valid = torch.arange(a.topk)[None, :] < counts[:, None]
    box = out_on["box"].cpu()[valid]
    bw, bh = (box[:, 2] - box[:, 0]).clamp(min=1).ceil(), (box[:, 3] - box[:, 1]).clamp(min=1).ceil()
    same = all(torch.equal(out_on[k], out_off[k]) for k in ("box", "score", "cls", "counts", "pred_masks", "mask_scores"))
    best = {name: min(v) for name, v in ms.items()}
    res = dict(batch=B, image=[H, W], body=BODY, num_keypoints=int(out_on["pred_keypoints"].shape[2]), slots=B * a.topk, detections=int(counts.sum()),
               ms_per_step={name: dict(best=round(min(v), 3), worst=round(max(v), 3)) for name, v in ms.items()},
               img_per_s={name: round(B / v * 1e3, 1) for name, v in best.items()},
               keypoint_branch_ms=round(best["keypoint_on"] - best["keypoint_off"], 3),
               keypoint_branch_share_of_step=round(1.0 - best["keypoint_off"] / best["keypoint_on"], 4),
               box_side_px=dict(min=round(float(torch.minimum(bw, bh).min()), 1), max=round(float(torch.maximum(bw, bh).max()), 1)),
               decode_work_pixels=int(float((bw * bh).sum()) * out_on["pred_keypoints"].shape[2]),
               record_floats_per_image=dict(keypoint_off=int(runs["keypoint_off"][2].shape[1]), keypoint_on=int(runs["keypoint_on"][2].shape[1])),
               other_outputs_bit_identical=bool(same), reps=a.reps, rounds=a.rounds,
               variants="{} entries of {} + library defaults for the keypoint head".format(n_loaded, os.path.relpath(table, ROOT)))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
