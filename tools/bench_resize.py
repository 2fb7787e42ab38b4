"""Resize front end (ops.resize_preprocess_images: cmk_resize_h_u8 + cmk_resize_v_preprocess) at the deployment shape — 8 raw 480x640
uint8 images -> 800x1067, padded to 800x1088 — against ops.preprocess_images on the 8 already-resized CHW uint8 images, which is all the
device did for the same batch before the resize moved to it.  One process, device events, warm-up, interleaved rounds.  A tool only:
bench.py does not run it.

    python tools/bench_resize.py [--reps 20] [--rounds 7] [--out profiles/bench_resize.json]

Bytes the two passes must move per image (each input byte read once, each output byte written once):
    horizontal  h*w*3 read + h*new_w*3 written;   vertical  h*new_w*3 read + 3*H*W*4 written (the float slot, padding included).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from centermask2_amd import _lib, ops  # noqa: E402

B, H_IN, W_IN, SHORT, MAX_SIZE = 8, 480, 640, 800, 1333
MEAN, STD = (103.53, 116.28, 123.675), (1.0, 1.0, 1.0)
MODEL_STEP_MS = 21.5      # README: V-39 at bs 8, 800x1280


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_resize.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs the GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    raws = [torch.randint(0, 256, (H_IN, W_IN, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    new_h, new_w = ops.resize_shortest_edge_shape(H_IN, W_IN, SHORT, MAX_SIZE)
    resized_chw = [ops.resize_bilinear_u8(r, new_h, new_w).permute(2, 0, 1).contiguous() for r in raws]
    ws = torch.empty((H_IN * new_w * 3 + 3,), dtype=torch.uint8, device=dev)
    fns = {
        "resize_preprocess": lambda: ops.resize_preprocess_images(raws, SHORT, MAX_SIZE, MEAN, STD),
        "preprocess_images": lambda: ops.preprocess_images(resized_chw, MEAN, STD),
        "horizontal_pass_only": lambda: [ops._resize_h(lib, r, new_w, ws) for r in raws],
    }
    outs = {}
    for k, f in fns.items():                                           # warm-up: code objects, tables, allocator
        for _ in range(3):
            outs[k] = f()
    torch.cuda.synchronize()
    batch, sizes = outs["resize_preprocess"]
    want, _ = outs["preprocess_images"]
    assert torch.equal(batch, want), "the fused path must give the bits of preprocess_images on the resized images"
    Hp, Wp = batch.shape[2], batch.shape[3]
    # the same two bodies captured once and replayed: device work without the host's launch cost (sequential kernels, one stream)
    graphs = {}
    for k in ("resize_preprocess", "preprocess_images"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fns[k]()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            kept = fns[k]()
        gr.replay(); gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(kept[0], want)
        graphs[k] = (gr, kept)
        fns[k + "_graph"] = gr.replay
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):                                          # interleaved
        for k, f in fns.items():
            ms[k].append(_timed(f, a.reps))
    h_bytes = B * (H_IN * W_IN * 3 + H_IN * new_w * 3)
    v_bytes = B * (H_IN * new_w * 3 + 3 * Hp * Wp * 4)
    pre_bytes = B * (3 * new_h * new_w + 3 * Hp * Wp * 4)
    best = {k: min(v) for k, v in ms.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = dict(shape=dict(batch=B, raw=[H_IN, W_IN], resized=[new_h, new_w], padded=[Hp, Wp]), reps=a.reps, rounds=a.rounds,
               ms_per_batch_best={k: round(v, 4) for k, v in best.items()}, ms_per_batch_median={k: round(v, 4) for k, v in med.items()},
               bytes_per_batch=dict(horizontal=h_bytes, vertical=v_bytes, resize_preprocess=h_bytes + v_bytes, preprocess_images=pre_bytes),
               GBps_best=dict(resize_preprocess=round((h_bytes + v_bytes) / best["resize_preprocess"] / 1e6, 1),
                              preprocess_images=round(pre_bytes / best["preprocess_images"] / 1e6, 1),
                              horizontal_pass_only=round(h_bytes / best["horizontal_pass_only"] / 1e6, 1)),
               ratio_to_preprocess_images=dict(best=round(best["resize_preprocess"] / best["preprocess_images"], 3),
                                               median=round(med["resize_preprocess"] / med["preprocess_images"], 3)),
               share_of_model_step=dict(model_step_ms=MODEL_STEP_MS, resize_preprocess=round(best["resize_preprocess"] / MODEL_STEP_MS, 4),
                                        preprocess_images=round(best["preprocess_images"] / MODEL_STEP_MS, 4)),
               upload_bytes_per_image=dict(raw_u8=H_IN * W_IN * 3, resized_float=3 * new_h * new_w * 4),
               ratio_to_preprocess_images_graph=dict(best=round(best["resize_preprocess_graph"] / best["preprocess_images_graph"], 3),
                                                     median=round(med["resize_preprocess_graph"] / med["preprocess_images_graph"], 3)),
               GBps_best_graph=dict(resize_preprocess=round((h_bytes + v_bytes) / best["resize_preprocess_graph"] / 1e6, 1),
                                    preprocess_images=round(pre_bytes / best["preprocess_images_graph"] / 1e6, 1)),
               share_of_model_step_graph=dict(resize_preprocess=round(best["resize_preprocess_graph"] / MODEL_STEP_MS, 4),
                                              preprocess_images=round(best["preprocess_images_graph"] / MODEL_STEP_MS, 4)),
               note="device-event times; the plain legs are eager calls (16 / 8 launches per batch plus the allocation of the batch tensor, "
                    "host launch cost included), the _graph legs replay the same launches from a captured graph")
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
