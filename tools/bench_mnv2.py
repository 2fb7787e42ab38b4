"""The MobileNetV2 (CenterMask-Lite) path, measured: every depth-wise layer of the body at batch 8, 3 x 800 x 1280, on the fused kernel
(ops.dwconv3x3_bn_act: min(x, 6) on load, FrozenBN and ReLU6 in the epilogue) with the plain ops.dwconv3x3 on the same shape beside it,
and the whole Lite-Mv2 model as a graph-replayed inference_padded step at 8 x 3 x 800 x 1280 and at the recipe's 8 x 3 x 608 x 1024.

Per layer: HIP-event time, best of several interleaved rounds; algorithmic bytes from the shapes (input + output, fp32); achieved TB/s
and its share of the HBM rate a float4 copy reaches on this chip (6.29 TB/s; 8.0 TB/s is the specification).  Layers whose input and
output together fit the 256 MiB last-level cache are marked: their rate is not an HBM rate.  A tool only: bench.py does not run it.

    python tools/bench_mnv2.py [--reps 20] [--rounds 5] [--out profiles/bench_mnv2.json]
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
from centermask2_amd.ops import View  # noqa: E402

B = 8
HBM_COPY_TBS, HBM_SPEC_TBS, LLC_BYTES = 6.29, 8.0, 256 << 20
LITE = dict(fpn_ch=128, mask_dim=128, num_tower_convs=2, mask_num_conv=2, maskiou_num_conv=2)


def dw_layers(h, w):
    """(block index, H, W, C, stride) of the depth-wise conv of features[1..17] for an h x w image."""
    out, cin, idx = [], 32, 1
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for t, c, n, s in S.MNV2_SETTING:
        for i in range(n):
            stride = s if i == 0 else 1
            out.append((idx, h, w, cin * t, stride))
            h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
            cin, idx = c, idx + 1
    return out


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_layers(dev, h, w, reps, rounds):
    shapes = {}
    for idx, lh, lw, c, stride in dw_layers(h, w):
        shapes.setdefault((lh, lw, c, stride), []).append(idx)
    g = torch.Generator().manual_seed(0)
    rows = []
    for (lh, lw, c, stride), blocks in shapes.items():
        x = View((torch.randn((B, lh, lw, c), generator=g) * 4.0).to(dev))
        ho, wo = (lh - 1) // stride + 1, (lw - 1) // stride + 1
        y = View(torch.empty((B, ho, wo, c), device=dev))
        w9c = (torch.randn((9, c), generator=g) / 3.0).to(dev)
        sc, sh = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
        fused = lambda: ops.dwconv3x3_bn_act(x, w9c, sc, sh, y, stride=stride, in_max=6.0, out_min=0.0, out_max=6.0)      # noqa: E731
        plain = lambda: ops.dwconv3x3(x, w9c, y, stride=stride)                                                          # noqa: E731
        for fn in (fused, plain):
            _time(fn, 3)
        ms = {"fused": [], "plain": []}
        for _ in range(rounds):
            ms["fused"].append(_time(fused, reps))
            ms["plain"].append(_time(plain, reps))
        nbytes = 4 * B * c * (lh * lw + ho * wo)
        best = min(ms["fused"])
        rows.append(dict(blocks=blocks, H=lh, W=lw, C=c, stride=stride, bytes=nbytes, fits_last_level_cache=nbytes <= LLC_BYTES,
                         fused_us=dict(best=round(best * 1e3, 2), worst=round(max(ms["fused"]) * 1e3, 2)),
                         plain_dwconv_us=dict(best=round(min(ms["plain"]) * 1e3, 2), worst=round(max(ms["plain"]) * 1e3, 2)),
                         fused_tb_per_s=round(nbytes / (best * 1e-3) / 1e12, 3),
                         share_of_copy_rate=round(nbytes / (best * 1e-3) / 1e12 / HBM_COPY_TBS, 3),
                         share_of_spec_rate=round(nbytes / (best * 1e-3) / 1e12 / HBM_SPEC_TBS, 3)))
        del x, y
    return rows


def capture(step):
    step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    torch.cuda.synchronize()
    return graph, out


def bench_model(model, dev, h, w, reps, rounds):
    x = S.make_synthetic_images(B, h, w, seed0=1234).to(dev)
    sizes = [(h, w)] * B

    def full():
        out = model.inference_padded(x, sizes)
        return out, pack_records(out)

    graphs = {"model": capture(full), "backbone": capture(lambda: model.backbone(x)), "body": capture(lambda: model.backbone.bottom_up(x))}
    for g, _ in graphs.values():
        _time(g.replay, 3)
    ms = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, (g, _) in graphs.items():
            ms[k].append(_time(g.replay, reps))
    counts = graphs["model"][1][0]["counts"].cpu()
    res = dict(batch=B, image=[h, w], detections=int(counts.sum()),
               ms_per_step={k: dict(best=round(min(v), 3), worst=round(max(v), 3)) for k, v in ms.items()},
               img_per_s=round(B / min(ms["model"]) * 1e3, 1))
    del graphs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_lite_Mv2_FPN_ms_4x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", str(dev)])
    cfg.freeze()
    model = build_model(cfg).eval()
    model.load_state_dict(S.make_synthetic_state_dict(S.MOBILENETV2, 0, **LITE))
    with torch.no_grad():
        layers = bench_layers(dev, 800, 1280, a.reps, a.rounds)
        models = [bench_model(model, dev, h, w, max(a.reps // 2, 1), a.rounds) for h, w in ((800, 1280), (608, 1024))]
    total = sum(r["bytes"] * len(r["blocks"]) for r in layers)
    us = sum(r["fused_us"]["best"] * len(r["blocks"]) for r in layers)
    res = dict(depthwise_layers=layers, depthwise_total=dict(bytes=total, fused_us=round(us, 1), tb_per_s=round(total / (us * 1e-6) / 1e12, 3)),
               lite_mv2_model=models, hbm_tb_per_s=dict(float4_copy=HBM_COPY_TBS, spec=HBM_SPEC_TBS), reps=a.reps, rounds=a.rounds,
               variants="library defaults (no measured variant table for this model)")
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
