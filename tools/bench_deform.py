"""Deformable 3x3 conv (cmk_deform_conv3x3_nhwc) on the V-39 DCN layer shapes at bs 8, 800x1280, against ops.conv2d of the same
shape, and whole-model throughput with STAGE_WITH_DCN = (False, True, True, True) against the default model — one process, device
events, warm-up, interleaved / alternating runs.  A tool only: bench.py does not run it.

    python tools/bench_deform.py [--reps 5] [--model-steps 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from centermask2_amd import ops, synthetic as S  # noqa: E402
from centermask2_amd.ops import View  # noqa: E402

B = 8
LAYERS = [  # name, H, W, Cin, Cout (first layer of each block: Cin = the block input; inner layers: Cin = the stage width)
    ("OSA3_1_0", 100, 160, 256, 160), ("OSA3_1_1", 100, 160, 160, 160),
    ("OSA4_1_0", 50, 80, 512, 192), ("OSA4_1_1", 50, 80, 192, 192), ("OSA4_2_0", 50, 80, 768, 192),
    ("OSA5_1_0", 25, 40, 768, 224), ("OSA5_1_1", 25, 40, 224, 224), ("OSA5_2_0", 25, 40, 1024, 224),
]
PEAK_TF = 157.3          # fp32 matrix peak of the MI355X


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_leg(dev, reps, rounds=3, modulated=False, dg=1):
    rows = []
    for name, h, w, cin, cout in LAYERS:
        g = torch.Generator().manual_seed(1)
        x = View(torch.randn((B, h, w, cin), generator=g).to(dev))
        wt = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
        noff = (27 if modulated else 18) * dg
        pc_off = ops.PackedConv(torch.randn((noff, cin, 3, 3), generator=g) * (1.5 / (cin * 9) ** 0.5), None,
                                torch.randn(noff, generator=g) * 0.5, dev)
        pd = ops.PackedDeformConv(wt, None, None, dev)
        pc = ops.PackedConv(wt, None, None, dev)
        y = View(torch.empty((B, h, w, cout), device=dev))
        off = ops.conv_out(x, pc_off)
        fns = {"deform": lambda: ops.deform_conv3x3(x, off.t, pd, y, dg, modulated),
               "offset_conv": lambda: ops.conv2d(x, pc_off, off),
               "conv3x3": lambda: ops.conv2d(x, pc, y, relu=True)}
        for f in fns.values():
            f(); f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(rounds):                                        # interleaved
            for k, f in fns.items():
                ms[k].append(_timed(f, reps))
        best = {k: min(v) for k, v in ms.items()}
        tiles = -(-(-(-cout // 32)) // 7)
        cout_exec = tiles * (-(-(-(-cout // 32)) // tiles)) * 32
        flops_exec = 2.0 * B * h * w * 9 * cin * cout_exec
        gathered = 4.0 * 4 * B * h * w * 9 * cin * tiles               # 4 corners x fp32 per sampled value, per cout tile
        rows.append(dict(layer=name, H=h, W=w, Cin=cin, Cout=cout, dg=dg, modulated=modulated,
                         deform_ms=round(best["deform"], 4), offset_conv_ms=round(best["offset_conv"], 4), conv3x3_ms=round(best["conv3x3"], 4),
                         dcn_over_conv=round((best["deform"] + best["offset_conv"]) / best["conv3x3"], 3),
                         deform_tflops_exec=round(flops_exec / best["deform"] / 1e9, 1),
                         deform_peak_share=round(flops_exec / best["deform"] / 1e9 / PEAK_TF, 3),
                         gathered_GBps=round(gathered / best["deform"] / 1e6, 0)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def model_leg(dev, steps, rounds=3):
    from centermask2_amd.config import config_path, get_cfg
    from centermask2_amd.modeling import build_model
    table = os.path.join(ROOT, "centermask2_amd", "tuned", "mi355x_V-39-eSE_b8_800x1280.json")
    if os.path.exists(table):
        ops.load_tuned(table)
    x = S.make_synthetic_images(B, 800, 1280, seed0=1234).to(dev)
    sizes = [(800, 1280)] * B
    graphs = {}
    for name, flags in (("default", (False,) * 4), ("dcn_stage3-5", (False, True, True, True))):
        cfg = get_cfg()
        cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
        cfg.merge_from_list(["MODEL.DEVICE", str(dev), "MODEL.VOVNET.STAGE_WITH_DCN", flags])
        cfg.freeze()
        model = build_model(cfg).eval()
        model.load_state_dict(S.make_synthetic_state_dict("V-39-eSE", 0, stage_with_dcn=flags))
        with torch.no_grad():
            model.inference_padded(x, sizes)
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.inference_padded(x, sizes)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = model.inference_padded(x, sizes)
        graph.replay(); graph.replay()
        torch.cuda.synchronize()
        graphs[name] = (graph, out, model)
    ms = {k: [] for k in graphs}
    for _ in range(rounds):                                            # alternating
        for k, (graph, _, _) in graphs.items():
            ms[k].append(_timed(graph.replay, steps))
    res = {k: dict(images_per_sec=round(B * 1e3 / min(v), 1), ms_per_step=round(min(v), 3),
                   detections_per_image=graphs[k][1]["counts"].cpu().tolist()) for k, v in ms.items()}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model-steps", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"layers_v1_dg1": layer_leg(dev, a.reps), "layers_mod_dg2": layer_leg(dev, a.reps, modulated=True, dg=2)}
    if not a.skip_model:
        res["model"] = model_leg(dev, a.model_steps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
