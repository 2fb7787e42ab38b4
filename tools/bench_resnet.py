"""The ResNet path, measured at the bench shape (batch 8, 3 x 800 x 1280):
  * the fused stem launch (ops.stem7x7_bn_relu_maxpool) beside the same arithmetic as F.conv2d + affine + relu + F.max_pool2d through
    PyTorch-ROCm on the same device (an outside yardstick: NCHW, MIOpen), and beside the kernel's own roofline: the bytes it must
    move (image in, pooled map out) at the float4-copy HBM rate, and its FLOPs times the recompute factor of its tiling (128 GEMM rows
    for the 96 conv pixels a workgroup owns) at the fp32 matrix rate;
  * the R-50 and R-101 CenterMask models as graph-replayed inference_padded steps, with V-39 from the same session beside them (all on
    the library's default conv variants; V-39 also with its shipped variant table, as bench.py runs it);
  * the three ops.maxpool1x1s2 launches that stand in for the stride of the 1x1 convs, as a share of the R-50 step.
HIP-event times, best and worst of several interleaved rounds.  A tool only: bench.py does not run it.

    python tools/bench_resnet.py [--reps 20] [--rounds 5] [--out profiles/bench_resnet.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from centermask2_amd import ops  # noqa: E402
from centermask2_amd import synthetic as S  # noqa: E402
from centermask2_amd.config import config_path, get_cfg  # noqa: E402
from centermask2_amd.dist import pack_records  # noqa: E402
from centermask2_amd.modeling import build_model  # noqa: E402
from centermask2_amd.ops import View  # noqa: E402

B, H, W = 8, 800, 1280
HBM_COPY_TBS, FP32_MATRIX_TFLOPS = 6.29, 157.3
STEM_ROWS_PER_OWNED_PIXEL = 128.0 / 96.0          # csrc/stem7_pool.hip: 4 x 32 GEMM rows per 8 x 12 owned conv pixels


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _rounds(fns, reps, rounds):
    for fn in fns.values():
        _time(fn, 3)
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(_time(fn, reps))
    return {k: dict(best=round(min(v) * 1e3, 2), worst=round(max(v) * 1e3, 2)) for k, v in ms.items()}


def bench_stem(dev, reps, rounds):
    key = "backbone.bottom_up.stem.conv1."
    w = S.synthetic_tensor(key + "weight", (64, 3, 7, 7))
    scale, shift = ops.fold_frozen_bn(*[S.synthetic_tensor(key + "norm." + n, (64,)) for n in ("weight", "bias", "running_mean", "running_var")])
    x = S.make_synthetic_images(B, H, W, seed0=1234).to(dev)
    w147, wd, sc, sh = ops.pack_stem7_weight(w).to(dev), w.to(dev), scale.to(dev), shift.to(dev)
    hc, wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    y = View(torch.empty((B, hp, wp, 64), device=dev))
    sc4, sh4 = sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1)

    def torch_pair():
        return F.max_pool2d(F.relu_(F.conv2d(x, wd, None, 2, 3).mul_(sc4).add_(sh4)), 3, 2, 1)

    def torch_conv_pool_only():                       # the two library calls alone, without the affine and relu passes
        return F.max_pool2d(F.conv2d(x, wd, None, 2, 3), 3, 2, 1)

    us = _rounds({"fused": lambda: ops.stem7x7_bn_relu_maxpool(x, w147, sc, sh, y), "torch_conv_affine_relu_pool": torch_pair,
                  "torch_conv_pool_only": torch_conv_pool_only}, reps, rounds)
    err = float((y.t.permute(0, 3, 1, 2) - torch_pair()).abs().max())
    nbytes = 4 * (B * 3 * H * W + B * hp * wp * 64)
    flops = 2.0 * 147 * 64 * B * hc * wc
    roof_us = max(nbytes / (HBM_COPY_TBS * 1e12), flops * STEM_ROWS_PER_OWNED_PIXEL / (FP32_MATRIX_TFLOPS * 1e12)) * 1e6
    best = us["fused"]["best"]
    return dict(shape=[B, 3, H, W], us=us, max_abs_diff_fused_vs_torch=err, bytes=nbytes, conv_map_bytes_not_written=4 * B * hc * wc * 64, flops=flops,
                recompute_factor=round(STEM_ROWS_PER_OWNED_PIXEL, 3), roofline_us=round(roof_us, 1), share_of_roofline=round(roof_us / best, 3),
                achieved_tflops_useful=round(flops / (best * 1e-6) / 1e12, 1), fused_over_torch=round(best / us["torch_conv_affine_relu_pool"]["best"], 3))


def bench_subsample(dev, reps, rounds):
    fns, shapes = {}, {}
    for name, c, div in (("res3.0", 256, 4), ("res4.0", 512, 8), ("res5.0", 1024, 16)):
        x = View(torch.randn((B, H // div, W // div, c), device=dev))
        fns[name] = (lambda v: (lambda: ops.maxpool1x1s2(v)))(x)
        shapes[name] = [B, H // div, W // div, c]
    us = _rounds(fns, reps, rounds)
    return dict(input_shapes_nhwc=shapes, us=us, total_us_best=round(sum(v["best"] for v in us.values()), 2))


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


def bench_model(yaml, body, dev, reps, rounds):
    cfg = get_cfg()
    cfg.merge_from_file(config_path(yaml))
    cfg.merge_from_list(["MODEL.DEVICE", str(dev)])
    cfg.freeze()
    model = build_model(cfg).eval()
    model.load_state_dict(S.make_synthetic_state_dict(body, 0))
    x = S.make_synthetic_images(B, H, W, seed0=1234).to(dev)
    sizes = [(H, W)] * B

    def full():
        out = model.inference_padded(x, sizes)
        return out, pack_records(out)

    graphs = {"model": capture(full), "backbone": capture(lambda: model.backbone(x)), "body": capture(lambda: model.backbone.bottom_up(x))}
    us = _rounds({k: g.replay for k, (g, _) in graphs.items()}, reps, rounds)
    counts = graphs["model"][1][0]["counts"].cpu()
    res = dict(body=body, batch=B, image=[H, W], detections=int(counts.sum()),
               ms_per_step={k: dict(best=round(v["best"] / 1e3, 3), worst=round(v["worst"] / 1e3, 3)) for k, v in us.items()},
               img_per_s=round(B / us["model"]["best"] * 1e6, 1))
    del graphs, model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_autotune(False)
    mreps = max(a.reps // 2, 1)
    with torch.no_grad():
        stem = bench_stem(dev, a.reps, a.rounds)
        sub = bench_subsample(dev, a.reps, a.rounds)
        models = [bench_model("centermask_R_50_FPN_ms_3x.yaml", "R-50", dev, mreps, a.rounds),
                  bench_model("centermask_R_101_FPN_ms_3x.yaml", "R-101", dev, mreps, a.rounds),
                  bench_model("centermask_V_39_eSE_FPN_ms_3x.yaml", "V-39-eSE", dev, mreps, a.rounds)]
        for m in models:
            m["variants"] = "library defaults"
        table = os.path.join(ROOT, "centermask2_amd", "tuned", "mi355x_V-39-eSE_b{}_800x1280.json".format(B))
        if os.path.exists(table):
            ops.load_tuned(table)
            models.append(dict(bench_model("centermask_V_39_eSE_FPN_ms_3x.yaml", "V-39-eSE", dev, mreps, a.rounds), variants="shipped table " + os.path.basename(table)))
    r50 = models[0]["ms_per_step"]["model"]["best"]
    sub["share_of_r50_step"] = round(sub["total_us_best"] / 1e3 / r50, 4)
    stem["share_of_r50_step"] = round(stem["us"]["fused"]["best"] / 1e3 / r50, 4)
    res = dict(stem=stem, subsample_launches=sub, models=models, rates=dict(hbm_float4_copy_tb_per_s=HBM_COPY_TBS, fp32_matrix_tflops=FP32_MATRIX_TFLOPS),
               reps=a.reps, rounds=a.rounds)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
