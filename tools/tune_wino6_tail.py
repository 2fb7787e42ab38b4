"""Targeted re-tuning of the RoI-pair F(4x4,3x3) convs (tune 6 / 16|32 / 2) for tail split-K (cmk.h splitk_tail): every such problem of
the model is timed on its real buffers with the shipped table's choice and with the tail in 2, 4 and 8 ways on both forms, interleaved,
and a table with the winners is written.
python tools/tune_wino6_tail.py <body> <out.json> [margin]   (a tail must beat the incumbent by `margin`, default 1.02)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from centermask2_amd import ops
import bench
body, out = sys.argv[1], sys.argv[2]
margin = float(sys.argv[3]) if len(sys.argv) > 3 else 1.02
B = 8
dev = torch.device("cuda:0")
ops._TUNED.clear()
ops.load_tuned(os.path.join(bench.ROOT, "centermask2_amd", "tuned", "mi355x_{}_b{}_800x1280.json".format(body, B)))
incumbent = {k: v for k, v in ops._TUNED.items() if k[0] == 3 and k[1] == 1 and tuple(v[:1]) == (6,) and v[1] in (16, 32) and v[2] == 2}
for k in incumbent: del ops._TUNED[k]
ops.TUNE_ONLY = lambda key: ([tuple(incumbent[key][:4])] + [(6, sc, 2, 1, t) for sc in (16, 32) for t in (2, 4, 8)]) if key in incumbent else [(0, 0, 0)]
ops.TUNE_REPS, ops.TUNE_ROUNDS = 10, 5
ops.set_autotune(True)
from centermask2_amd import synthetic as S
model, _ = bench.build(body, dev)
x = S.make_synthetic_images(B, 800, 1280, seed0=1234).to(dev)
with torch.no_grad():
    model.inference_padded(x, [(800, 1280)] * B)
torch.cuda.synchronize()
won = 0
for key, times in ops.TUNE_LOG:
    if key not in incumbent: continue
    inc = ops._variant5(tuple(incumbent[key][:4]))
    t_inc = times.get(inc, float("inf"))
    best = min(times, key=times.get)
    keep = best if (len(best) == 5 and times[best] * margin < t_inc) else inc
    ops._TUNED[key] = keep[:3] if (keep[3] == 1 and len(keep) == 4) else keep
    won += len(keep) == 5
    print("%-70s inc %s %.4f | %s | -> %s" % (ops._key_to_str(key), list(incumbent[key]), t_inc,
                                            " ".join("sc%d/t%d %.4f" % (tv[1], tv[4], ms) for tv, ms in times.items() if len(tv) == 5), list(ops._TUNED[key])), flush=True)
ops.save_tuned(out)
print("RoI-pair 3x3 problems: %d, with a tail: %d; table: %s" % (len(incumbent), won, out))
