"""Same-session A/B of library builds on the GroupNorm and plain depth-wise entry points: ab_gn_dw.py [--rounds R] <lib.so> [<lib.so> ...]
One subprocess per (round, library), interleaved, best-of per case, microseconds per call (device events around 200 calls)."""
import sys, os, subprocess
CASES = ["gn_relu_100x160", "gn_relu_13x20", "gn_affine_100x160", "gn_affine_13x20", "dw_s1_100x160x128", "dw_s2_100x160x128"]
if sys.argv[1] != "--one":
    args = sys.argv[1:]
    rounds = 3
    while args and args[0].startswith("--"):
        if args[0] == "--rounds": rounds = int(args[1])
        args = args[2:]
    res = {l: [] for l in args}
    for _ in range(rounds):
        for lib in args:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", lib], capture_output=True, text=True)
            try:
                res[lib].append([float(v) for v in r.stdout.strip().split("\n")[-1].split()])
            except Exception:
                print(lib, "FAILED", r.returncode, r.stdout[-300:], r.stderr[-600:], flush=True)
                sys.exit(1)                                  # nothing more is started on the device after a failed run
    for lib in args:
        best = [min(r[i] for r in res[lib]) for i in range(len(CASES))]
        print("%-22s" % os.path.basename(lib), " ".join("%s %.2f" % (n, b) for n, b in zip(CASES, best)), flush=True)
    sys.exit(0)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from centermask2_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[2])
from centermask2_amd import ops
dev = torch.device("cuda:0"); out = []
N, C = 8, 256
gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1


def timed(fn, reps=200):
    for _ in range(20): assert fn() == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


lib, st = _lib.load(), ops._stream()
for fn in ("relu", "affine"):                                        # the C entry points with the workspaces ops.py would pass, allocated once
    for h, w in ((100, 160), (13, 20)):
        t = torch.randn((N, h, w, C), device=dev)
        chunks = max(1, min(128, h * w // 128))
        ws = torch.empty((N, 32, chunks, 2), dtype=torch.float64, device=dev)
        sc, sh = torch.empty((N, C), device=dev), torch.empty((N, C), device=dev)
        a = (t.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), chunks, N, h * w, C, 32, 1e-5)
        if fn == "relu":                                             # in place: the values drift over the calls, the work does not
            out.append(timed(lambda: lib.cmk_groupnorm_relu_nhwc(*a, st)))
        else:
            out.append(timed(lambda: lib.cmk_groupnorm_affine(*a, sc.data_ptr(), sh.data_ptr(), st)))
x = torch.randn((N, 100, 160, 128), device=dev); w9c = torch.randn((9, 128), device=dev)
for stride in (1, 2):
    y = torch.empty((N, (100 - 1) // stride + 1, (160 - 1) // stride + 1, 128), device=dev)
    out.append(timed(lambda: lib.cmk_dwconv3x3_nhwc(x.data_ptr(), 128, 0, w9c.data_ptr(), y.data_ptr(), 128, 0, N, 100, 160, 128, stride, st)))
print(" ".join("%.3f" % v for v in out))
