"""Same bits from two library builds on the pointwise and direct-split convs: ab_conv_bits.py <lib.so> <lib.so> [...]
Every accepted case of the conformance table (tests/conv_cases.py) of the families that run conv_pw_kernel or conv_sp3_kernel — census rows
and feature rows — is launched on seeded inputs in one child process per library; the child prints a hash of every output view, of the pooled
sums and of the GroupNorm records where the case has them.  The parent compares the lists: exit status 0 when every library gave the first
one's hashes for every case.  Nothing is checked against a reference here (tests/test_gpu_conv_conformance.py does that)."""
import hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FAMILIES = ("pw (wm 8)", "pw gather (wm 9)", "pw split bf16 (wm 10)", "pw split fp16 (wm 12)", "sp3 (sc 2)", "sp3 (sc 21)")
if len(sys.argv) < 2 or sys.argv[1] != "--one":
    libs = sys.argv[1:]
    runs = []
    for lib in libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", lib], capture_output=True, text=True)
        rows = dict(l.split("\t")[1:3] for l in r.stdout.splitlines() if l.startswith("case\t"))
        if r.returncode != 0 or not rows:
            print(lib, "FAILED", r.stdout[-300:], r.stderr[-900:])
            sys.exit(2)
        runs.append(rows)
    bad = 0
    for name, h in runs[0].items():
        same = all(rows.get(name) == h for rows in runs[1:])
        bad += not same
        print("%s %s %s" % (h, "identical" if same else "DIFFERENT " + " ".join(str(rows.get(name)) for rows in runs[1:]), name))
    bad += sum(len(rows) != len(runs[0]) for rows in runs[1:])
    print("%d cases, %d libraries: %s" % (len(runs[0]), len(libs), "all identical" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)
sys.path.insert(0, ROOT)
import torch
from centermask2_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[2])
from centermask2_amd import ops
from tests import conv_cases as cc
from tests.test_gpu_conv_conformance import _device_buffers, _launch
ops.ALLOW_SPLIT_BF16 = ops.ALLOW_SPLIT_F16 = True
ops.FORCE_VARIANT = None
lib = _lib.load(); dev = torch.device("cuda:0")
for i, c in enumerate(cc.all_cases()):
    if c["family"] not in FAMILIES or c["answer"] != "accept":
        continue
    t = cc.host_tensors(c, i)
    b = _device_buffers(c, t, dev)
    descs, keep = cc.fill_descs(c, _lib, bufs=b, ops=ops)
    assert (keep["affine"] is not None) == bool(c["gn_groups"]), (c["id"], "a case with GroupNorm groups and no records to hash")
    if keep["affine"] is not None:
        keep["affine"].records.fill_(float("nan"))       # a record the kernel leaves unwritten hashes as NaN, not as what the allocator left
    rc, err = _launch(lib, descs)
    assert rc == 0, (c["id"], err)
    h = hashlib.sha1()
    (_, _), (_, y_co) = cc.views_of(c)
    for yv in b["yv"]:
        h.update(yv.t[..., y_co:y_co + c["cout"]].contiguous().cpu().numpy().tobytes())
    if keep["pool"] is not None:
        h.update(keep["pool"].cpu().numpy().tobytes())
    if keep["affine"] is not None:              # the records themselves: the workspace ops._gn_records pointed the descriptors at
        h.update(keep["affine"].records.cpu().numpy().tobytes())
    print("case\t%s\t%s" % (c["id"], h.hexdigest()[:16]), flush=True)
