"""Writes tests/golden/conv_plan_cases.json: what ops._kernel_name / ops.executed_flops / cmk_conv_gn_records(H, W, 110 + geometry) answered
before cmk_conv_plan replaced them.  It therefore runs only at commit 7fef572, the last one that has those functions:

    python tests/golden/make_conv_plan_cases.py --menu menu.json        # on the GPU: the tuner's menu on tiny problems, really launched
    python tests/golden/make_conv_plan_cases.py --merge menu.json       # anywhere: the tuned tables + the menu -> conv_plan_cases.json

Rows: {"problem": index, "tvs": [variants that share this answer], "pool": pool_ws set, "groups": gn_groups (0 = no fused statistics),
"kernel", "flops", "gn_records" (per problem, per image) | "refused": the library's error text}.  tests/test_cpu_conv_plan.py reads it."""
import ctypes
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["CMK_ALLOW_SPLIT_BF16"] = os.environ["CMK_ALLOW_SPLIT_F16"] = "1"      # the whole menu, opt-in forms included

from centermask2_amd import _lib, ops  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "conv_plan_cases.json")
TINY = [dict(k=1, stride=1, cin=32, cout=256, x_cs=32, y_cs=256, res=0, shapes=[[1, 16, 16]]),
        dict(k=3, stride=1, cin=32, cout=80, x_cs=32, y_cs=80, res=0, shapes=[[2, 14, 14]]),
        dict(k=3, stride=2, cin=32, cout=128, x_cs=32, y_cs=128, res=0, shapes=[[1, 16, 16]]),
        dict(k=3, stride=1, cin=32, cout=80, x_cs=32, y_cs=80, res=0, shapes=[[2, 14, 14], [2, 13, 41], [2, 7, 10], [2, 4, 5], [2, 25, 12]])]
TINY_GROUPS = 5           # Cout 80 = 5 groups of 16: the statistics rows of the 3x3 stride-1 problems


def out_shape(p, s):
    return (s[0], s[1], s[2]) if p["stride"] == 1 else (s[0], (s[1] - 1) // 2 + 1, (s[2] - 1) // 2 + 1)


def answer(p, tv, pool, groups):
    """The parent's mirrors for problem p run as variant tv."""
    tv4 = ops._variant4(tv)
    taps = p["k"] * p["k"]
    name = ops._kernel_name(taps, p["stride"], tv4, aff=p["res"] >= 4, pool=bool(pool), upres=(p["res"] & 3) == 2, cout=p["cout"])
    fl = ops.executed_flops(taps, p["stride"], tv4, [out_shape(p, s) for s in p["shapes"]], p["cin"], p["cout"])
    assert fl == int(fl)
    recs = None
    if groups:
        lib = _lib.load()
        recs = [lib.cmk_conv_gn_records(s[1], s[2], 110 + tv4[2] if tv4[0] == 11 else tv4[0]) for s in p["shapes"]]
    return dict(kernel=name, flops=int(fl), gn_records=recs)


def menu_rows():
    """The start-up tuner's candidates on the tiny problems, launched on real buffers: accepted ones get the mirrors' answer, refused ones
    the library's text.  The 3x3 stride-1 problems also run the Winograd / direct-split candidates and one plain one with statistics."""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rows = []
    for pi, p in enumerate(TINY):
        n = len(p["shapes"])
        g = torch.Generator().manual_seed(pi)
        pc = ops.PackedConv(torch.randn(p["cout"], p["cin"], p["k"], p["k"], generator=g) * 0.05, None, None, dev, stride=p["stride"])
        xs = [ops.View(torch.randn(s[0], s[1], s[2], p["cin"], generator=g).to(dev)) for s in p["shapes"]]
        ys = [ops.View(torch.empty(out_shape(p, s) + (p["cout"],), device=dev)) for s in p["shapes"]]
        descs = (_lib.ConvDesc * n)()
        for i in range(n):
            ops._fill_desc(descs[i], xs[i], pc, ys[i], False, None, None, False, False)
        ops._tune(descs, n, ops._problem_key(descs, n))
        cands = list(ops.TUNE_LOG[-1][1])
        passes = [(0, cands)]
        if p["k"] == 3 and p["stride"] == 1:
            passes.append((TINY_GROUPS, [tv for tv in cands if tv[0] in (5, 6, 11)] + [(1, 16, 1, 1)]))
        for groups, tvs in passes:
            for tv in tvs:
                ws = ops._set_variant(descs, n, tv)
                gws = None
                if groups:
                    recs = sum(lib.cmk_conv_gn_records(s[1], s[2], 110 + tv[2] if tv[0] == 11 else tv[0]) for s in p["shapes"])
                    gws = torch.empty((p["shapes"][0][0] * recs, groups, 2), dtype=torch.float64, device=dev)
                for i in range(n):
                    descs[i].gn_ws, descs[i].gn_groups = (gws.data_ptr(), groups) if groups else (None, 0)
                rc = lib.cmk_conv2d_nhwc_multi(descs, n, ops._stream()) if n > 1 else lib.cmk_conv2d_nhwc(ctypes.byref(descs[0]), ops._stream())
                torch.cuda.synchronize()
                row = dict(problem=pi, tv=list(tv), pool=0, groups=groups)
                row.update(answer(p, tv, 0, groups) if rc == 0 else dict(refused=lib.cmk_last_error().decode()))
                rows.append(row)
                del ws, gws
    return rows


def table_rows(problems):
    """Every (key, variant) of the shipped tables; 1x1 entries on the pointwise kernel also with pool_ws; the 5-level tower launches also
    with statistics (32 groups, as the FCOS head runs them)."""
    lib = _lib.load()
    rows = []
    for path in sorted(glob.glob(os.path.join(ROOT, "centermask2_amd", "tuned", "*.json"))):
        for key, tv in sorted(json.load(open(path)).items()):
            k, stride, cin, cout, xcs, ycs, res, shapes = ops._str_to_key(key)
            p = dict(k=k, stride=stride, cin=cin, cout=cout, x_cs=xcs, y_cs=ycs, res=res, shapes=[list(s) for s in shapes])
            if p not in problems:
                problems.append(p)
            pi = problems.index(p)
            rows.append(dict(problem=pi, tv=list(tv), pool=0, groups=0, **answer(p, tv, 0, 0)))
            tv4 = ops._variant4(tv)
            if k == 1 and tv4[0] in (8, 10, 12) and tv4[3] == 1 and (res & 3) != 2:
                d = _lib.ConvDesc()
                d.N, d.H, d.W = shapes[0]
                d.Cin, d.Cout, d.ksize, d.stride, d.x_cs, d.y_cs, d.res_mode = cin, cout, 1, 1, xcs, ycs, res & 3
                d.tune_wm, d.tune_sc, d.tune_wn = tv4[:3]
                d.w_split = d.w_splith = 16
                if lib.cmk_conv_pool_rows(ctypes.byref(d)) > 0:
                    rows.append(dict(problem=pi, tv=list(tv), pool=1, groups=0, **answer(p, tv, 1, 0)))
            if len(shapes) == 5 and tv4[0] in (5, 6, 11) and cout % 32 == 0:
                rows.append(dict(problem=pi, tv=list(tv), pool=0, groups=32, **answer(p, tv, 0, 32)))
    return rows


def profile_rows(problems):
    """The three launches of tests/test_gpu_conv_plan.py (its literals are these answers)."""
    lib = _lib.load()
    rows = []
    for p, tv, pool in ((TINY[0], (8, 32, 2), 1),
                        (dict(k=3, stride=1, cin=32, cout=32, x_cs=32, y_cs=32, res=0, shapes=[[1, 12, 40]]), (6, 16, 1), 0),
                        (dict(k=3, stride=2, cin=32, cout=64, x_cs=32, y_cs=64, res=0, shapes=[[1, 16, 16]]), None, 0)):
        if p not in problems:
            problems.append(p)
        if tv is None:                       # untuned: what the library resolves
            d = _lib.ConvDesc()
            d.x = d.w = d.scale = d.shift = d.y = 16
            d.N, d.H, d.W = p["shapes"][0]
            d.Cin, d.Cout, d.ksize, d.stride, d.x_cs, d.y_cs = p["cin"], p["cout"], p["k"], p["stride"], p["x_cs"], p["y_cs"]
            v = (ctypes.c_int * 3)()
            _lib.check(lib.cmk_conv_resolve(ctypes.byref(d), 1, 0, v))
            rows.append(dict(problem=problems.index(p), tv=[0, 0, 0], pool=pool, groups=0, **answer(p, tuple(v), pool, 0)))
        else:
            rows.append(dict(problem=problems.index(p), tv=list(tv), pool=pool, groups=0, **answer(p, tv, pool, 0)))
    return rows


def main():
    if sys.argv[1] == "--menu":
        json.dump(menu_rows(), open(sys.argv[2], "w"))
        return
    problems = [dict(p) for p in TINY]
    rows = json.load(open(sys.argv[2])) + table_rows(problems) + profile_rows(problems)
    merged = {}                              # rows that differ in the variant alone share one row
    for r in rows:
        tv = r.pop("tv")
        merged.setdefault(json.dumps(r, sort_keys=True), (r, []))[1].append(tv)
    out = []
    for r, tvs in merged.values():
        uniq = []
        for tv in tvs:
            if tv not in uniq:
                uniq.append(tv)
        out.append(dict(r, tvs=uniq))
    with open(OUT, "w") as f:
        f.write('{"problems": [\n' + ",\n".join(json.dumps(p) for p in problems) + '\n],\n"rows": [\n' + ",\n".join(json.dumps(r) for r in out) + "\n]}\n")
    print(len(problems), "problems,", len(out), "rows,", sum(len(r["tvs"]) for r in out), "cases")


if __name__ == "__main__":
    main()
