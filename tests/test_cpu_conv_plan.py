"""cmk_conv_plan, the library's own account of a conv launch (kernel name, executed FLOPs, fused-GroupNorm records), against the answers the
Python mirrors it replaced gave at the last commit that had them (tests/golden/conv_plan_cases.json; DESIGN.md, "The plan golden", says how it was recorded):
every (key, variant) of the shipped tables and the start-up tuner's whole menu on tiny problems, refusals with their text.  No GPU: dummy
aligned pointers, nothing is launched."""
import ctypes
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_STATS = "conv: fused GroupNorm statistics are only produced by the Winograd form"


def _cases():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan_cases.json")) as f:
        return json.load(f)


def _descs(_lib, ptr, p, tv, pool, groups, gn_ws):
    """The descriptors ops.py fills for problem p run as variant tv = (wm, sc, wn[, splitk[, tail ways]])."""
    n = len(p["shapes"])
    descs = (_lib.ConvDesc * n)()
    for d, (N, H, W) in zip(descs, p["shapes"]):
        d.x = d.w = d.scale = d.shift = d.y = d.w_wino = d.w_wino6 = d.w_split = d.w_splith = ptr
        d.w_splith_scale = 1.0
        d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = N, H, W, p["cin"], p["cout"], p["k"], p["stride"]
        d.x_cs, d.y_cs = p["x_cs"], p["y_cs"]
        d.res_mode = p["res"] & 3
        if d.res_mode:
            d.res, d.res_cs, d.Hr, d.Wr = ptr, p["cout"], (H + 1) // 2, (W + 1) // 2
        if p["res"] >= 4:
            d.in_scale = d.in_shift = ptr
        d.tune_wm, d.tune_sc, d.tune_wn = tv[:3]
        d.gn_groups, d.gn_ws = groups, (ptr if gn_ws else None)
    d = descs[0]
    if len(tv) > 3 and tv[3] > 1:
        d.splitk, d.splitk_ws = tv[3], ptr
    if len(tv) > 4 and tv[4] > 1:
        d.splitk_tail, d.splitk_ws = tv[4], ptr
    if pool:
        d.pool_ws = ptr
    return descs


def _plan(lib, descs):
    n = len(descs)
    name, flops, recs = ctypes.create_string_buffer(96), ctypes.c_double(), (ctypes.c_int * n)()
    if lib.cmk_conv_plan(descs, n, name, len(name), ctypes.byref(flops), recs) != 0:
        return {"refused": lib.cmk_last_error().decode()}
    return {"kernel": name.value.decode(), "flops": flops.value, "gn_records": list(recs)}


def test_plan_reproduces_every_recorded_answer():
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    cases = _cases()
    checked = 0
    for row in cases["rows"]:
        p = cases["problems"][row["problem"]]
        for tv in row["tvs"]:
            what = (p, tv, row["pool"], row["groups"])
            got = _plan(lib, _descs(_lib, ptr, p, tv, row["pool"], row["groups"], gn_ws=row["groups"] > 0))
            if "refused" in row:
                assert got == {"refused": row["refused"]}, what
            else:
                assert "refused" not in got, (what, got)
                assert got["kernel"] == row["kernel"] and got["flops"] == row["flops"], (what, got)
                assert got["gn_records"] == (row["gn_records"] or [0] * len(p["shapes"])), (what, got)
            if row["groups"]:
                # the question ops.py asks before it has a workspace (gn_groups, no gn_ws): the same answer, except that a kernel without
                # statistics is planned as the launch without them
                ask = _plan(lib, _descs(_lib, ptr, p, tv, row["pool"], row["groups"], gn_ws=False))
                if row.get("refused") == NO_STATS:
                    assert ask == _plan(lib, _descs(_lib, ptr, p, tv, row["pool"], 0, gn_ws=False)) and not any(ask["gn_records"]), what
                else:
                    assert ask == got, what
            checked += 1
    assert checked == sum(len(r["tvs"]) for r in cases["rows"]) and checked > 600


def test_plan_names_are_kernels_of_the_library():
    """Every distinct name of the fixture is a kernel symbol of the built library."""
    from centermask2_amd import _lib
    names = {r["kernel"] for r in _cases()["rows"] if "kernel" in r}
    syms = subprocess.run("nm -C --defined-only '{}'".format(_lib.LIB_PATH), shell=True, check=True, capture_output=True, text=True).stdout
    kernels = {line.split("cmk::", 1)[1].split("(")[0] for line in syms.splitlines() if " cmk::conv_" in line and "_kernel<" in line}
    assert len(names) >= 40 and names <= kernels, sorted(names - kernels)


def test_plan_arguments_and_the_records_entry_point():
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    p = dict(k=3, stride=1, cin=64, cout=64, x_cs=64, y_cs=64, res=0, shapes=[[8, 50, 80], [8, 25, 40]])
    descs = _descs(_lib, ptr, p, (6, 16, 1), 0, 32, gn_ws=False)
    assert lib.cmk_conv_plan(descs, 2, None, 0, None, None) == 0                    # every output is optional
    short = ctypes.create_string_buffer(8)
    assert lib.cmk_conv_plan(descs, 2, short, len(short), None, None) == 0 and short.value == b"conv_wi"
    got = _plan(lib, descs)
    assert got["gn_records"] == [lib.cmk_conv_gn_records(50, 80, 6), lib.cmk_conv_gn_records(25, 40, 6)] == [4 * 5 * 2, 4 * 3 * 1]
    got5 = _plan(lib, _descs(_lib, ptr, p, (5, 16, 2), 0, 32, gn_ws=False))
    assert got5["gn_records"] == [lib.cmk_conv_gn_records(50, 80, 5), lib.cmk_conv_gn_records(25, 40, 5)] == [2 * 7 * 5, 2 * 4 * 3]
    # untuned descriptors resolve as in a launch (cmk_conv_resolve), with and without statistics
    v = (ctypes.c_int * 3)()
    for groups in (0, 32):
        d0 = _descs(_lib, ptr, p, (0, 0, 0), 0, groups, gn_ws=False)
        assert lib.cmk_conv_resolve(d0, 2, int(groups > 0), v) == 0
        assert _plan(lib, d0) == _plan(lib, _descs(_lib, ptr, p, tuple(v), 0, groups, gn_ws=False))
    assert lib.cmk_conv_plan(None, 1, None, 0, None, None) == -1 and b"null" in lib.cmk_last_error()
    bad = _descs(_lib, ptr, dict(p, cin=24, x_cs=24), (6, 16, 1), 0, 0, gn_ws=False)
    assert lib.cmk_conv_plan(bad, 2, None, 0, None, None) == -1 and b"multiple of 16" in lib.cmk_last_error()
