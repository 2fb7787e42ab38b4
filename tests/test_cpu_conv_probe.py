"""tools/conv_probe.py: its shape table against the library's front door and the shipped tuned tables, `plan` against the plan golden of
tests/test_cpu_conv_plan.py, the variant spelling, and the fault discipline of the --lib driver on children that open no GPU.  The tests
marked gpu run the tool in-process at the conformance table's smallest shapes, at the bar tests/test_gpu_conv_conformance.py holds."""
import glob
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_probe", os.path.join(ROOT, "tools", "conv_probe.py"))      # tools/ is no package and stays off sys.path
cp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cp)


def _key(p):
    return (p.k, p.stride, (p.cin + 15) // 16 * 16, p.cout, tuple(tuple(s) for s in p.shapes))


def test_shape_table():
    from centermask2_amd import ops
    names = [r[0] for r in cp.SHAPES]
    assert len(set(names)) == len(names)
    assert len({r[1:8] for r in cp.SHAPES}) == len(cp.SHAPES), "one problem under two names"
    assert {"v39", "v99", "pw", "s2", "roi", "single", "small", "tower"} <= set(cp.SETS) and all(cp.rows([s]) for s in cp.SETS)
    tower, = cp.rows(["tower"])
    assert tower.shapes == ((8, 100, 160), (8, 50, 80), (8, 25, 40), (8, 13, 20), (8, 7, 10))
    status, planned = cp.main(["plan", "--set", "tower", "--row"] + names + ["-v", "default"])        # the library's validate, through plan
    assert status == 0 and len(planned) == len(cp.SHAPES) + 1 and not [r for r in planned if "refused" in r]
    have = {_key(p) for p in cp.rows(cp.SETS)}
    seen = 0
    for path in glob.glob(os.path.join(ROOT, "centermask2_amd", "tuned", "*V-39*.json")):
        with open(path) as f:
            for key in json.load(f):
                k, stride, cin, cout, _, _, _, shapes = ops._str_to_key(key)
                if len(shapes) == 1 and (k, stride) in ((3, 1), (1, 1)):
                    assert (k, stride, cin, cout, shapes) in have, key
                    seen += 1
    assert seen >= 50


def test_plan_gives_the_golden_kernels_and_the_refusal_text():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan_cases.json")) as f:
        golden = json.load(f)
    table = {_key(p): p.name for p in cp.rows(cp.SETS) if len(p.shapes) == 1}
    checked = 0
    for row in golden["rows"]:
        p = golden["problems"][row["problem"]]
        name = table.get((p["k"], p["stride"], p["cin"], p["cout"], tuple(tuple(s) for s in p["shapes"])))
        if name is None or (p["x_cs"], p["y_cs"], p["res"], row["pool"], row["groups"]) != (p["cin"], p["cout"], 0, 0, 0) or "kernel" not in row:
            continue
        _, got = cp.main(["plan", "--row", name, "-v"] + [cp.spell(tv) for tv in row["tvs"]])
        assert [(r["kernel"], r["flops"]) for r in got] == [(row["kernel"], row["flops"])] * len(row["tvs"]), (name, row)
        checked += len(got)
    assert checked >= 20
    _, got = cp.main(["plan", "--row", "OSA2_cat", "fpn_lat3", "-v", "9/32/2", "tuned"])
    assert [r.get("refused") for r in got] == ["conv: pointwise gather variant not available for this conv", None, got[2]["refused"], "no entry in the table"]
    _, (gn,) = cp.main(["plan", "--set", "tower", "--gn", "32", "--in-affine", "-v", "tuned"])
    assert gn["kernel"] == "conv_wino6p_kernel<true, 0>" and gn["gn_records"] == [144, 40, 12, 8, 4]


def test_variant_spelling_round_trips():
    from centermask2_amd.ops import Variant
    roi, = cp.rows([], ["roi"])
    osa, = cp.rows([], ["OSA2_x"])
    for tv in ((1, 16, 2), (6, 32, 2, 1, 8), (0, 0, 0, 2), (7, 32, 4, 4), (11, 21, 0), (6, 16, 1, 1, 1)):
        assert cp.parse_variant(cp.spell(tv), osa) == Variant.of(tv) and cp.spell(cp.parse_variant(cp.spell(tv), osa)) == cp.spell(tv)
    assert cp.spell((6, 16, 1, 1)) == "6/16/1" and cp.spell((6, 16, 1, 2, 0)) == "6/16/1/2"
    assert cp.parse_variant("default", osa) == Variant(0, 0, 0)
    assert cp.parse_variant("6/64/roi", roi) == Variant(6, 64, 2) and cp.parse_variant("6/64/roi", osa) == Variant(6, 64, 1)
    with pytest.raises(SystemExit):
        cp.parse_variant("6/16", osa)


OK_CHILD = "import sys; open(sys.argv[1], 'a').write('x'); print('RESULT {\"a\": [1.5, null], \"b\": [%s, 2.0]}' % sys.argv[2])"
BAD_CHILD = {"segv": "import sys, os; open(sys.argv[1], 'a').write('x'); os._exit(139)",
             "late": "import sys, time; open(sys.argv[1], 'a').write('x'); time.sleep(30)"}


@pytest.mark.parametrize("how", sorted(BAD_CHILD))
def test_lib_driver_stops_at_the_first_bad_child(how, tmp_path, capsys):
    starts = str(tmp_path / "starts")
    cmds = iter([[sys.executable, "-c", OK_CHILD, starts, "3.0"], [sys.executable, "-c", OK_CHILD, starts, "2.5"],
                 [sys.executable, "-c", BAD_CHILD[how], starts], [sys.executable, "-c", OK_CHILD, starts, "1.0"]])
    status, times = cp.ab(["A.so", "B.so"], 2, lambda lib: next(cmds), 1.0)
    assert status != 0 and len(open(starts).read()) == 3, "no child is started after the one that failed"
    assert times == {"A.so": {"a": [1.5, None], "b": [3.0, 2.0]}, "B.so": {"a": [1.5, None], "b": [2.5, 2.0]}}
    out = capsys.readouterr().out
    assert "no further child is started" in out and ("exit status 139" if how == "segv" else "killed") in out
    assert "A.so" in out and "b 3.000/2.000" in out and "b 2.500/2.000" in out          # what was gathered is printed


def test_lib_driver_takes_the_best_of_rounds(tmp_path):
    starts = str(tmp_path / "starts")
    cmds = iter([[sys.executable, "-c", OK_CHILD, starts, v] for v in ("3.0", "2.5", "2.0", "4.0")])
    status, times = cp.ab(["A.so", "B.so"], 2, lambda lib: next(cmds), 30.0)
    assert status == 0 and times["A.so"]["b"] == [2.0, 2.0] and times["B.so"]["b"] == [2.5, 2.0] and len(open(starts).read()) == 4


# ---------------------------------------------------------------------------------------------------------------
# -m gpu: the tool in-process
# ---------------------------------------------------------------------------------------------------------------
SMALL = "2,13,41,48,80,3,1"            # tests/conv_cases.py: the Winograd families' own small problem


def _within_the_bar(row, what):
    from tests.test_gpu_conv_conformance import _fp32_bar
    assert "refused" not in row and row["unwritten"] == 0, row
    for diff, ref in zip(row["diff"], row["ref"]):
        _fp32_bar(diff, ref, 2e-4, what)


@pytest.mark.gpu
def test_time_and_check_on_the_small_3x3_problem(dev):
    import torch
    from tests import conv_cases as cc
    assert cc.FAMILIES["wino6 map tiles"]["shapes"] == [(2, 13, 41)] and (cc.FAMILIES["wino6 map tiles"]["cin"], cc.FAMILIES["wino6 map tiles"]["cout"]) == (48, 80)
    # 1/16/2 does not tile Cout 80 (the padded Cout, 96, is no multiple of 64): the library refuses it and the tool says n/a; 1/16/3 is the
    # direct variant the conformance table itself runs on this problem
    variants = ["1/16/3", "1/16/2", "5/16/2", "6/16/1"]
    status, (row,) = cp.main(["time", "--shape", SMALL, "--rounds", "1", "--iters", "2", "-v"] + variants, keep=True)
    assert status == 0 and row["refused"] == [None, "conv: variant not available for this shape", None, None]
    assert row["ms"][1] is None and all(ms > 0 for k, ms in enumerate(row["ms"]) if k != 1)
    assert row["equal"][0] is True and row["maxdiff"][0] == 0.0 and row["equal"][1] is None
    assert row["outputs"][1] is None
    for k in (0, 2, 3):
        assert row["equal"][k] == all(torch.equal(y, y0) for y, y0 in zip(row["outputs"][k], row["outputs"][0]))
    status, checked = cp.main(["check", "--shape", SMALL, "--reps", "2", "-v"] + variants, keep=True)
    assert status == 0 and len(checked) == 4 and checked[1].get("refused") == "conv: variant not available for this shape"
    for r in checked[:1] + checked[2:]:
        assert r["reps_equal"] is True
        _within_the_bar(r, "conv_probe check " + r["variant"])


@pytest.mark.gpu
@pytest.mark.parametrize("res", [[], ["--res", "add"]], ids=["plain", "res"])
def test_check_split_k_pointwise(dev, res):
    status, (row,) = cp.main(["check", "--shape", "1,1,400,1024,80,1,1", "--relu", "-v", "0/0/0/2"] + res, keep=True)
    assert status == 0
    _within_the_bar(row, "conv_probe check split-K 1x1")


@pytest.mark.gpu
def test_two_level_launch_with_groupnorm_is_bit_equal_between_the_f4x4_forms(dev):
    status, (row,) = cp.main(["time", "--shape", "2,13,20,256,256,3,1", "--levels", "13x20,7x10", "--gn", "32", "--in-affine", "--rounds", "1", "--iters", "2",
                              "-v", "6/16/1", "6/64/1"], keep=True)
    assert status == 0 and row["refused"] == [None, None]
    assert row["equal"] == [True, True] and row["affines_equal"] == [True, True]
