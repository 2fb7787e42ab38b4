"""-m gpu: conv2d, conv2d_multi, conv_gn_multi and conv_gn_multi_pair still choose and launch what they did.  The kernel name and executed
FLOPs they record in ops.PROFILE equal cmk_conv_plan's answer for descriptors filled by hand on dummy pointers (conv_cases.fill_descs: no
field comes through ops._fill_desc or the launch path under test); the outputs, GroupNorm affines and pooled means meet the float64 bars of
tests/test_gpu_conv_conformance.py; a launch of several problems gives the bits of the same convs run one at a time through conv2d."""
import ctypes

import pytest
import torch

from centermask2_amd import _lib, ops
from tests import conv_cases as cc
from tests.test_cpu_conv_plan import _plan
from tests.test_gpu_conv_conformance import _check_output, _device_buffers, _fp32_bar

pytestmark = pytest.mark.gpu

LEVELS = [(1, 12, 40), (1, 7, 10)]
WHAT = "conv wrappers"


def _planned(lib, c):
    got = _plan(lib, cc.fill_descs(c, _lib, ptr=4096))
    return got["kernel"], got["flops"]


def _set_up(c, dev, monkeypatch, forced):
    """No table, no tuner, FORCE_VARIANT = forced, a fresh PROFILE list; the case's tensors on the device and its float64 answers."""
    for name, value in (("_TUNED", {}), ("AUTOTUNE", False), ("FORCE_VARIANT", forced), ("PROFILE", [])):
        monkeypatch.setattr(ops, name, value)
    t = cc.host_tensors(c)
    return t, _device_buffers(c, t, dev), cc.reference(c, t), ops.PROFILE


def test_conv2d_launches_the_planned_kernel(dev, cmk_lib, monkeypatch):
    c = cc.case(k=1, shapes=[(1, 16, 16)], cin=32, cout=256, tv=(0, 0, 0))
    t, b, ref, profile = _set_up(c, dev, monkeypatch, None)
    pool = []
    ops.conv2d(b["xv"][0], b["pcs"][0], b["yv"][0], relu=True, pool=pool)
    torch.cuda.synchronize()
    descs, v = cc.fill_descs(c, _lib, ptr=4096), (ctypes.c_int * 3)()
    assert cmk_lib.cmk_conv_resolve(descs, 1, 0, v) == 0
    descs[0].tune_wm, descs[0].tune_sc, descs[0].tune_wn = v
    rows = cmk_lib.cmk_conv_pool_rows(ctypes.byref(descs[0]))          # the pooled sums are on offer exactly where the chosen kernel has them
    assert len(pool) == (1 if rows > 0 else 0)
    assert len(profile) == 1 and (profile[0][0], profile[0][6]) == _planned(cmk_lib, dict(c, tv=tuple(v), pool=rows > 0))
    assert profile[0][5] == (1, 16, 16, 32, 256, 1, 1)
    _check_output(c, b, ref, WHAT)
    if pool:
        want = cc.reference(dict(c, pool=True), t)["pool"][0]
        assert pool[0][1] == rows
        _fp32_bar(pool[0][0].double().cpu().sum(0)[None] / 256.0 - want, want, 1e-5, WHAT + " pooled means")


@pytest.mark.parametrize("forced", [None, (6, 16, 1), (6, 16, 1, 4)], ids=["untuned", "6-16-1", "6-16-1-splitk4"])
def test_multi_wrappers_launch_the_planned_kernel(dev, cmk_lib, monkeypatch, forced):
    pair_case = cc.case(shapes=LEVELS + LEVELS, cin=32, cout=64, tv=forced or (0, 0, 0), relu_upto=0, weight_sets=2, gn_groups=32)
    tower = dict(pair_case, shapes=LEVELS, weight_sets=1)
    t, b, ref, profile = _set_up(pair_case, dev, monkeypatch, forced)
    xs, pcs = b["xv"], b["pcs"]
    gns = [tuple(v.to(dev) for v in gn) for gn in t["gn"]]
    multi = lambda: ops.conv2d_multi(xs[:2], pcs[:2], b["yv"][:2])
    gn_multi = lambda: ops.conv_gn_multi(xs[:2], pcs[:2], gns[0][0], gns[0][1], 32, 1e-5)
    pair = lambda: ops.conv_gn_multi_pair(xs[:2], pcs[0], gns[0], xs[2:], pcs[2], gns[1], 32, 1e-5)
    if forced is not None and len(forced) > 3:
        for call in (multi, gn_multi):         # split-K: the library takes it for one problem only ...
            with pytest.raises(_lib.CmkError):
                call()
        assert pair() is None and profile == []          # ... and the pair hands such a variant back to its caller, as its docstring says
        return

    def check(ys, affs, planned_case):
        assert len(profile) == 1 and (profile[0][0], profile[0][6]) == _planned(cmk_lib, planned_case) and profile[0][5] is None
        del profile[:]
        torch.cuda.synchronize()
        for i, y in enumerate(ys):
            _fp32_bar(y.t.double().cpu() - ref["y"][i], ref["y"][i], 2e-4, WHAT)
        for (sc, sh), (ref_sc, ref_sh) in zip(affs, ref["gn"]):
            _fp32_bar(sc.double().cpu() - ref_sc, ref_sc, 1e-4, WHAT + " GroupNorm scale")
            _fp32_bar(sh.double().cpu() - ref_sh, ref_sh, 1e-4, WHAT + " GroupNorm shift")

    multi()
    check(b["yv"][:2], [], dict(tower, gn_groups=0))
    ys_gn, affs = gn_multi()
    check(ys_gn, affs, tower)
    both = pair()
    if forced is None:
        # the library's own choice for these two small levels is no F(4x4) map kernel: one weight pointer per launch, so no pair
        assert not _planned(cmk_lib, tower)[0].startswith("conv_wino6") and both is None and profile == []
        return
    assert both is not None
    check(both[0][0] + both[1][0], both[0][1] + both[1][1], pair_case)
    singles = [ops.conv_out(x, pc) for x, pc in zip(xs, pcs)]
    torch.cuda.synchronize()
    for i, (single, y) in enumerate(zip(singles, both[0][0] + both[1][0])):
        assert torch.equal(y.t, single.t), i
        assert i >= 2 or (torch.equal(b["yv"][i].t, single.t) and torch.equal(ys_gn[i].t, single.t)), i
