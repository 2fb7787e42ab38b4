"""-m gpu: every case of the conv conformance table (tests/conv_cases.py) through the C ABI on real buffers, one test id per family.

An accepted case is launched (cmk_conv2d_nhwc for one problem, cmk_conv2d_nhwc_multi otherwise; descriptors from ops._fill_desc and
ops._set_variant, through conv_cases.fill_descs) and checked for: the output against a float64 reference at the bar the family already holds in its own tests; nothing
written outside the output view (the view lies in a NaN-filled tensor that is itself the middle images of a NaN-filled allocation with one
guard image before and one after); input, residual, weights and epilogue vectors bit-unchanged; a second launch giving the same bits;
cmk_conv_plan agreeing with the launch.  A refused case must return non-zero with an error text and leave the NaN-filled output and every
workspace handed in NaN: nothing was launched before the refusal.  Inputs are finite (the kernels' ReLU maps a NaN to 0, groupnorm.hip).

Bars (none is new): the fp32 and Winograd families max abs err <= min(1e-3, 2e-4 * max(1, max|ref|)) (test_gpu_backbone_ops._close); the
split GEMM forms tune_wm 10 / 12 2e-5 absolute; the direct split form tune_wm 11 1e-5 * max|ref| per image with a zero shift; GroupNorm
{scale, shift} from the records min(1e-3, 1e-4 * max(1, max|ref|)) on the Winograd forms (test_conv_with_fused_groupnorm_statistics) and 2e-3
of max|ref| (shift: of max(1, max|ref|)) on tune_wm 11 (test_conv_direct_split_tower_launches); pooled means min(1e-3, 1e-5 * max(1,
max|ref|)) (test_conv_pointwise_pooled_sums_and_ese_gate).

Observed on an MI355X (the run's error report has them per family): relative to max(1, max|ref|) igemm 1x1 4.2e-7, 3x3 stride 1 1.2e-6,
stride 2 9.2e-7, gather 9.0e-7, pw 4.5e-7, pw gather 1.3e-6, wino4r 3.5e-7, the six F(4x4) forms 5.5e-6 .. 7.8e-6; tune_wm 10 7.8e-6 and
tune_wm 12 4.5e-6 absolute; tune_wm 11 7.5e-7 of the image's magnitude; GroupNorm scale / shift below 5.4e-7; pooled means below 1.1e-7.
Census rows write a dense output between the guard images, feature rows a channel slice of a wider tensor."""
import pytest
import torch

from centermask2_amd import _lib, ops
from centermask2_amd.ops import View
from tests import conformance as C
from tests import conv_cases as cc
from tests.helpers import close, close_abs, relaunch

pytestmark = pytest.mark.gpu

NAN = float("nan")
PACKINGS = ("w", "w_wino", "w_wino6", "w_split", "w_splith", "scale", "shift")


def _device_buffers(c, t, dev):
    """The tensors of a case on the device.  y: the images 1..N of a NaN-filled allocation of N + 2 (guard images); same_buffer: x and y in
    that one allocation, every channel outside the output view finite."""
    (x_cs, x_co), (y_cs, y_co) = cc.views_of(c)
    b = {"xa": [], "ya": [], "xv": [], "yv": [], "pcs": [], "res": [], "aff": []}
    base = [ops.PackedConv(w, None, None, dev, stride=c["stride"]) for w in t["w"]]
    for i, (n, h, w) in enumerate(c["shapes"]):
        ho, wo = cc.out_hw(c, h, w)
        if c["same_buffer"]:
            alloc = torch.full((n + 2, h, w, x_cs), NAN, device=dev)
            alloc[1:n + 1] = t["x"][i].to(dev)
            alloc[1:n + 1, :, :, y_co:y_co + c["cout"]] = NAN
            xa = ya = alloc
            xv, yv = View(alloc[1:n + 1], x_co, c["cin"]), View(alloc[1:n + 1], y_co, c["cout"])
        else:
            xa = t["x"][i].to(dev)
            ya = torch.full((n + 2, ho, wo, y_cs), NAN, device=dev)
            xv, yv = View(xa, x_co, c["cin"]), View(ya[1:n + 1], y_co, c["cout"])
        pc = ops.PackedConv.__new__(ops.PackedConv)
        pc.__dict__.update(base[cc.weight_set(c, i)].__dict__)
        pc.scale, pc.shift = t["scale"][i].to(dev), t["shift"][i].to(dev)
        b["xa"].append(xa); b["ya"].append(ya); b["xv"].append(xv); b["yv"].append(yv); b["pcs"].append(pc)
        b["res"].append(t["res"][i].to(dev) if c["res_mode"] else None)
        b["aff"].append(tuple(v.to(dev) for v in t["aff"][i]) if c["in_affine"] else None)
    return b


def _read_only(c, b):
    """Everything a launch may only read, by name."""
    ro = {}
    for i in range(len(c["shapes"])):
        if not c["same_buffer"]:
            ro["x{}".format(i)] = b["xa"][i]
        if b["res"][i] is not None:
            ro["res{}".format(i)] = b["res"][i]
        if b["aff"][i] is not None:
            ro["in_scale{}".format(i)], ro["in_shift{}".format(i)] = b["aff"][i]
        for name in PACKINGS:
            v = getattr(b["pcs"][i], name, None)
            if v is not None:
                ro["{}{}".format(name, i)] = v
    return ro


def _all_nan(t):
    return t is None or bool(torch.isnan(t).all())


def _launch(lib, descs):
    rc = relaunch(descs)
    return rc, lib.cmk_last_error().decode() if rc != 0 else ""


def _fp32_bar(diff, ref, rel, what):
    """max abs err <= min(1e-3, rel * max(1, max|ref|)), both halves on record."""
    zero = torch.zeros_like(diff)
    close(diff / max(1.0, float(ref.abs().max())), zero, rel, what)
    close_abs(diff, zero, 1e-3, what)


def _check_output(c, b, ref, what):
    wm = c["tv"][0]
    (_, _), (_, y_co) = cc.views_of(c)
    for i, (n, _, _) in enumerate(c["shapes"]):
        got = b["yv"][i].t[..., y_co:y_co + c["cout"]].double().cpu()
        want = ref["y"][i]
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), (c["id"], i, "the output view is not written everywhere")
        diff = got - want
        if wm in (10, 12):
            close_abs(diff, torch.zeros_like(diff), 2e-5, what)
        elif wm == 11:
            for j in range(n):                    # per image, relative to that image's own output magnitude
                mag = float(want[j].abs().max())
                if mag == 0.0:
                    assert float(diff[j].abs().max()) == 0.0, (c["id"], i, j)
                else:
                    close_abs(diff[j] / mag, torch.zeros_like(diff[j]), 1e-5, what)
        else:
            _fp32_bar(diff, want, 2e-4, what)


def _check_outside(c, b, before):
    """Guard images and the channels beside the output view: NaN as before (same_buffer: the finite channels bit-unchanged)."""
    (_, _), (_, y_co) = cc.views_of(c)
    for i, (n, _, _) in enumerate(c["shapes"]):
        ya = b["ya"][i]
        assert _all_nan(ya[0]) and _all_nan(ya[n + 1]), (c["id"], i, "a guard image was written")
        left, right = ya[1:n + 1, :, :, :y_co], ya[1:n + 1, :, :, y_co + c["cout"]:]
        if c["same_buffer"]:
            old = before["same{}".format(i)]
            assert C.same_bits(left.contiguous(), old[..., :y_co].contiguous()) and C.same_bits(right.contiguous(), old[..., y_co + c["cout"]:].contiguous()), \
                (c["id"], i, "channels outside the output view changed")
        else:
            assert _all_nan(left) and _all_nan(right), (c["id"], i, "written outside the output view")


def _check_records(c, b, keep, ref, t, dev, what):
    wm = c["tv"][0]
    if c["gn_groups"]:
        assert keep["affine"] is not None, (c["id"], "the kernel is declared to write GroupNorm records and the plan offers none")
        n = len(c["shapes"])
        half = n // 2 if c["weight_sets"] == 2 else n
        got = []
        for s in range(c["weight_sets"]):
            gamma, beta = (v.to(dev) for v in t["gn"][s])
            got += keep["affine"](s * half, (s + 1) * half, gamma, beta, 1e-5)
        torch.cuda.synchronize()
        for (sc, sh), (ref_sc, ref_sh) in zip(got, ref["gn"]):
            d_sc, d_sh = sc.double().cpu() - ref_sc, sh.double().cpu() - ref_sh
            if wm == 11:
                close_abs(d_sc / float(ref_sc.abs().max()), torch.zeros_like(d_sc), 2e-3, what + " GroupNorm scale")
                close_abs(d_sh / max(1.0, float(ref_sh.abs().max())), torch.zeros_like(d_sh), 2e-3, what + " GroupNorm shift")
            else:
                _fp32_bar(d_sc, ref_sc, 1e-4, what + " GroupNorm scale")
                _fp32_bar(d_sh, ref_sh, 1e-4, what + " GroupNorm shift")
    if c["pool"]:
        pws, rows = keep["pool"].double().cpu(), keep["rows"]
        assert bool(torch.isfinite(pws).all()), (c["id"], "a pooled record was not written")
        n, h, w = c["shapes"][0]
        sums = torch.zeros((n + 1, c["cout"]), dtype=torch.float64)
        for g in range(pws.shape[0] // 2):       # record 2g: the rows of block g in the image of its first pixel; 2g + 1: those in the next image
            img = (g * rows) // (h * w)
            sums[img] += pws[2 * g]
            sums[img + 1] += pws[2 * g + 1]
        assert float(sums[n].abs().max()) == 0.0
        want = ref["pool"][0]
        _fp32_bar(sums[:n] / (h * w) - want, want, 1e-5, what + " pooled means")


def _run_case(c, seed, dev, lib, what, skipped):
    t = cc.host_tensors(c, seed)
    b = _device_buffers(c, t, dev)
    descs, keep = cc.fill_descs(c, _lib, bufs=b, ops=ops)
    n = len(descs)
    ro = _read_only(c, b)
    before = {k: v.clone() for k, v in ro.items()}
    if c["same_buffer"]:
        for i, (ni, _, _) in enumerate(c["shapes"]):
            before["same{}".format(i)] = b["ya"][i][1:ni + 1].clone()
    rc, err = _launch(lib, descs)
    planned = lib.cmk_conv_plan(descs, n, None, 0, None, None)
    if rc != 0 and "hipFuncSetAttribute failed" in err and c["tv"][:2] == (6, 32):
        skipped.append(c["id"])                   # the paired form on a device whose LDS limit is below its 160 KiB workgroup
        return "skipped"
    assert (planned == 0) == (rc == 0), (c["id"], "plan and launch disagree", planned, rc, err)
    if c["answer"] == "refuse":
        assert rc != 0 and err.strip(), (c["id"], "declared refuse, launched", rc)
        for i in range(n):
            if not c["same_buffer"]:
                assert _all_nan(b["ya"][i]), (c["id"], "the output was written before the refusal")
        assert _all_nan(keep["ws"]) and _all_nan(keep["pool"]) and _all_nan(keep["gn"]), (c["id"], "a workspace was written before the refusal")
        for k, v in ro.items():
            assert C.same_bits(v, before[k]), (c["id"], k, "changed by a refused launch")
        return "refused"
    assert rc == 0, (c["id"], "declared accept, refused", err)
    ref = cc.reference(c, t)
    _check_output(c, b, ref, what)
    _check_outside(c, b, before)
    _check_records(c, b, keep, ref, t, dev, what)
    for k, v in ro.items():
        assert C.same_bits(v, before[k]), (c["id"], k, "an input of the launch changed")
    # determinism: the same launch into a NaN output again
    (_, _), (_, y_co) = cc.views_of(c)
    first = [b["yv"][i].t[..., y_co:y_co + c["cout"]].clone() for i in range(n)]
    first_pool = keep["pool"].clone() if keep["pool"] is not None else None
    for i in range(n):
        b["yv"][i].t[..., y_co:y_co + c["cout"]] = NAN
    for ws in (keep["ws"], keep["pool"]):
        if ws is not None:
            ws.fill_(NAN)
    rc2, err2 = _launch(lib, descs)
    assert rc2 == 0, (c["id"], err2)
    for i in range(n):
        assert C.same_bits(b["yv"][i].t[..., y_co:y_co + c["cout"]].contiguous(), first[i].contiguous()), (c["id"], i, "a second launch gave other bits")
    if first_pool is not None:
        assert C.same_bits(keep["pool"], first_pool), (c["id"], "a second launch gave other pooled sums")
    return "launched"


CASES = cc.all_cases()


@pytest.mark.parametrize("family", list(cc.FAMILIES))
def test_conv_conformance(dev, cmk_lib, family, monkeypatch):
    monkeypatch.setattr(ops, "ALLOW_SPLIT_BF16", True)
    monkeypatch.setattr(ops, "ALLOW_SPLIT_F16", True)
    monkeypatch.setattr(ops, "FORCE_VARIANT", None)
    mine = [(i, c) for i, c in enumerate(CASES) if c["family"] == family]
    seed = {c["id"]: i for i, c in mine}
    skipped = []
    how = C.run_rows([c for _, c in mine], lambda c: _run_case(c, seed[c["id"]], dev, cmk_lib, "conformance " + family, skipped))
    done = {k: how.count(k) for k in ("launched", "refused", "skipped")}
    if skipped:
        print("skipped (the device's LDS limit refuses the paired form):", skipped)
    # nothing skips silently: every declared case ran, and was answered as declared
    assert done["launched"] + done["skipped"] == sum(c["answer"] == "accept" for _, c in mine) and done["launched"] > 0
    assert done["refused"] == sum(c["answer"] == "refuse" for _, c in mine)
    assert not skipped or family.startswith("wino6p")


def test_conformance_covers_the_whole_table():
    """The per-family test ids above partition the table: no case belongs to a family without an id."""
    assert {c["family"] for c in CASES} == set(cc.FAMILIES)
