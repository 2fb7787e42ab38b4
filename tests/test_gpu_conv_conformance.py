"""-m gpu: every case of the conv conformance table (tests/conv_cases.py) through the C ABI on real buffers, one test id per family.

An accepted case is launched (cmk_conv2d_nhwc for one problem, cmk_conv2d_nhwc_multi otherwise; descriptors from ops._fill_desc and
ops._set_variant, through conv_cases.fill_descs) and checked for: the output against a float64 reference at the bar the family already holds in its own tests; nothing
written outside the output view (the view lies in a NaN-filled tensor that is itself the middle images of a NaN-filled allocation with one
guard image before and one after); input, residual, weights and epilogue vectors bit-unchanged; a second launch giving the same bits;
cmk_conv_plan agreeing with the launch.  A refused case must return non-zero with an error text and leave the NaN-filled output and every
workspace handed in NaN: nothing was launched before the refusal.  The values a row reads are finite (the kernels' ReLU maps a NaN to 0,
groupnorm.hip), but nothing around them is: x and the residual lie between NaN guard images like the output, the channels beside their
views are NaN (same_buffer: the channels of neither x nor y), so a finite output means that none of it was read into a product; and the
second launch runs after all of that was refilled with the byte 0xC3 and must give the same bits.

Value rows (conv_cases.VALUE_FEATURES; regimes, emulations and bars in tests/conv_values.py): ints and pow2_channels are compared with
torch.equal / same_bits wherever the table claims exactness, the all-zero image of sparse too; cancel, sparse, f16_domain and the cells of
conv_cases.HELD_TO_BAR at 4x the CPU emulation's own distance from float64 on the row's tensors; nonfinite by the bits of its clean launch
outside the poisoned pixel's reach, in every other image and problem and in their pooled sums and GroupNorm {scale, shift}.

Bars (none is new): the fp32 and Winograd families max abs err <= min(1e-3, 2e-4 * max(1, max|ref|)) (test_gpu_backbone_ops._close); the
split GEMM forms tune_wm 10 / 12 2e-5 absolute; the direct split form tune_wm 11 1e-5 * max|ref| per image with a zero shift; GroupNorm
{scale, shift} from the records min(1e-3, 1e-4 * max(1, max|ref|)) on the Winograd forms (test_conv_with_fused_groupnorm_statistics) and 2e-3
of max|ref| (shift: of max(1, max|ref|)) on tune_wm 11 (test_conv_direct_split_tower_launches); pooled means min(1e-3, 1e-5 * max(1,
max|ref|)) (test_conv_pointwise_pooled_sums_and_ese_gate).

Observed on an MI355X (the run's error report has them per family): relative to max(1, max|ref|) igemm 1x1 4.2e-7, 3x3 stride 1 1.2e-6,
stride 2 9.2e-7, gather 9.0e-7, pw 4.5e-7, pw gather 1.3e-6, wino4r 3.5e-7, the six F(4x4) forms 5.5e-6 .. 7.8e-6; tune_wm 10 7.8e-6 and
tune_wm 12 4.5e-6 absolute; tune_wm 11 7.5e-7 of the image's magnitude; GroupNorm scale / shift below 5.4e-7; pooled means below 1.1e-7.
Census rows write a dense output between the guard images, feature rows a channel slice of a wider tensor.

Value rows observed on an MI355X (the run prints kernel, emulation and bar per row; cancel and f16_domain relative to max|ref|, the others
to max(1, max|ref|)); every exact cell was exact, the 16-bit-MFMA families (tune_wm 10, 11, 12) on ints included, and every nonfinite row
kept the clean launch's bits outside the reach:
  family               ints      pow2      cancel    sparse    f16 a     f16 b
  igemm 1x1            exact     bits      5.4e-7    1.2e-7
  igemm 3x3 stride 1   exact     bits      7.8e-7    5.0e-7
  igemm 3x3 stride 2   exact     bits      5.8e-7    5.0e-7
  gather (wm 7)        exact     bits      8.4e-7    5.6e-7
  pw (wm 8)            exact     bits      8.3e-7    2.5e-7
  pw gather (wm 9)     exact     bits      6.0e-7    7.1e-7
  pw split bf16 (10)   exact     bits      4.1e-7    2.6e-7
  pw split fp16 (12)   exact     2.7e-7    2.9e-6    3.1e-7    1.9e-7    2.1e-7
  wino4r (wm 5)        exact     bits      2.2e-6    2.1e-7
  wino6 map tiles      3.4e-6    bits      2.9e-6    3.2e-6
  wino6 RoI pairs      4.1e-6    bits      3.0e-6    4.1e-6
  wino6p map tiles     4.6e-6    bits      2.5e-6    3.4e-6
  wino6p RoI pairs     3.3e-6    bits      3.3e-6    3.6e-6
  wino6s map tiles     5.6e-6    bits      2.7e-6    3.9e-6
  wino6s RoI pairs     5.1e-6    bits      2.6e-6    2.3e-6
  sp3 (sc 2)           exact     5.6e-7    5.0e-5    3.9e-7    3.8e-7    3.7e-7
  sp3 (sc 21)          exact     4.1e-7    4.1e-5    4.4e-7    4.2e-7    4.0e-7
The emulations' own distances on the same rows are 0.6x to 3.5x these (the bars 4x that): cancel 3.9e-7 .. 5.8e-7 for the direct forms,
1.8e-6 F(2x2), 3.7e-6 .. 5.5e-6 F(4x4), 4.4e-7 tune_wm 10, 2.6e-6 tune_wm 12, 4.2e-5 tune_wm 11 (a zero-shift signal of 1.6e-2)."""
import pytest
import torch

from centermask2_amd import _lib, ops
from centermask2_amd.ops import View
from tests import conformance as C
from tests import conv_cases as cc
from tests import conv_values as cv
from tests import helpers
from tests.helpers import close, close_abs, relaunch

pytestmark = pytest.mark.gpu

NAN = float("nan")
PACKINGS = ("w", "w_wino", "w_wino6", "w_split", "w_splith", "scale", "shift")


def _guarded(data, co, ch, dev):
    """The channels [co, co + ch) of `data` (N, H, W, CS) as the images 1..N of a NaN-filled allocation of N + 2 images: guard images
    before and after, and NaN in every channel beside the slice."""
    n = data.shape[0]
    alloc = torch.full((n + 2,) + tuple(data.shape[1:]), NAN, device=dev)
    alloc[1:n + 1, :, :, co:co + ch] = data[..., co:co + ch].to(dev)
    return alloc


def _refill(alloc, n, co, ch, byte=0xC3):
    """Every guard image and every channel outside [co, co + ch) of a _guarded allocation gets another (finite) byte pattern."""
    kept = alloc[1:n + 1, :, :, co:co + ch].clone()
    alloc.view(torch.uint8).fill_(byte)
    alloc[1:n + 1, :, :, co:co + ch] = kept


def _device_buffers(c, t, dev):
    """The tensors of a case on the device.  x, y and the residual are each the images 1..N of a NaN-filled allocation of N + 2 (guard
    images) and NaN in every channel outside their view; same_buffer: x and y in that one allocation, NaN in the channels of neither."""
    (x_cs, x_co), (y_cs, y_co) = cc.views_of(c)
    b = {"xa": [], "ya": [], "xv": [], "yv": [], "pcs": [], "res": [], "ra": [], "aff": []}
    base = [ops.PackedConv(w, None, None, dev, stride=c["stride"]) for w in t["w"]]
    for i, (n, h, w) in enumerate(c["shapes"]):
        ho, wo = cc.out_hw(c, h, w)
        xa = _guarded(t["x"][i], x_co, c["cin"], dev)
        if c["same_buffer"]:
            ya = xa
        else:
            ya = torch.full((n + 2, ho, wo, y_cs), NAN, device=dev)
        xv, yv = View(xa[1:n + 1], x_co, c["cin"]), View(ya[1:n + 1], y_co, c["cout"])
        pc = ops.PackedConv.__new__(ops.PackedConv)
        pc.__dict__.update(base[cc.weight_set(c, i)].__dict__)
        pc.scale, pc.shift = t["scale"][i].to(dev), t["shift"][i].to(dev)
        b["xa"].append(xa); b["ya"].append(ya); b["xv"].append(xv); b["yv"].append(yv); b["pcs"].append(pc)
        ra = _guarded(t["res"][i], c["res_view"][1] if c["res_view"] else 0, c["cout"], dev) if c["res_mode"] else None
        b["ra"].append(ra)
        b["res"].append(ra[1:ra.shape[0] - 1] if ra is not None else None)
        b["aff"].append(tuple(v.to(dev) for v in t["aff"][i]) if c["in_affine"] else None)
    return b


def _refill_inputs(c, b):
    """The surroundings of every input (guard images, channels outside the views) refilled with the byte 0xC3: what a launch read of them
    shows as other output bits."""
    (_, x_co), _ = cc.views_of(c)
    for i, (n, _, _) in enumerate(c["shapes"]):
        _refill(b["xa"][i], n, x_co, c["cin"])       # same_buffer: the output view with it; the caller fills that with NaN again
        if b["ra"][i] is not None:
            _refill(b["ra"][i], n, c["res_view"][1] if c["res_view"] else 0, c["cout"])


def _read_only(c, b):
    """Everything a launch may only read, by name (x and the residual with their guards and outside channels)."""
    ro = {}
    for i in range(len(c["shapes"])):
        if not c["same_buffer"]:
            ro["x{}".format(i)] = b["xa"][i]
        if b["ra"][i] is not None:
            ro["res{}".format(i)] = b["ra"][i]
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
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), (c["id"], i, "the output view is not finite everywhere: {} of {} values".format(
            int((~torch.isfinite(got)).sum()), got.numel()))
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


def _gn_affine(c, keep, t, dev):
    """[(scale, shift)] per problem from the GroupNorm records of the launch."""
    assert keep["affine"] is not None, (c["id"], "the kernel is declared to write GroupNorm records and the plan offers none")
    n = len(c["shapes"])
    half = n // 2 if c["weight_sets"] == 2 else n
    got = []
    for s in range(c["weight_sets"]):
        gamma, beta = (v.to(dev) for v in t["gn"][s])
        got += keep["affine"](s * half, (s + 1) * half, gamma, beta, 1e-5)
    torch.cuda.synchronize()
    return got


def _check_records(c, b, keep, ref, t, dev, what):
    wm = c["tv"][0]
    if c["gn_groups"]:
        for (sc, sh), (ref_sc, ref_sh) in zip(_gn_affine(c, keep, t, dev), ref["gn"]):
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


def _one(c, t, dev, lib, skipped, again=True):
    """One launch of a case on the tensors t, with everything that does not depend on the values: plan and launch agree, a refusal touches
    nothing, an accepted launch writes nothing outside its output view and changes no input, and (again) a second launch gives the same
    bits after every guard image and outside channel of the inputs was refilled with 0xC3.  Returns "skipped" | "refused" | what the
    launch left: {"b", "keep", "y": [output view per problem, host], "pool", "gn": [(scale, shift) per problem] of a value row}."""
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
    _check_outside(c, b, before)
    for k, v in ro.items():
        assert C.same_bits(v, before[k]), (c["id"], k, "an input of the launch changed")
    (_, _), (_, y_co) = cc.views_of(c)
    first = [b["yv"][i].t[..., y_co:y_co + c["cout"]].clone() for i in range(n)]
    first_pool = keep["pool"].clone() if keep["pool"] is not None else None
    out = {"b": b, "keep": keep, "y": [f.cpu() for f in first], "pool": None if first_pool is None else first_pool.cpu(), "gn": None}
    if c["regime"] and c["gn_groups"]:
        out["gn"] = [(sc.cpu(), sh.cpu()) for sc, sh in _gn_affine(c, keep, t, dev)]
    if again:                                     # determinism, and nothing read of the inputs' surroundings: the same launch into a NaN output again
        _refill_inputs(c, b)
        for i in range(n):
            b["yv"][i].t[..., y_co:y_co + c["cout"]] = NAN
        for ws in (keep["ws"], keep["pool"]):
            if ws is not None:
                ws.fill_(NAN)
        rc2, err2 = _launch(lib, descs)
        assert rc2 == 0, (c["id"], err2)
        for i in range(n):
            assert C.same_bits(b["yv"][i].t[..., y_co:y_co + c["cout"]].contiguous(), first[i].contiguous()), \
                (c["id"], i, "a second launch, with 0xC3 around its inputs, gave other bits")
        if first_pool is not None:
            assert C.same_bits(keep["pool"], first_pool), (c["id"], "a second launch gave other pooled sums")
    return out


def _held_to_bar(c, t, y, what, label):
    """The outputs y of a value row's launch against float64 at the row's bar: 4x the emulation's own distance on these tensors."""
    ref = cc.reference(c, t)
    bar, own = cv.bar(c, t, ref)
    norm = cv.norm_of(c, torch.cat([r.reshape(-1) for r in ref["y"]]))
    err = 0.0
    for i, (got, want) in enumerate(zip(y, ref["y"])):
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), (c["id"], label, i, "{} outputs are not finite".format(int((~torch.isfinite(got)).sum())))
        err = max(err, float((got.double() - want).abs().max()))
    print("{} [{}]: {:.3e} (emulation {:.3e}, bar {:.3e}) of {:.3e}".format(c["id"], label, err / norm, own / norm, bar / norm, norm))
    helpers.OBSERVED["{} {} {} (of the row's norm)".format(what, c["feature"], label)] = err / norm
    assert err <= bar, "{} [{}]: max abs err {:.3e} > {:.3e}, 4x the emulation's {:.3e}".format(c["id"], label, err, bar, own)


def _records_by_image(c, out, p, j):
    """(the records of a launch that belong to the image j of problem p, all the others), each as a list of tensors."""
    mine, others = [], []
    if out["pool"] is not None:
        n, h, w = c["shapes"][0]
        rows = out["keep"]["rows"]
        for g in range(out["pool"].shape[0] // 2):           # record 2g: the image of block g's first pixel; 2g + 1: the next image
            img = (g * rows) // (h * w)
            for k, im in ((2 * g, img), (2 * g + 1, img + 1)):
                (mine if (0, im) == (p, j) else others).append(out["pool"][k])
    for i, pair in enumerate(out["gn"] or ()):
        for v in pair:
            for im in range(v.shape[0]):
                (mine if (i, im) == (p, j) else others).append(v[im])
    return mine, others


def _check_values(c, sets, outs, what):
    r = c["regime"]
    finite = lambda o: all(bool(torch.isfinite(y).all()) for y in o["y"])
    if r == "ints" and cv.exact_ints(c):
        ref = cc.reference(c, sets["row"])
        for i, (got, want) in enumerate(zip(outs["row"]["y"], ref["y"])):
            assert torch.equal(got.double(), want), "{}: integers are not exact, max abs err {:.3e}".format(c["id"], float((got.double() - want).abs().max()))
        print("{} [row]: equal to float64".format(c["id"]))
    elif r == "pow2_channels" and cv.exact_pow2(c):
        assert finite(outs["row"])
        for i, (got, want) in enumerate(zip(outs["row"]["y"], outs["plain"]["y"])):
            assert C.same_bits(got, want), "{}: per-channel powers of two changed the output, by {:.3e}".format(c["id"], float((got.double() - want.double()).abs().max()))
        print("{} [row]: the bits of the plain launch".format(c["id"]))
    elif r in ("ints", "pow2_channels", "cancel", "sparse"):
        _held_to_bar(c, sets["row"], outs["row"]["y"], what, "row")
        if r == "sparse":
            want = sets["row"]["shift"][-1].relu()
            got = outs["row"]["y"][-1][-1]
            assert torch.equal(got, want.expand_as(got)), (c["id"], "the all-zero image is not relu(shift)", float((got - want).abs().max()))
    elif r == "f16_domain":
        for label in ("a", "b"):
            _held_to_bar(c, sets[label], outs[label]["y"], what, label)
    elif r == "nonfinite":
        clean = outs["clean"]
        assert finite(clean) and (clean["pool"] is None or bool(torch.isfinite(clean["pool"]).all()))
        for label in ("inf", "nan"):
            p, j, py, px, _ = cv.poison_site(c, label)
            got, ref = outs[label], cc.reference(c, sets[label])
            for i, (n, h, w) in enumerate(c["shapes"]):
                for img in range(n):
                    g, cl = got["y"][i][img], clean["y"][i][img]
                    if (i, img) != (p, j):
                        assert C.same_bits(g, cl), (c["id"], label, "problem {} image {} changed with the {} in problem {} image {}".format(i, img, label, p, j))
                        continue
                    inside = cv.reach(c, h, w, py, px)
                    assert C.same_bits(g[~inside], cl[~inside]), (c["id"], label, "{} outputs outside the pixel's reach changed".format(
                        int((C.bits(g) != C.bits(cl))[~inside].sum())))
                    bad = ~torch.isfinite(ref["y"][i][img])
                    assert bool(bad.any()) and bool((~torch.isfinite(g))[bad].all()), (c["id"], label, "finite where float64 is not: {} of {}".format(
                        int(torch.isfinite(g)[bad].sum()), int(bad.sum())))
            mine, others = _records_by_image(c, got, p, j)
            for a, b_ in zip(others, _records_by_image(c, clean, p, j)[1]):
                assert C.same_bits(a, b_), (c["id"], label, "a record of another image changed")
            assert not mine or not all(bool(torch.isfinite(v).all()) for v in mine), (c["id"], label, "the records of the poisoned image are finite")
        print("{}: outside the reach of the Inf and of the NaN, the bits of the clean launch ({} records)".format(c["id"], len(_records_by_image(c, clean, 0, 0)[1]) + 0))
    else:
        raise KeyError(r)


def _run_case(c, seed, dev, lib, what, skipped):
    sets = cv.launch_sets(c, seed) if c["regime"] else {"row": cc.host_tensors(c, seed)}
    outs = {}
    for label, t in sets.items():
        outs[label] = _one(c, t, dev, lib, skipped, again=not outs)
        if not isinstance(outs[label], dict):
            return outs[label]
    if c["regime"]:
        _check_values(c, sets, outs, what)
    else:
        ref = cc.reference(c, sets["row"])
        _check_output(c, outs["row"]["b"], ref, what)
        _check_records(c, outs["row"]["b"], outs["row"]["keep"], ref, sets["row"], dev, what)
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
