"""-m gpu: every row of the variant-conv conformance table (tests/variant_cases.py) through the C ABI on real buffers, one test id per entry
point.

An accepted row is launched and checked for: its output against a float64 restatement of the operation written here in plain torch (no
code of ops.py, no kernel code; the weight packings are restated from the layouts include/cmk.h and the kernel files document); nothing
written outside the output view (every output is the middle of a NaN-filled allocation with a guard image before and after it, views are
channel slices of NaN-filled wider tensors); every input bit-unchanged; the same call again into a fresh NaN-filled output giving the same
bits; a row with views also as a dense call, bit-equal.  NaN and Inf must sit exactly where the float64 result has them, with the one
documented exception that the deformable conv's fused ReLU gives relu(NaN) = 0 (include/cmk.h).  A refused row returns non-zero with an
error text and leaves every output handed in NaN and every input bit-unchanged.

Restatements.  Depth-wise and grouped: F.conv2d(groups=...) in float64, then the affine and the clamps / ReLU.  Stem: conv -> affine -> relu
-> max_pool2d(3, 2, 1) in float64.  Deformable: deform_ref.deform_conv3x3_ref_corners, the per-corner float64 restatement that follows the
rule of include/cmk.h literally and says what is read (tests/test_cpu_variant_conformance.py holds it to the grid_sample restatement).

Bars, all from the project and the references, none from a kernel.  Depth-wise: 1e-5 * max(1, max|ref|) (test_depthwise_conv3x3).
Deformable: min(1e-3, 2e-4 * max(1, max|ref|)) (test_gpu_deform_conv._close).  Grouped and stem: 4x the largest distance of torch's own fp32
CPU result from the float64 one over the table's accepted finite rows, normalised by max(1, max|ref|), computed at run time from the
references alone (the recipe of test_group_conv_matches_float64_torch and test_fused_stem_matches_float64_torch).

A second_trip row holds tens of thousands of images: the float64 reference is computed for image 0, for the image that holds the first
thread of the loop's second trip and for the last image; every other image must be finite everywhere in the view (no NaN sentinel left)
with the sentinel intact outside it.

Observed values: the docstring of test_variant_conformance and DESIGN.md "Variant-conv conformance table"."""
import pytest
import torch
import torch.nn.functional as F

from centermask2_amd import ops
from tests import conformance as C
from tests import variant_cases as vc
from tests.deform_ref import deform_conv3x3_ref_corners, make_offsets

pytestmark = pytest.mark.gpu

NAN, INF = C.NAN, C.INF
CASES = vc.all_cases()
INDEX = {c["id"]: i for i, c in enumerate(CASES)}
_HOST = {}            # row id -> the host tensors and references of a row (the bars and the rows share them)


# ---------------------------------------------------------------------------------------------------------------
# host tensors and float64 references
# ---------------------------------------------------------------------------------------------------------------
def _gen(c, k=0):
    return torch.Generator().manual_seed(9000 + 13 * INDEX[c["id"]] + k)


def _ref_images(c):
    """The images a row's reference is computed for: all, or three of a second_trip row."""
    if c["feature"] != "second_trip":
        return list(range(c["n"]))
    return sorted({0, vc.second_trip_image(c), c["n"] - 1})


def _poison_nhwc(x):
    n, h, w, ch = x.shape
    assert n == 3
    x[0, h // 2, w // 2, ch // 2] = INF
    x[1, 0, 0, 1] = -INF
    x[2, h - 1, w - 1, 0] = NAN
    return x


def _affine(c, ch, k=4, spread=0.1):
    return torch.rand((ch,), generator=_gen(c, k)) + 0.5, torch.randn((ch,), generator=_gen(c, k + 1)) * spread


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous()


def _host(c):
    """dict(x (NHWC; stem: NCHW), w (the packed floats), [scale, shift, off], ref64 (NHWC, the images of _ref_images), [ref32])."""
    if c["id"] in _HOST:
        return _HOST[c["id"]]
    e, n, h, w, ch, stride = c["entry"], c["n"], c["h"], c["w"], c["c"], c["stride"]
    imgs = _ref_images(c)
    finite = not c["poison"]
    out = {}
    if e == vc.DEFORM:
        cin, dg, mod = c["cin"], c["dg"], c["modulated"]
        x = torch.randn((n, cin, h, w), generator=_gen(c))
        if c["poison"]:
            assert n == 3 and h >= 3
            x[0, cin // 2, 0, 0] = INF              # pixel (0,0) of its image and of the batch: where a stand-in address for an unread corner would point
            x[1, 1, h - 1, w // 2] = -INF           # the last row: an in-map corner of weight 0 of the samples on the row above
            x[2, 0, h // 2, w // 2] = NAN
        weight = torch.randn((ch, cin, 3, 3), generator=_gen(c, 1)) / (9 * cin) ** 0.5
        scale, shift = _affine(c, ch)
        off = make_offsets(c["offsets"], c["mask"], n, h, w, dg, mod, seed=50 + INDEX[c["id"]])
        wp = torch.zeros((9, cin, vc.cout_pad(ch)))                                          # [tap][Cin/16][cout_pad][16], zero padded
        wp[:, :, :ch] = weight.permute(2, 3, 1, 0).reshape(9, cin, ch)
        wp = wp.reshape(9, cin // 16, 16, vc.cout_pad(ch)).permute(0, 1, 3, 2).contiguous()
        ref = deform_conv3x3_ref_corners(x, off, weight, dg, mod, scale, shift, relu=bool(c["relu"]))
        out.update(x=_nhwc(x), off=_nhwc(off), w=wp.reshape(-1), scale=scale, shift=shift, ref64=_nhwc(ref))
    elif e in (vc.DWACT, vc.DW):
        x = torch.randn((n, h, w, ch), generator=_gen(c)) * 3.0
        if c["poison"]:
            _poison_nhwc(x)
        weight = torch.randn((ch, 1, 3, 3), generator=_gen(c, 1)) / 3.0
        in_max, out_min, out_max = c["clamps"] if e == vc.DWACT else (INF, -INF, INF)
        scale, shift = _affine(c, ch, spread=2.0) if e == vc.DWACT else (torch.ones(ch), torch.zeros(ch))

        def ref(dtype):
            xin = _nchw(x[imgs]).to(dtype).clamp(max=in_max)                                 # clamp keeps a NaN
            y = F.conv2d(xin, weight.to(dtype), None, stride=stride, padding=1, groups=ch)
            y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
            return _nhwc(y.clamp(min=out_min, max=out_max))

        out.update(x=x, w=weight.reshape(ch, 9).t().contiguous().reshape(-1), scale=scale, shift=shift, ref64=ref(torch.float64))      # [9][C]
    elif e == vc.GROUP:
        groups = c["groups"]
        cg = ch // groups
        x = torch.randn((n, h, w, ch), generator=_gen(c))
        if c["poison"]:
            _poison_nhwc(x)
        weight = torch.randn((ch, cg, 3, 3), generator=_gen(c, 1)) / (9 * cg) ** 0.5
        scale, shift = _affine(c, ch)

        def ref(dtype):
            y = F.conv2d(_nchw(x[imgs]).to(dtype), weight.to(dtype), None, stride=stride, padding=1, groups=groups)
            y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
            return _nhwc(torch.relu(y) if c["relu"] else y)                                  # torch's relu keeps a NaN

        if cg < 16:                                 # [tap][ci][C]
            wp = weight.permute(2, 3, 1, 0)
        else:                                       # [group][chunk][tap][tile][q][n][j]: weight[group*Cg + tile*16 + n][chunk*16 + 4q + j][kh][kw]
            t = cg // 16
            wp = weight.reshape(groups, t, 16, t, 4, 4, 3, 3)                                # group, tile, n, chunk, q, j, kh, kw
            wp = wp.permute(0, 3, 6, 7, 1, 4, 2, 5)
        out.update(x=x, w=wp.contiguous().reshape(-1), scale=scale, shift=shift, ref64=ref(torch.float64))
        if finite:
            out["ref32"] = ref(torch.float32)
    else:
        x = torch.randn((n, 3, h, w), generator=_gen(c)) * 60.0                              # pixel scale
        if c["poison"]:
            x[0, 1, h // 2, w // 3] = INF
            x[1, 0, 0, 0] = -INF
            x[2, 2, h - 1, w - 1] = NAN
        weight = torch.randn((ch, 3, 7, 7), generator=_gen(c, 1)) / (60.0 * 147 ** 0.5)
        scale, shift = _affine(c, ch, spread=0.5)

        def ref(dtype):
            y = F.conv2d(x[imgs].to(dtype), weight.to(dtype), None, stride=2, padding=3)
            y = torch.relu(y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1))
            return _nhwc(F.max_pool2d(y, 3, 2, 1))

        out.update(x=x, w=weight.permute(2, 3, 1, 0).reshape(-1).contiguous(), scale=scale, shift=shift, ref64=ref(torch.float64))      # [147][Cout]
        if finite:
            out["ref32"] = ref(torch.float32)
    if c["feature"] == "second_trip" or e in (vc.GROUP, vc.STEM7):
        _HOST[c["id"]] = out
    return out


# ---------------------------------------------------------------------------------------------------------------
# a row on the device
# ---------------------------------------------------------------------------------------------------------------
def _ceil4(v):
    return -(-v // 4) * 4


def _build(c, dev, bars):
    """(the row's buffers, the output "y" among them, check(the output view on the host) -> normalised distance)."""
    e = c["entry"]
    accept = c["answer"] == "accept"
    what = c["id"]
    B = C.Bufs(dev)

    def put(name, t):
        return B.put(name, t, guard=256)

    def out(rest, **kw):
        """The output: c["n"] maps of shape `rest` between guards (conformance.map_guard)."""
        return B.out("y", (max(1, c["n"]),) + tuple(rest), guard=C.map_guard(c, rest), **kw)

    if not accept:
        # a refused geometry (N = 0, C = 6, a slice that leaves its pixel): buffers large enough for whatever the row says, contents arbitrary
        n, h, w = max(1, c["n"]), max(1, c["h"]), max(1, c["w"])
        ch = max(4, _ceil4(c["c"]))
        xc = max(16, -(-c["cin"] // 16) * 16) if e == vc.DEFORM else ch
        x_cs, x_co = c["x_view"] or (xc, 0)
        y_cs, y_co = c["y_view"] or (ch, 0)
        x_cs, y_cs = _ceil4(max(x_cs, abs(x_co) + xc)) + 8, _ceil4(max(y_cs, abs(y_co) + ch)) + 8
        s = c["stride"] if c["stride"] in (1, 2) else 1
        ho, wo = ((h - 1) // 2 // 2 + 1, (w - 1) // 2 // 2 + 1) if e == vc.STEM7 else ((h - 1) // s + 1, (w - 1) // s + 1)
        g = torch.Generator().manual_seed(1)
        if c["same_buffer"]:
            out((h, w, max(x_cs, y_cs)))
            B.p["x"] = B.p["y"]
        else:
            put("x", torch.randn((n, 3, h, w) if e == vc.STEM7 else (n, h, w, x_cs), generator=g))
            out((ho, wo, y_cs))
        put("w", torch.randn((1 << 19,), generator=g))
        if "scale" in vc.POINTERS[e]:
            put("scale", torch.ones(1024))
            put("shift", torch.zeros(1024))
        if e == vc.DEFORM:
            put("offsets", torch.zeros((n, h, w, max(c["off_cs"] or 0, 27 * max(1, c["dg"])) + 8)))
        return B, None

    hst = _host(c)
    n, h, w, ch = c["n"], c["h"], c["w"], c["c"]
    ho, wo = vc.out_hw(c)
    xc = c["cin"] if e == vc.DEFORM else ch
    y_cs, y_co = c["y_view"] or (ch, 0)

    def wide(x, view):
        if view is None:
            return x
        t = torch.full(tuple(x.shape[:-1]) + (view[0],), NAN)
        t[..., view[1]:view[1] + x.shape[-1]] = x
        return t

    if c["same_buffer"]:
        x_cs, x_co = c["x_view"]
        assert x_cs == y_cs and (ho, wo) == (h, w)
        out((h, w, y_cs), window=(y_co, ch), keep=(x_co, xc, hst["x"]))        # the input slice of the same tensor: the call must keep it
        B.p["x"] = B.p["y"]
    else:
        put("x", hst["x"] if e == vc.STEM7 else wide(hst["x"], c["x_view"]))
        out((ho, wo, y_cs), window=(y_co, ch) if c["y_view"] else None)
    put("w", hst["w"])
    if "scale" in vc.POINTERS[e]:
        put("scale", hst["scale"])
        put("shift", hst["shift"])
    if e == vc.DEFORM:
        put("offsets", wide(hst["off"], (c["off_cs"], 0)) if c["off_cs"] else hst["off"])        # channels past 27*dg are NaN: nothing may read them

    imgs = _ref_images(c)

    def check(got):
        ref = hst["ref64"]
        if len(imgs) != n:
            rest = torch.ones(n, dtype=torch.bool)
            rest[imgs] = False
            assert bool(torch.isfinite(got[rest]).all()), what + ": an image outside the reference set is not written everywhere"
            got = got[imgs]
        if c["poison"]:
            bad = ~torch.isfinite(ref)
            assert bool(bad.any()) and not bool(bad.all()), what + ": the float64 result holds non-finite and finite outputs"
        a, r = C.finite_parts(got.double(), ref, what, nan_is_zero=(e == vc.DEFORM and bool(c["relu"])))
        m = max(1.0, float(r.abs().max())) if r.numel() else 1.0
        err = float((a - r).abs().max()) if r.numel() else 0.0
        bar = {vc.DEFORM: min(1e-3, 2e-4 * m), vc.DWACT: 1e-5 * m, vc.DW: 1e-5 * m, vc.GROUP: bars["group"] * m, vc.STEM7: bars["stem"] * m}[e]
        assert err <= bar, "{}: max abs err {:.3e} from float64 > bar {:.3e}".format(what, err, bar)
        return err / m

    return B, check


def _launch(c, p, lib):
    rc = vc.call(lib, c, p, ops._stream())
    err = lib.cmk_last_error().decode() if rc != 0 else ""
    torch.cuda.synchronize()
    return rc, err


def _conform(c, dev, lib, bars):
    B, check = _build(c, dev, bars)

    def dense_call(first):
        """A row with views also as a dense call, bit-equal."""
        dense = dict(c, x_view=None, y_view=None, off_cs=None)
        B3, _ = _build(dense, dev, bars)
        rc3, err3 = _launch(dense, B3.p, lib)
        assert rc3 == 0, (c["id"], "the dense call", err3)
        assert torch.equal(B3.outs["y"].region(), first["y"]), (c["id"], "the dense call gave other bits than the view call")
    if (c["x_view"] or c["y_view"] or c["off_cs"]) and not c["same_buffer"]:
        B.extra = dense_call
    d = C.run_row(c, B, lambda row: _launch(row, B.p, lib), check and (lambda got: check(got["y"])))
    if c["feature"] == "second_trip":
        _HOST.pop(c["id"], None)                  # hundreds of MB that nothing reads again
    return d


@pytest.fixture(scope="module")
def bars():
    """{"group", "stem"}: 4x the largest normalised distance of torch's own fp32 CPU result from the float64 one over the accepted finite
    rows of the table — from the references alone, before any kernel runs."""
    return {name: C.fp32_bar(name, [c for c in CASES if c["entry"] == entry and c["answer"] == "accept" and not c["poison"]],
                             lambda c: C.dist(_host(c)["ref32"], _host(c)["ref64"])) for name, entry in (("group", vc.GROUP), ("stem", vc.STEM7))}


@pytest.mark.parametrize("entry", vc.ENTRIES)
def test_variant_conformance(dev, cmk_lib, bars, entry):
    """Every row of one entry point.  Measured (torch 2 on an x86 host, an MI355X): torch's own fp32 distance from float64 is at most 8.96e-07
    over the grouped rows (Cg 64 at stride 2) and 4.01e-07 over the stem rows, so the bars came out 3.58e-06 and 1.60e-06; the kernels are at
    most 8.09e-07 (grouped, the same row) and 5.11e-07 (stem, 18 x 26) from float64.  The deformable kernel is at most 6.81e-07 of
    max(1, max|ref|) from float64 (Cout 128, Cin 32) against its bar of 2e-4, the fused depth-wise kernel 3.92e-07 and the plain one 1.34e-07
    against 1e-5.  On the library before the deformable kernel stopped multiplying stand-in loads by 0, the four poison rows fail: 19, 29 and
    30 non-finite pixels of 30 in the image with an Inf at (0,0) where float64 has 4, 9 and 6."""
    C.run_entry(entry, [c for c in CASES if c["entry"] == entry and not c["host_only"]], lambda c: _conform(c, dev, cmk_lib, bars))
