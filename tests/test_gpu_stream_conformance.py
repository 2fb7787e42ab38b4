"""-m gpu: every row of the stream conformance table (tests/stream_cases.py) through the C ABI on real buffers, one test id per entry point.

An accepted row is launched and checked for: its output against a float64 restatement of the operation written here in plain torch (no
code of ops.py); nothing written outside the output view (every output and workspace is the middle of a NaN-filled allocation with a guard
image before and after it, views are channel slices of NaN-filled wider tensors); every input bit-unchanged; the same call again into a
fresh NaN-filled output giving the same bits.  NaN and Inf must sit exactly where the float64 result has them, with the one documented
exception that the stem's and GroupNorm's fused ReLU give relu(NaN) = 0 (groupnorm.hip).  A refused row returns non-zero with an error text
and leaves every output and workspace handed in NaN (an in-place operand: bit-unchanged).

Bars.  Pools, subsample, upsample + add: torch.equal with fp32 torch (max, copy and one rounded add are exact; the gated pool equals
max_pool2d(x) * g in fp32).  ese_scale: |got - ref64| <= 2^-23 * (|x * g| + |identity|) elementwise — the product and the sum round once
each, contracted or not.  eSE gates and the stem: 4x the largest distance of torch's own fp32 CPU result from the float64 one over the
table's accepted rows, normalised by max(1, max|ref|), computed at run time from the references alone (the recipe of
test_fused_stem_matches_float64_torch: another summation order and the MFMA's accumulation tree; a wrong tap, chunk or divisor is off by
orders of magnitude more).  GroupNorm: close(got, ref64, 2e-5) as test_groupnorm_relu; the *_affine entry points through x * scale + shift.

Observed values: the docstring of test_stream_conformance and DESIGN.md §3 "Stream conformance table"."""
import pytest
import torch
import torch.nn.functional as F

from centermask2_amd import ops, synthetic as S
from centermask2_amd._lib import CmkError
from tests import conformance as C
from tests import stream_cases as sc
from tests.helpers import close

pytestmark = pytest.mark.gpu

NAN, INF = C.NAN, C.INF
CASES = sc.all_cases()
INDEX = {c["id"]: i for i, c in enumerate(CASES)}
_HOST = {}            # row id -> the host tensors and references of a stem or gate row (the bars and the rows share them)


# ---------------------------------------------------------------------------------------------------------------
# host tensors
# ---------------------------------------------------------------------------------------------------------------
def _gen(c, k=0):
    return torch.Generator().manual_seed(7000 + 13 * INDEX[c["id"]] + k)


def _sane(c):
    """The row with a geometry that can be allocated (a refused row may say N = 0, H = 0, C = 6 or no records): only sizes buffers."""
    ch = c["c"] if c["entry"] in (sc.GN_RELU, sc.GN, sc.AFFINE, sc.MULTI, sc.TILES) else max(4, -(-c["c"] // 4) * 4)      # float4 lanes: whole quads
    g = dict(c, n=max(1, c["n"]), h=max(1, c["h"]), w=max(1, c["w"]), c=ch, chunks=max(1, c["chunks"]), rows=max(1, c["rows"]), groups=max(1, c["groups"]))
    if c["levels"] is not None:
        g["levels"] = [tuple(max(1, v) for v in lv) for lv in c["levels"]] or [(1, 1, 1) if c["entry"] == sc.TILES else (1, 1)]
    for k in ("x_view", "y_view", "id_view"):
        if c[k]:
            g[k] = (-(-max(c[k][0], c[k][1] + g["c"]) // 4) * 4, c[k][1])
    return g


def _poison(x, window=False):
    """One +Inf in image 0, a -Inf in image 1 (window: a whole 3x3 window of every channel), one NaN in image 2 of an (3, h, w, c) map,
    all at even coordinates (the stride-2 subsample reads those)."""
    n, h, w, c = x.shape
    assert n == 3
    x[0, h // 4 * 2, w // 6 * 2, c // 2] = INF
    if window:
        x[1, :3, :3, :] = -INF
    else:
        x[1, 0, 0, 1] = -INF
    x[2, (h - 1) // 2 * 2, (w - 1) // 2 * 2, 0] = NAN
    return x


def _data(c, shape, k=0, window=False):
    """Seeded fp32 map of a row: randn, or all negative, poisoned where the row says so."""
    x = torch.randn(shape, generator=_gen(c, k))
    if c["fill"] == "negative":
        x = -(x.abs() + 0.1)
    if c["poison"] and k == 0:
        _poison(x, window)
    return x


def _wide(x, view):
    """x as the channel slice `view` = (cs, co) of a NaN-filled wider tensor (None: x itself)."""
    if view is None:
        return x
    cs, co = view
    t = torch.full(tuple(x.shape[:-1]) + (cs,), NAN)
    t[..., co:co + x.shape[-1]] = x
    return t


def _pool3_out(h):
    ho = -(-(h - 3) // 2) + 1
    return max(1, ho - 1 if (ho - 1) * 2 >= h else ho)


def _stem_host(c):
    """Pixel-scale images and the synthetic stem_1 parameters; ref(dtype) = relu(conv3x3 s2 p1 (x) * scale + shift), NHWC."""
    if c["id"] in _HOST:
        return _HOST[c["id"]]
    g = _sane(c)
    n, h, w, cout = g["n"], g["h"], g["w"], g["c"]
    x = S.make_synthetic_images(n, h, w, seed0=900 + 10 * INDEX[c["id"]])
    if c["poison"]:
        x[0, 1, h // 2, w // 3] = INF
        x[1, 0, 0, 0] = -INF
        x[2, 2, h - 1, w - 1] = NAN
    key = "backbone.bottom_up.stem.stem_1/"
    wt = S.synthetic_tensor(key + "conv.weight", (cout, 3, 3, 3))
    bw, bb, mean, var = (S.synthetic_tensor(key + "norm." + k, (cout,)) for k in ("weight", "bias", "running_mean", "running_var"))
    scale = (bw / torch.sqrt(var + 1e-5)).float()
    shift = (bb - mean * scale).float()

    def ref(dtype):
        y = F.conv2d(x.to(dtype), wt.to(dtype), None, stride=2, padding=1) * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
        return F.relu(y).permute(0, 2, 3, 1).contiguous()

    out = dict(x=x, w27=wt.permute(2, 3, 1, 0).reshape(27, cout).contiguous(), scale=scale, shift=shift, ref64=ref(torch.float64))
    if c["answer"] == "accept" and not c["poison"]:
        out["ref32"] = ref(torch.float32)
    _HOST[c["id"]] = out
    return out


def _gate_of(mean, fw, fb):
    """relu6(fc(mean) + 3) / 6 in the dtype of its arguments."""
    return torch.clamp(mean @ fw.t() + fb + 3.0, 0.0, 6.0) / 6.0


def _gate_host(c):
    """A map with channel means of order one and an FC that saturates some gates at 0, some at 1 and leaves some between.  cmk_ese_gate:
    ref64 from the map.  cmk_ese_gate_pooled: the fp32 records by the layout's definition (record 2g: the rows of block g that lie in the
    image of the block's first pixel, 2g + 1: its rows in the next image; a record nothing may read is NaN) and ref64 from those records."""
    if c["id"] in _HOST:
        return _HOST[c["id"]]
    g = _sane(c)
    n, h, w, ch, hw = g["n"], g["h"], g["w"], g["c"], g["h"] * g["w"]
    x = torch.randn((n, h, w, ch), generator=_gen(c)) + torch.randn((ch,), generator=_gen(c, 1))
    if c["poison"]:
        _poison(x)
    fw = torch.randn((ch, ch), generator=_gen(c, 2)) * 3.0 * ch ** -0.5
    fb = torch.randn((ch,), generator=_gen(c, 3)) * 2.0
    if ch == 4:
        fw, fb = fw * 0.1, torch.tensor([-9.0, 9.0, 0.5, -0.5])       # eight gates of a random FC all lie between 0 and 1: set by hand
    out = dict(x=x, fw=fw, fb=fb)
    x64 = x.double().reshape(n, hw, ch)
    mean64 = x64.mean(1)
    if c["entry"] == sc.POOLED:
        rows = g["rows"]
        flat = x64.reshape(n * hw, ch)
        blocks = -(-(n * hw) // rows)
        rec = torch.full((2 * blocks + 2, ch), NAN)      # two records past the last block: nothing may read them either
        sums = torch.zeros((n + 1, ch), dtype=torch.float64)
        for b in range(blocks):
            p0, p1 = b * rows, min((b + 1) * rows, n * hw)
            img = p0 // hw
            split = min(p1, (img + 1) * hw)
            rec[2 * b] = flat[p0:split].sum(0).float()
            sums[img] += rec[2 * b].double()
            if p1 > split:
                rec[2 * b + 1] = flat[split:p1].sum(0).float()
                sums[img + 1] += rec[2 * b + 1].double()
        out["rec"] = rec
        mean64 = sums[:n] / hw
    out["ref64"] = _gate_of(mean64, fw.double(), fb.double())
    if c["answer"] == "accept" and not c["poison"]:
        out["ref32"] = _gate_of(x.reshape(n, hw, ch).mean(1), fw, fb)
    _HOST[c["id"]] = out
    return out


def _gn_ref(x, gamma, beta, groups, relu):
    """float64 GroupNorm of an NHWC fp32 map."""
    y = F.group_norm(x.double().permute(0, 3, 1, 2), groups, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 3, 1).contiguous()
    return F.relu(y) if relu else y


def _gn_host(c, shape, k=0):
    x = torch.randn(shape, generator=_gen(c, 10 + k)) * 3.0 + 1.5
    if c["poison"]:
        cpg = shape[3] // max(1, c["groups"])
        x[0, shape[1] // 2, shape[2] // 3, cpg + 1] = INF            # group 1 of image 0
        x[1, 0, 0, 2 * cpg] = -INF                                   # group 2 of image 1
        x[2, shape[1] - 1, shape[2] - 1, 0] = NAN                    # group 0 of image 2
    return x


def _gn_params(c, ch):
    return torch.rand((ch,), generator=_gen(c, 4)) + 0.5, torch.randn((ch,), generator=_gen(c, 5)) * 0.1


# ---------------------------------------------------------------------------------------------------------------
# a row on the device
# ---------------------------------------------------------------------------------------------------------------
def _build(c, dev, bars):
    """(the row's buffers, check(got {name: the output on the host}) -> distance on record)."""
    e = c["entry"]
    g = _sane(c)
    n, h, w, ch, hw = g["n"], g["h"], g["w"], g["c"], g["h"] * g["w"]
    accept = c["answer"] == "accept"
    what = c["id"]
    B = C.Bufs(dev)
    p = B.p

    def put(name, t):
        return B.put(name, t, guard=256)

    def out(name, rest, view=None, init=None, dtype=torch.float32, images=n):
        """`images` maps of shape `rest` between guards (conformance.map_guard); view: the call owns a channel slice of the last dimension."""
        return B.out(name, (images,) + tuple(rest), dtype, init=init, guard=C.map_guard(c, rest, 8 if dtype == torch.float64 else 4),
                     window=None if view is None else (view[1], ch))

    if e == sc.STEM:
        hst = _stem_host(c)
        for k, v in (("x", hst["x"]), ("w", hst["w27"]), ("scale", hst["scale"]), ("shift", hst["shift"])):
            put(k, v)
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out("y", (ho, wo, ch))

        def check(got):
            d = C.dist(*C.finite_parts(got["y"].double(), hst["ref64"], what, nan_is_zero=True))
            assert d <= bars["stem"], "{}: {:.3e} from float64 > bar {:.3e}".format(what, d, bars["stem"])
            return d
    elif e in (sc.POOL3, sc.POOL1):
        x = _data(c, (n, h, w, ch), window=True)
        put("x", _wide(x, g["x_view"]))
        gate = None
        if c["gate"]:
            gate = torch.rand((n, ch), generator=_gen(c, 6)) + (0.05 if c["poison"] else 0.0)      # -inf * 0 would be a NaN of the gate's, not of the pool's
            if not c["poison"]:
                gate[0, 0], gate[n - 1, ch - 1] = 0.0, 1.0
            put("gate", gate)
        elif e == sc.POOL3:
            p["gate"] = None
        if e == sc.POOL3:
            ho, wo = _pool3_out(h), _pool3_out(w)
        else:
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out("y", (ho, wo, (g["y_view"] or (ch, 0))[0]), g["y_view"])

        def check(got):
            xc = x.permute(0, 3, 1, 2)
            ref = F.max_pool2d(xc, 3, 2, ceil_mode=True) if e == sc.POOL3 else xc[:, :, ::2, ::2]
            ref = ref.permute(0, 2, 3, 1)
            if gate is not None:
                ref = ref * gate[:, None, None, :]
            if c["fill"] == "negative":
                assert bool((ref <= 0).all()) and bool((ref < 0).any())
            if c["poison"]:
                assert bool((ref[1, 0, 0] == -INF).all()) and bool(torch.isnan(ref[2]).any()) and bool((ref[0] == INF).any())
            return C.exact(got["y"], ref.contiguous(), what)
    elif e == sc.UPADD:
        y0, coarse = _data(c, (n, h, w, ch)), torch.randn((n, max(1, g["hc"]), max(1, g["wc"]), ch), generator=_gen(c, 1))
        if c["poison"]:
            coarse[0, 0, 0, 1] = NAN
        put("coarse", coarse)
        out("y", (h, w, ch), init=y0)

        def check(got):
            up = coarse.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h, :w]
            return C.exact(got["y"], y0 + up, what)
    elif e in (sc.GATE, sc.POOLED):
        hst = _gate_host(c)
        put("fc_w", hst["fw"])
        put("fc_b", hst["fb"])
        if e == sc.GATE:
            put("x", _wide(hst["x"], g["x_view"]))
            chunks = g["chunks"]
            out("ws", (chunks, ch))
        else:
            put("pool_ws", hst["rec"])
        out("gate", (ch,))

        def check(got):
            ref = hst["ref64"]
            if not c["poison"]:
                assert bool((ref == 0).any()) and bool((ref == 1).any()) and bool(((ref > 0) & (ref < 1)).any()), what + ": the gates must saturate both ways and lie between"
            else:
                assert bool(torch.isnan(ref[2]).all()) and not bool(torch.isnan(ref[:2]).any())
            d = C.dist(*C.finite_parts(got["gate"].double(), ref, what))
            assert d <= bars["gate"], "{}: {:.3e} from float64 > bar {:.3e}".format(what, d, bars["gate"])
            if e == sc.GATE:
                per = -(-hw // chunks)
                used = -(-hw // per)
                ws = got["ws"]
                assert bool((ws[:, used:] == 0).all()), what + ": an empty chunk must hold exact zeros"
                if not c["poison"]:
                    assert bool(torch.isfinite(ws).all())
                    close(ws.double().sum(1) / hw, hst["x"].double().reshape(n, hw, ch).mean(1), 1e-5, "stream eSE partial sums")       # the partial sums themselves
            return d
    elif e == sc.SCALE:
        x = _data(c, (n, h, w, ch))
        gate = torch.rand((n, ch), generator=_gen(c, 6))
        gate[0, 0], gate[n - 1, ch - 1] = 0.0, 1.0
        idn = torch.randn((n, h, w, ch), generator=_gen(c, 7)) if c["identity"] else None
        put("gate", gate)
        if idn is not None:
            put("identity", _wide(idn, g["id_view"]))
        else:
            p["identity"] = None
        if c["same_buffer"]:
            out("y", (h, w, ch), init=x)
            p["x"] = p["y"]
        else:
            put("x", _wide(x, g["x_view"]))
            out("y", (h, w, (g["y_view"] or (ch, 0))[0]), g["y_view"])

        def check(got):
            prod = x.double() * gate.double()[:, None, None, :]
            ref = prod + (idn.double() if idn is not None else 0.0)
            bound = 2.0 ** -23 * (prod.abs() + (idn.double().abs() if idn is not None else 0.0))
            a, r = C.finite_parts(got["y"].double(), ref, what)
            err = (a - r).abs()
            b = bound[torch.isfinite(ref)]
            assert bool((err <= b).all()), "{}: {:.3e} over the rounding bound".format(what, float((err - b).max()))
            return float((err / b.clamp_min(1e-30)).max()) if err.numel() else 0.0
    elif e in (sc.GN_RELU, sc.GN, sc.AFFINE):
        x = _gn_host(c, (n, h, w, ch))
        gamma, beta = _gn_params(c, ch)
        put("gamma", gamma)
        put("beta", beta)
        out("ws", (g["groups"], g["chunks"], 2), dtype=torch.float64)
        if e == sc.AFFINE:
            put("x", x)
            out("out_scale", (ch,))
            out("out_shift", (ch,))
        else:
            out("x", (h, w, ch), init=x)

        def check(got):
            if e == sc.AFFINE:
                y = x.double() * got["out_scale"].double()[:, None, None, :] + got["out_shift"].double()[:, None, None, :]
                ref = _gn_ref(x, gamma, beta, g["groups"], False)
            else:
                y, ref = got["x"].double(), _gn_ref(x, gamma, beta, g["groups"], e == sc.GN_RELU)
            if c["poison"]:
                cpg = ch // g["groups"]
                hole = torch.zeros_like(ref, dtype=torch.bool)
                hole[0, :, :, cpg:2 * cpg] = hole[1, :, :, 2 * cpg:3 * cpg] = hole[2, :, :, :cpg] = True
                ref = _gn_ref(x, gamma, beta, g["groups"], False)
                assert torch.equal(torch.isnan(ref), hole), what + ": float64 GroupNorm makes exactly the poisoned (image, group) NaN"
                if e == sc.GN_RELU:
                    ref = F.relu(torch.nan_to_num(ref, nan=0.0))
                    assert not bool(torch.isnan(y).any()) and bool((y[hole] == 0).all()), what + ": relu(NaN) must be 0"
                else:
                    assert torch.equal(torch.isnan(y), hole), what + ": a poisoned value must make exactly its (image, group) NaN"
                y, ref = y[~hole], ref[~hole]
            assert bool(torch.isfinite(y).all()), what + ": the output is not written everywhere"
            return close(y, ref, 2e-5, "stream " + e) / max(1.0, float(ref.abs().max()))
    elif e in (sc.MULTI, sc.TILES):
        levels = g["levels"]
        nlev = len(levels)
        groups = g["groups"]
        xs = [_gn_host(c, (n, lv[0], lv[1], ch), k) for k, lv in enumerate(levels)]
        gamma, beta = _gn_params(c, ch)
        put("gamma", gamma)
        put("beta", beta)
        p["out_scale"], p["out_shift"] = [], []
        for k in range(nlev):
            for name in ("out_scale", "out_shift"):
                p[name].append(out("{}{}".format(name, k), (ch,)).ptr())
        if e == sc.MULTI:
            p["xs"] = [put("x{}".format(k), x).ptr() for k, x in enumerate(xs)]
            out("ws", (groups, g["chunks"], 2), dtype=torch.float64, images=nlev * n)
        elif not accept:
            put("ws", torch.full((64, groups, 2), NAN, dtype=torch.float64))        # (a refused geometry need not cut into records)
        else:
            # the records a conv epilogue would leave: each image's pixels cut into `recs` arbitrary (some empty) parts, per part and
            # group {sum, sumsq} in float64; level l starts at record sum(N * recs of the levels before it)
            cpg = ch // groups
            recs = []
            for k, (lh, lw, nrec) in enumerate(levels):
                xg = xs[k].double().reshape(n, lh * lw, groups, cpg)
                cuts = torch.randint(0, lh * lw + 1, (n, max(0, nrec - 1)), generator=_gen(c, 20 + k)).sort(1).values
                for i in range(n):
                    edges = [0] + cuts[i].tolist() + [lh * lw]
                    for r in range(nrec):
                        part = xg[i, edges[r]:edges[r + 1]]
                        recs.append(torch.stack([part.sum((0, 2)), (part * part).sum((0, 2))], 1))
            recs.append(torch.full((8, groups, 2), NAN, dtype=torch.float64))       # past the last level: nothing may read them
            put("ws", torch.cat([r.reshape(-1, groups, 2) for r in recs]))

        def check(got):
            worst = 0.0
            for k, x in enumerate(xs):
                y = x.double() * got["out_scale{}".format(k)].double()[:, None, None, :] + got["out_shift{}".format(k)].double()[:, None, None, :]
                ref = _gn_ref(x, gamma, beta, groups, False)
                if c["poison"]:
                    assert bool(torch.isnan(ref).any()) and torch.equal(torch.isnan(y), torch.isnan(ref)), what + ": a poisoned value must make exactly its (image, group) NaN"
                    y, ref = y[~torch.isnan(ref)], ref[~torch.isnan(ref)]
                assert bool(torch.isfinite(y).all()), what + ": scale and shift are not written everywhere"
                worst = max(worst, close(y, ref, 2e-5, "stream " + e) / max(1.0, float(ref.abs().max())))
            return worst
    else:
        raise KeyError(e)
    return B, check


def _conform(c, dev, lib, bars):
    B, check = _build(c, dev, bars)

    def launch(row):
        rc = sc.call(lib, row, B.p, ops._stream())
        err = lib.cmk_last_error().decode() if rc != 0 else ""
        torch.cuda.synchronize()
        return rc, err
    return C.run_row(c, B, launch, check)


@pytest.fixture(scope="module")
def bars():
    """{"stem", "gate"}: 4x the largest normalised distance of torch's own fp32 CPU result from the float64 one over the accepted finite
    rows of the table — from the references alone, before any kernel runs."""
    def distance(host):
        return lambda c: C.dist(host(c)["ref32"], host(c)["ref64"])
    return {name: C.fp32_bar(name, [c for c in CASES if c["entry"] in entries and c["answer"] == "accept" and not c["poison"]], distance(host))
            for name, entries, host in (("stem", (sc.STEM,), _stem_host), ("gate", (sc.GATE, sc.POOLED), _gate_host))}


@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_stream_conformance(dev, cmk_lib, bars, entry):
    """Every row of one entry point.  Measured (torch 2 on an x86 host, an MI355X): torch's own fp32 distance from float64 is at most 3.24e-07
    over the stem rows (the 1449x1449 image) and 9.51e-07 over the gate rows (C 1280 at one pixel; 4.26e-07 on another host's BLAS), so the
    bars came out 1.29e-06 and 3.80e-06 (1.71e-06 on the other host); the kernels are at most 3.02e-07 (stem), 4.19e-07 (cmk_ese_gate, C 1280
    in one chunk: the fp32 partial sums) and 5.96e-08 (cmk_ese_gate_pooled) from float64.  cmk_ese_scale uses at most 0.946 of its rounding
    bound.  The GroupNorm entry points are at most 1.54e-07 (relu), 1.44e-07 (plain), 1.45e-07 (affine), 1.39e-07 (multi) and 1.09e-07 (tiles)
    of max(1, max|ref|) from float64 against the bar of 2e-5.  The pools, the subsample and the upsample + add are bit-equal."""
    C.run_entry(entry, [c for c in CASES if c["entry"] == entry and not c["host_only"]], lambda c: _conform(c, dev, cmk_lib, bars))


def test_wrong_inputs_are_refused(dev):
    """The wrappers of ops.py take raw data pointers: a tensor the C ABI would misread is refused before any launch, the outputs untouched."""
    x = torch.randn((2, 5, 7, 16), device=dev)
    gamma, beta = torch.ones(16, device=dev), torch.zeros(16, device=dev)
    permuted = torch.randn((2, 16, 5, 7), device=dev).permute(0, 2, 3, 1)      # NHWC by shape, NCHW in memory
    keep = permuted.clone()
    for bad in (permuted, x[:, :, :, :8], x[0], x.double()):
        with pytest.raises(CmkError):
            ops.groupnorm_relu_(bad, gamma[:bad.shape[-1]], beta[:bad.shape[-1]], groups=2)
        with pytest.raises(CmkError):
            ops.groupnorm_affine(bad, gamma[:bad.shape[-1]], beta[:bad.shape[-1]], groups=2)
    assert torch.equal(permuted, keep)
    xv = ops.View(x)
    fw, fb = torch.randn((16, 16), device=dev), torch.randn((16,), device=dev)
    good = torch.rand((2, 16), device=dev)
    for gate in (torch.rand((2, 20), device=dev), torch.rand((16, 2), device=dev).t(), good.double(), good.cpu(), good[:1]):
        y = ops.View(torch.full((2, 5, 7, 16), NAN, device=dev))
        with pytest.raises(CmkError):
            ops.ese(xv, fw, fb, y, gate=gate)
        pooled = ops.View(torch.full((2, 2, 3, 16), NAN, device=dev))
        with pytest.raises(CmkError):
            ops.maxpool3x3s2_ceil(xv, pooled, gate=gate)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y.t).all()) and bool(torch.isnan(pooled.t).all())
    for y in (ops.View(torch.full((2, 5, 8, 16), NAN, device=dev)), ops.View(torch.full((2, 5, 7, 32), NAN, device=dev), 0, 20),
              ops.View(torch.full((1, 5, 7, 16), NAN, device=dev))):
        with pytest.raises(CmkError):
            ops.ese(xv, fw, fb, y, gate=good)
        with pytest.raises(CmkError):
            ops.ese(xv, fw, fb, ops.View(torch.empty_like(x)), identity=y, gate=good)
        with pytest.raises(CmkError):
            ops.maxpool3x3s2_ceil(xv, y)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y.t).all())
    # and the right ones pass
    y = ops.View(torch.full((2, 5, 7, 16), NAN, device=dev))
    ops.ese(xv, fw, fb, y, gate=good)
    ops.groupnorm_relu_(x.clone(), gamma, beta, groups=2)
    torch.cuda.synchronize()
    assert torch.equal(y.t, x * good[:, None, None, :])
