"""The value side of the conv conformance table (tests/conv_cases.py): the data regimes of its value features, the fp32 CPU emulations of
the families' algorithms, the bars that come from them, and the reach of one poisoned input pixel.  No tests here and no call into the
library: tests/test_cpu_conv_values.py proves on the CPU that the rows can fail, tests/test_gpu_conv_conformance.py launches them.

Regimes (launch_sets gives the tensors of every launch of a row, keyed by a label):
  ints           x in [-4, 4], w in [-2, 2], scale 1, shift in [-3, 3] (0 for the split forms): every product and partial sum is an integer
                 below 2^24 in any order, so every family but F(4x4) (thirds in G) must EQUAL the float64 reference.
  pow2_channels  x[..., c] * 2^e_c and w[:, c] * 2^-e_c: the products are unchanged, so the output has the bits of the "plain" launch
                 (the fp16-split families, whose pieces can go subnormal: e_c in [-6, 6] and the bar).
  cancel         x = 1 + 2^-9 r, the mean of every output channel's filter bank subtracted (rounded to fp32 once): the signal lives in the
                 low bits of x; the bar is taken relative to max|ref| itself.  Odd input channels hold minus their even neighbour's weights
                 plus 2^-10 of noise: with plain zero-mean filters the partial sums walk up to ~1.4, the fma chain's own error is 2.7e-6
                 and a tune_wm 10 kernel without one of its six products (1.5e-5 .. 2.5e-5, whatever the 2^-k) stays within 4x the bar;
                 with the pairs the chain is at 1.3e-7 and the mutants 24x to 48x above the bar (tests/test_cpu_conv_values.py).
  sparse         x = relu(r), every fifth channel and the whole last image zero, the fused ReLU on: that image is relu(shift) exactly.
  nonfinite      a "clean" launch, one with +Inf at (H/2, W/2, Cin/2) of image 0 and one with NaN at (H-1, W-1, 0) of the last image.
  f16_domain     the fp16-split families: "a" max|x| = 1e6; "b" one input channel's weights at 2^-16 of the largest, its x times 2^16.

Emulations (emulate): fp32 arithmetic in the family's order, written from include/cmk.h and DESIGN.md.
  direct, gather, pointwise   one fp32 fma chain over K = taps x Cin in the packed layout's order (tap-major), one rounding per product;
  F(2x2), F(4x4)              tools/wino_numerics.py:wino_conv (the one copy, loaded from the tool) with the channel contraction as an fma chain;
  tune_wm 10                  three bf16 pieces per operand, per 16-channel chunk the six products l*h, h*l, m*m, m*h, h*m, h*h, fma chain;
  tune_wm 11, 12              two fp16 pieces with the 2^-4, 2^11 and S_w scalings, per chunk the products m*h, h*m, h*h, fma chain.
An fma is emulated as a float64 product (exact for fp32 operands) added in float64 and rounded to fp32: one rounding except in the rare
double-rounding tie, which is far below what a bar resolves and cannot occur on exact integer sums.  The epilogue is one fma per output.

The bar of a row is conformance.fp32_bar's recipe: 4x the emulation's own distance from float64 on that row's tensors."""
import importlib.util
import math
import os

import torch
import torch.nn.functional as F

from tests import conv_cases as cc

_spec = importlib.util.spec_from_file_location("wino_numerics", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "wino_numerics.py"))
wino_numerics = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wino_numerics)

INF, NAN = float("inf"), float("nan")
MARGIN = 4.0                       # the project's margin for summation order (conformance.fp32_bar)
CANCEL_BITS = 9                    # cancel: x = 1 + 2^-9 r
BF16_PRODUCTS = ("lh", "hl", "mm", "mh", "hm", "hh")       # activation piece, weight piece; smallest terms first (conv_split.hpp mfma6_bf16)
F16_PRODUCTS = ("mh", "hm", "hh")                          # conv_split.hpp mfma3_f16


def f16_split(c):
    return c["tv"][0] in (11, 12)


def exact_ints(c):
    """ints must equal float64: every family but the six F(4x4) ones (conv_cases.HELD_TO_BAR has the reason)."""
    return (c["family"], "ints") not in cc.HELD_TO_BAR


def exact_pow2(c):
    return (c["family"], "pow2_channels") not in cc.HELD_TO_BAR


# ---------------------------------------------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------------------------------------------
def poison_site(c, label):
    """(problem, image, row, column, channel) of the poisoned input element of the launch `label` ("inf" | "nan")."""
    if label == "inf":
        n, h, w = c["shapes"][0]
        return 0, 0, h // 2, w // 2, c["cin"] // 2
    n, h, w = c["shapes"][-1]
    return len(c["shapes"]) - 1, n - 1, h - 1, w - 1, 0


def launch_sets(c, seed):
    """{label: tensors as conv_cases.host_tensors gives them} of a value row, in launch order."""
    r = c["regime"]
    t = cc.host_tensors(c, seed)
    g = torch.Generator().manual_seed(7000 + seed)
    cin, cout, n_p = c["cin"], c["cout"], len(c["shapes"])
    assert c["x_view"] is None and not c["same_buffer"] and not c["res_mode"] and not c["in_affine"] and not c["in_relu"] and c["weight_sets"] == 1
    if r == "ints":
        t["x"] = [torch.randint(-4, 5, x.shape, generator=g).float() for x in t["x"]]
        t["w"] = [torch.randint(-2, 3, w.shape, generator=g).float() for w in t["w"]]
        t["scale"] = [torch.ones(cout)] * n_p
        t["shift"] = [torch.zeros(cout) if c["zero_shift"] else torch.randint(-3, 4, (cout,), generator=g).float()] * n_p
        return {"row": t}
    if r == "pow2_channels":
        span = 6 if f16_split(c) else 12
        e = torch.exp2(torch.randint(-span, span + 1, (cin,), generator=g).float())
        s = dict(t, x=[x * e for x in t["x"]], w=[w / e[None, :, None, None] for w in t["w"]])
        return {"plain": t, "row": s}
    if r == "cancel":
        t["x"] = [1.0 + 2.0 ** -CANCEL_BITS * x for x in t["x"]]
        ws = []
        for w in t["w"]:
            w = w.clone()
            # neighbouring input channels cancel down to 2^-10: the partial sums of any K order stay at one weight's size (so the emulation's
            # own error, and with it the bar, is that of the signal and not of a random walk of weights), the low pieces of the pair do not
            w[:, 1::2] = -(w[:, 0::2] + 2.0 ** -10 * torch.randn(w[:, 0::2].shape, generator=g) * float(w.std()))
            ws.append((w.double() - w.double().mean(dim=(1, 2, 3), keepdim=True)).float())
        t["w"] = ws
        return {"row": t}
    if r == "sparse":
        xs = []
        for x in t["x"]:
            x = x.relu()
            x[..., ::5] = 0
            xs.append(x)
        xs[-1][-1] = 0
        t["x"] = xs
        return {"row": t}
    if r == "nonfinite":
        sets = {"clean": t}
        for label, v in (("inf", INF), ("nan", NAN)):
            p, j, y, x, ch = poison_site(c, label)
            xs = [v_.clone() for v_ in t["x"]]
            xs[p][j, y, x, ch] = v
            sets[label] = dict(t, x=xs)
        return sets
    if r == "f16_domain":
        top = max(float(x.abs().max()) for x in t["x"])
        a = dict(t, x=[x * (1e6 / top) for x in t["x"]])
        a["x"] = [x * (1e6 / float(x.abs().max())) if float(x.abs().max()) > 1e6 else x for x in a["x"]]     # the rounding of the factor must not pass 1e6
        ch = cin // 3
        w = t["w"][0].clone()
        w[:, ch] *= 2.0 ** -16 * float(w.abs().max()) / float(w[:, ch].abs().max())
        xs = [x.clone() for x in t["x"]]
        for x in xs:
            x[..., ch] *= 2.0 ** 16
        return {"a": a, "b": dict(t, x=xs, w=[w])}
    raise KeyError(r)


def reach(c, h, w, py, px):
    """The (Ho, Wo) bool map of the outputs of one image that may depend on its input pixel (py, px), from the family and the geometry
    alone: the k x k outputs whose taps read it (a stride of 2 keeps those it lands on), or, for the Winograd forms, the 2x2 / 4x4 output
    tiles (anchored at the image's corner) whose 4x4 / 6x6 input window holds it."""
    ho, wo = cc.out_hw(c, h, w)
    wm, k, s = c["tv"][0], c["k"], c["stride"]
    if wm in (5, 6):
        m = 2 if wm == 5 else 4
        rows = [o for o in range(ho) if m * (o // m) - 1 <= py <= m * (o // m) + m]
        cols = [o for o in range(wo) if m * (o // m) - 1 <= px <= m * (o // m) + m]
    else:
        rows = [o for o in range(ho) if 0 <= py - (o * s - k // 2) < k]
        cols = [o for o in range(wo) if 0 <= px - (o * s - k // 2) < k]
    out = torch.zeros((ho, wo), dtype=torch.bool)
    if rows and cols:
        out[torch.tensor(rows)[:, None], torch.tensor(cols)[None, :]] = True
    return out


# ---------------------------------------------------------------------------------------------------------------
# emulations
# ---------------------------------------------------------------------------------------------------------------
def _fma(acc, a, b):
    return (acc.double() + a.double() * b.double()).float()


def _gemm_operands(c, x, w):
    """A (pixels, K) and B (K, Cout) of the conv as a GEMM, K = taps x Cin tap-major as the packed layouts walk it."""
    k, cin = c["k"], c["cin"]
    cols = F.unfold(x.permute(0, 3, 1, 2), k, padding=k // 2, stride=c["stride"])               # (N, Cin * k * k, L), channel-major
    n, _, L = cols.shape
    a = cols.reshape(n, cin, k * k, L).permute(0, 3, 2, 1).reshape(n * L, k * k * cin)
    return a.contiguous(), _b_operand(w)


def _b_operand(w):
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()


def _chain(products, chunk=16):
    """The fp32 accumulator after one fma per (product, k), walking K in chunks of 16 and, inside a chunk, the products in order."""
    a0, b0 = products[0]
    acc = torch.zeros((a0.shape[0], b0.shape[1]))
    for k0 in range(0, a0.shape[1], chunk):
        for a, b in products:
            for k in range(k0, min(k0 + chunk, a0.shape[1])):
                acc = _fma(acc, a[:, k, None], b[None, k])
    return acc


def pieces_bf16(t):
    h = t.bfloat16().float()
    m = (t - h).bfloat16().float()
    return {"h": h, "m": m, "l": (t - h - m).bfloat16().float()}


def pieces_f16_x(x):
    """Activations: x' = x * 2^-4, h = fp16(x'), m = fp16((x' - h) * 2^11)."""
    xs = x * 0.0625
    h = xs.half().float()
    return {"h": h, "m": ((xs - h) * 2048.0).half().float()}


def pieces_f16_w(w):
    """Weights: w' = w * S_w (max |w'| in [2^14, 2^15)), h = fp16(w'), m = fp16(w' - h); "s": the piece h * 2^-11 in fp16 that meets the
    activations' scaled residual.  Returns (pieces, S_w)."""
    s_w = 2.0 ** (14 - math.floor(math.log2(float(w.abs().max()))))
    ws = w * s_w
    h = ws.half().float()
    return {"h": h, "m": (ws - h).half().float(), "s": (h * (1.0 / 2048.0)).half().float()}, s_w


def _chain_contract(u, v):
    a, b, o, ch = u.shape
    m = torch.zeros((a, b, v.shape[2], o, v.shape[4]))
    for k in range(ch):
        m = _fma(m, u[:, :, None, :, k, None], v[:, :, :, None, k, :])
    return m


def emulate(c, t, drop=None, mats=None):
    """Per problem the fp32 output (N, Ho, Wo, Cout) of the family's algorithm on the tensors t.  drop: a product of the split forms to
    leave out; mats: other Winograd matrices (both: the mutants of tests/test_cpu_conv_values.py)."""
    wm, cout = c["tv"][0], c["cout"]
    relu_upto = cout if c["relu_upto"] is None else c["relu_upto"]
    out = []
    for i, (n, h, w_) in enumerate(c["shapes"]):
        x, w = t["x"][i], t["w"][0]
        ho, wo = cc.out_hw(c, h, w_)
        gain = 1.0
        if wm in (5, 6):
            m = 2 if wm == 5 else 4
            acc = wino_numerics.wino_conv(x.permute(0, 3, 1, 2), w, None, m, m, mats=mats, contract=_chain_contract).permute(0, 2, 3, 1)
        else:
            a, b = _gemm_operands(c, x, w)
            if wm == 10:
                pa, pb = pieces_bf16(a), pieces_bf16(b)
                products = [(pa[p[0]], pb[p[1]]) for p in BF16_PRODUCTS if p != drop]
            elif wm in (11, 12):
                pa, (pb, s_w) = pieces_f16_x(a), pieces_f16_w(w)
                pb = {k: _b_operand(v) for k, v in pb.items()}
                products = [(pa[p[0]], pb["s" if p == "mh" else p[1]]) for p in F16_PRODUCTS if p != drop]
                gain = 16.0 / s_w
            else:
                products = [(a, b)]
            acc = _chain(products).reshape(n, ho, wo, cout)
        y = _fma(t["shift"][i].expand_as(acc), acc, t["scale"][i] * gain)
        y[..., :relu_upto] = y[..., :relu_upto].relu()
        out.append(y)
    return out


def norm_of(c, ref):
    """What a row's distances are printed relative to: max|ref| itself where the signal is small (cancel) or huge (f16_domain)."""
    top = float(ref[torch.isfinite(ref)].abs().max())
    return top if c["regime"] in ("cancel", "f16_domain") else max(1.0, top)


def bar(c, t, ref=None):
    """(the absolute bar of the row on the tensors t, the emulation's own absolute distance from float64): 4x that distance, over all
    problems.  No kernel has a say in it."""
    ref = ref or cc.reference(c, t)
    own = max(float((e.double() - r).abs().max()) for e, r in zip(emulate(c, t), ref["y"]))
    return MARGIN * own, own
