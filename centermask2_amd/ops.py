"""Thin host wrappers: torch tensors (device memory, current stream) -> C ABI calls of libcmk_hip.so.

PyTorch is plumbing here (allocation, streams); the arithmetic happens in the HIP kernels.  Activations are
NHWC float32; `View` is (NHWC tensor, channel offset, channels) so producers write straight into slices of
an OSA concat buffer.  Every function raises if the tensors are not on a GPU — there is no CPU fallback.
"""
import ctypes
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ConvDesc, FcosLevel, check


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.CmkError("{}: tensor is on {}; the CenterMask2 HIP path needs a GPU (no CPU fallback)".format(what, t.device))
    if t.dtype != torch.float32:
        raise _lib.CmkError("{}: expected float32, got {}".format(what, t.dtype))
    _need_current_device(t, what)


def _need_current_device(t: torch.Tensor, what: str) -> None:
    """The library launches on the stream it is handed — torch's CURRENT stream, i.e. the current device's.  A tensor of another
    device would be read through a stream (and split-K / GroupNorm workspaces) of the wrong GPU: refuse instead of faulting."""
    cur = torch.cuda.current_device()
    if t.device.index is not None and t.device.index != cur:
        raise _lib.CmkError("{}: tensor lives on cuda:{} but the current device is cuda:{}; wrap the call in "
                            "`with torch.cuda.device({})` (one process per GPU is the supported layout)".format(what, t.device.index, cur, t.device.index))


def _need_dense_nhwc(t: torch.Tensor, what: str) -> None:
    """The entry points that take a bare pointer and (N, HW, C) read the tensor as dense NHWC: a permuted or sliced view would be
    normalised along the wrong axis without a word."""
    if t.dim() != 4 or not t.is_contiguous():
        raise _lib.CmkError("{}: expected a dense (contiguous) 4-d NHWC tensor, got shape {} strides {}".format(what, tuple(t.shape), tuple(t.stride())))
    _need_gpu(t, what)


def _need_gate(gate: torch.Tensor, n: int, c: int, like: torch.Tensor, what: str) -> None:
    """An eSE gate is read as N * C consecutive floats on the device of the map it scales."""
    if tuple(gate.shape) != (n, c) or not gate.is_contiguous():
        raise _lib.CmkError("{}: the gate must be a contiguous ({}, {}) tensor, got shape {} strides {}".format(what, n, c, tuple(gate.shape), tuple(gate.stride())))
    if gate.dtype != torch.float32 or gate.device != like.device:
        raise _lib.CmkError("{}: the gate must be float32 on {}, got {} on {}".format(what, like.device, gate.dtype, gate.device))


def _need_same_geometry(v: "View", n: int, h: int, w: int, c: int, like: torch.Tensor, what: str) -> None:
    if v.nhw != (n, h, w) or v.c != c:
        raise _lib.CmkError("{}: expected a view of ({}, {}, {}) pixels x {} channels, got {} x {}".format(what, n, h, w, c, tuple(v.nhw), v.c))
    if v.t.dtype != torch.float32 or v.t.device != like.device:
        raise _lib.CmkError("{}: expected float32 on {}, got {} on {}".format(what, like.device, v.t.dtype, v.t.device))


class View:
    """Channel slice [co, co+c) of a contiguous NHWC tensor (N,H,W,CS)."""
    __slots__ = ("t", "co", "c")

    def __init__(self, t: torch.Tensor, co: int = 0, c: Optional[int] = None):
        assert t.dim() == 4 and t.is_contiguous(), "View needs a contiguous (N,H,W,C) tensor"
        self.t = t
        self.co = co
        self.c = t.shape[3] - co if c is None else c
        assert 0 <= co and co + self.c <= t.shape[3]

    @property
    def cs(self) -> int:
        return self.t.shape[3]

    @property
    def nhw(self) -> Tuple[int, int, int]:
        return self.t.shape[0], self.t.shape[1], self.t.shape[2]

    def nchw(self) -> torch.Tensor:
        """Logical (N,C,H,W) view with channels_last strides (what the plugin API hands to callers)."""
        return self.t[..., self.co:self.co + self.c].permute(0, 3, 1, 2)


def as_view(x) -> "View":
    """Accept a View, an NHWC-contiguous 4-D tensor wrapped earlier, or a logical NCHW tensor (made channels_last)."""
    if isinstance(x, View):
        return x
    assert x.dim() == 4
    nhwc = x.permute(0, 2, 3, 1)
    if not nhwc.is_contiguous():
        nhwc = nhwc.contiguous()
    return View(nhwc)


# ---------------------------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------------------------
def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """(Cout,Cin,k,k) -> [tap][Cin/16][cout_pad][16] (zero padded), the layout conv_igemm.hip streams."""
    lib = _lib.load()
    cout, cin, k, _ = w.shape
    cin_pad = (cin + 15) // 16 * 16
    cout_pad = lib.cmk_conv_cout_pad(cout)
    wp = torch.zeros((k * k, cin_pad, cout_pad), dtype=torch.float32)
    wp[:, :cin, :cout] = w.detach().float().cpu().permute(2, 3, 1, 0).reshape(k * k, cin, cout)
    wp = wp.reshape(k * k, cin_pad // 16, 16, cout_pad).permute(0, 1, 3, 2).contiguous()
    assert wp.numel() == lib.cmk_conv_packed_floats(cout, cin, k)
    return wp


_WINO_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


def _wino_u(w: torch.Tensor) -> torch.Tensor:
    """(Cout,Cin,3,3) -> U = G g G^T as [chunk][ntile][16 freq in step order][64 co][16 ci] (float64 transform, rounded once)."""
    cout, cin = w.shape[0], w.shape[1]
    u = torch.einsum("ik,ockl,jl->ocij", _WINO_G, w.detach().double().cpu(), _WINO_G).reshape(cout, cin, 16)
    cin_pad, nt = (cin + 15) // 16 * 16, (cout + 63) // 64
    up = torch.zeros((cin_pad, nt * 64, 16), dtype=torch.float64)
    up[:cin, :cout] = u.permute(1, 0, 2)
    order = [f for g in range(4) for f in (2 * g, 2 * g + 1, 8 + 2 * g, 9 + 2 * g)]      # the kernels' streaming order
    up = up[:, :, order]
    return up.reshape(cin_pad // 16, 16, nt, 64, 16).permute(0, 2, 4, 3, 1).contiguous().float()


def pack_wino_weight(w: torch.Tensor) -> torch.Tensor:
    """Packed U for the Winograd kernel (cmk_conv_desc.w_wino):
    [chunk][ntile][step 4][fh 2][ng 2][fl 2][piece 2][lane = 32*hh + li][4] with freq = step*4 + fh*2 + fl (step order),
    co = ng*32 + li, ci = 8*hh + 4*piece + j — every operand load of a wave is one contiguous KiB."""
    lib = _lib.load()
    up = _wino_u(w)
    nc, nt = up.shape[0], up.shape[1]
    r = up.reshape(nc, nt, 4, 2, 2, 2, 32, 2, 2, 4)               # [chunk][nt][g][fh][fl][ng][li][hh][piece][j]
    r = r.permute(0, 1, 2, 3, 5, 4, 8, 7, 6, 9).contiguous().reshape(nc, nt, 16, 64, 16)
    assert r.numel() == lib.cmk_wino_packed_floats(w.shape[0], w.shape[1])
    return r


_WINO6_G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                        dtype=torch.float64)


def pack_wino6_weight(w: torch.Tensor) -> torch.Tensor:
    """Packed U = G g G^T of the Winograd F(4x4,3x3) kernel (cmk_conv_desc.w_wino6; float64 transform, rounded once):
    [Cin/8][ceil(Cout/32)][wave 4][slot 9][lane = 32*hh + li][4] — slot k < 6: frequency (wave, k); k >= 6: (4 + wave//2, 3*(wave%2) + k - 6);
    co = tile*32 + li, ci = chunk*8 + 4*hh + j — every operand load of a wave is one contiguous KiB."""
    lib = _lib.load()
    cout, cin = w.shape[0], w.shape[1]
    u = torch.einsum("ik,ockl,jl->ocij", _WINO6_G, w.detach().double().cpu(), _WINO6_G)              # (O, C, 6, 6)
    cin_pad, nt = (cin + 15) // 16 * 16, (cout + 31) // 32       # the same channel padding as the direct layout (PackedConv.cin_pad)
    up = torch.zeros((nt * 32, cin_pad, 6, 6), dtype=torch.float64)
    up[:cout, :cin] = u
    fa = torch.tensor([[wv if k < 6 else 4 + wv // 2 for k in range(9)] for wv in range(4)])
    fb = torch.tensor([[k if k < 6 else 3 * (wv % 2) + k - 6 for k in range(9)] for wv in range(4)])
    sel = up[:, :, fa, fb]                                                                               # (O, C, 4 waves, 9 slots)
    r = sel.reshape(nt, 32, cin_pad // 8, 2, 4, 4, 9)                                                    # [tile][li][chunk][hh][j][wave][slot]
    r = r.permute(2, 0, 5, 6, 3, 1, 4).contiguous().float()                                             # [chunk][tile][wave][slot][hh][li][j]
    assert r.numel() == lib.cmk_wino6_packed_floats(cout, cin_pad)
    return r.reshape(cin_pad // 8, nt, 4, 9, 64, 4)


def pack_split_weight(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin[,1,1]) fp32 -> the bf16-split packing of cmk_conv_desc.w_split (opt-in tune_wm 10): every weight as three bf16 values
    hi + mid + lo (round to nearest even, exact to 2^-24), laid out [Cin/16][cout_pad/32][piece][lane = 32*hh + li][8]:
    input channel 16*chunk + 8*hh + e of output channel 32*tile + li; cout_pad = Cout rounded up to 128, zero filled."""
    lib = _lib.load()
    if w.dim() == 4 and w.shape[2] == 3:          # 3x3 conv in the gather form: K walks the taps (kh, kw) outermost, then the padded input channels
        cout, cin = w.shape[0], w.shape[1]
        cin_pad1 = (cin + 15) // 16 * 16
        wk = torch.zeros((cout, 9, cin_pad1), dtype=torch.float32)
        wk[:, :, :cin] = w.detach().float().cpu().permute(0, 2, 3, 1).reshape(cout, 9, cin)
        w2 = wk.reshape(cout, 9 * cin_pad1)
        taps = 9
    else:
        w2 = w.detach().float().cpu().reshape(w.shape[0], w.shape[1])
        taps = 1
    cout, cin = w2.shape
    cin_pad, cout_pad = (cin + 15) // 16 * 16, (cout + 127) // 128 * 128
    full = torch.zeros((cout_pad, cin_pad), dtype=torch.float32)
    full[:cout, :cin] = w2
    pieces, rest = [], full
    for _ in range(3):
        p = rest.to(torch.bfloat16)
        pieces.append(p)
        rest = rest - p.float()
    st = torch.stack(pieces, 0)                                                    # (3, cout_pad, cin_pad)
    r = st.reshape(3, cout_pad // 32, 32, cin_pad // 16, 2, 8)                      # [piece][tile][li][chunk][hh][e]
    r = r.permute(3, 1, 0, 4, 2, 5).contiguous()                                   # [chunk][tile][piece][hh][li][e]
    assert r.numel() == taps * lib.cmk_split_packed_halves(cout, cin_pad // taps)
    return r.reshape(cin_pad // 16, cout_pad // 32, 3, 64, 8)


def pack_splith_weight(w: torch.Tensor):
    """(Cout, Cin, k, k) fp32, k = 1 | 3 -> (the fp16 two-piece packing of cmk_conv_desc.w_splith, 1 / S_w) for the opt-in fp16-split forms (tune_wm 11, 12):
    w' = w * S_w with S_w the power of two that puts max |w'| in [2^14, 2^15); pieces h = fp16(w'), m = fp16(w' - h) (the residual is exact in
    fp32); laid out [tap][Cin/16][cout_pad/32][piece][lane = 32*hh + li][8]: input channel 16*chunk + 8*hh + e of output channel 32*tile + li;
    cout_pad = Cout rounded up to 128, zero filled."""
    import math
    lib = _lib.load()
    cout, cin = w.shape[0], w.shape[1]
    cin_pad, cout_pad = (cin + 15) // 16 * 16, (cout + 127) // 128 * 128
    wf = w.detach().float().cpu()
    amax = float(wf.abs().max())
    s_w = 2.0 ** (14 - math.floor(math.log2(amax))) if amax > 0 and math.isfinite(amax) else 1.0
    taps = w.shape[2] * w.shape[3] if w.dim() == 4 else 1
    full = torch.zeros((cout_pad, taps, cin_pad), dtype=torch.float32)
    full[:cout, :, :cin] = wf.reshape(cout, cin, taps).permute(0, 2, 1) * s_w
    h = full.to(torch.float16)
    m = (full - h.float()).to(torch.float16)
    st = torch.stack([h, m], 0)                                                     # (2, cout_pad, taps, cin_pad)
    r = st.reshape(2, cout_pad // 32, 32, taps, cin_pad // 16, 2, 8)                # [piece][tile][li][tap][chunk][hh][e]
    r = r.permute(3, 4, 1, 0, 5, 2, 6).contiguous()                                 # [tap][chunk][tile][piece][hh][li][e]
    assert r.numel() == taps * lib.cmk_splith_packed_halves(cout, cin_pad)
    return r.reshape(taps, cin_pad // 16, cout_pad // 32, 2, 64, 8), 1.0 / s_w


class PackedConv:
    """Device-resident packed weights + per-channel epilogue (scale, shift) of one conv / linear layer."""

    def __init__(self, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor], device,
                 stride: int = 1):
        if weight.dim() == 2:
            weight = weight[:, :, None, None]
        self.cout, self.cin, self.k, _ = weight.shape
        self.cin_pad = (self.cin + 15) // 16 * 16
        self.stride = stride
        self.w = pack_conv_weight(weight).to(device)
        self.w_wino = pack_wino_weight(weight).to(device) if (self.k == 3 and stride == 1 and self.cin >= 16) else None
        # F(4x4,3x3) weights: 4x the 3x3 filter bank; packed for every conv that can use them (PACK_WINO6 = False skips it)
        self.w_wino6 = pack_wino6_weight(weight).to(device) if (PACK_WINO6 and self.k == 3 and stride == 1 and self.cin >= 32) else None
        # opt-in (ALLOW_SPLIT_BF16): the bf16-split packing for the pointwise GEMM's fp32-accurate split form (cmk.h tune_wm 10)
        self.w_split = pack_split_weight(weight).to(device) if (ALLOW_SPLIT_BF16 and self.cin_pad % 32 == 0 and (
            (self.k == 1 and self.cout > 224) or (self.k == 3 and (self.cout > 224 or 96 < self.cout <= 128)))) else None
        # opt-in (ALLOW_SPLIT_F16): the fp16 two-piece packing for the direct 3x3 form (cmk.h tune_wm 11)
        self.w_splith, self.w_splith_scale = None, 0.0
        if ALLOW_SPLIT_F16 and self.cin >= 32 and (self.k == 3 or (self.k == 1 and self.cout > 224 and self.cin_pad % 32 == 0)):
            wh_, self.w_splith_scale = pack_splith_weight(weight)
            self.w_splith = wh_.to(device)
        self.scale = (torch.ones(self.cout) if scale is None else scale.detach().float().cpu()).contiguous().to(device)
        self.shift = (torch.zeros(self.cout) if shift is None else shift.detach().float().cpu()).contiguous().to(device)


def fold_frozen_bn(weight, bias, running_mean, running_var, eps=1e-5):
    """FrozenBN as a per-channel epilogue: y = conv * scale + shift (d2 FrozenBatchNorm2d, eps 1e-5)."""
    scale = weight.double() / torch.sqrt(running_var.double() + eps)
    shift = bias.double() - running_mean.double() * scale
    return scale.float(), shift.float()


def _out_hw(h: int, w: int, stride: int) -> Tuple[int, int]:
    """Output size of a conv here: 'same' padding, stride 1 or 2."""
    return (h, w) if stride == 1 else ((h - 1) // 2 + 1, (w - 1) // 2 + 1)


def _fill_desc(d: ConvDesc, x: View, pc: PackedConv, y: View, relu, relu_upto, res, res_upsample, in_relu, in_affine=None) -> None:
    _need_gpu(x.t, "conv2d")
    n, h, w = x.nhw
    d.x, d.x_cs, d.x_co = x.t.data_ptr(), x.cs, x.co
    d.w = pc.w.data_ptr()
    d.w_wino = pc.w_wino.data_ptr() if getattr(pc, "w_wino", None) is not None else None
    d.w_wino6 = pc.w_wino6.data_ptr() if getattr(pc, "w_wino6", None) is not None else None
    d.w_split = pc.w_split.data_ptr() if getattr(pc, "w_split", None) is not None else None
    d.w_splith = pc.w_splith.data_ptr() if getattr(pc, "w_splith", None) is not None else None
    d.w_splith_scale = float(getattr(pc, "w_splith_scale", 0.0))
    d.scale, d.shift = pc.scale.data_ptr(), pc.shift.data_ptr()
    if res is not None:
        d.res, d.res_cs, d.res_co = res.t.data_ptr(), res.cs, res.co
        d.res_mode = 2 if res_upsample else 1
        d.Hr, d.Wr = res.t.shape[1], res.t.shape[2]
    else:
        d.res, d.res_mode = None, 0
    d.y, d.y_cs, d.y_co = y.t.data_ptr(), y.cs, y.co
    d.N, d.H, d.W, d.Cin, d.Cout = n, h, w, pc.cin_pad, pc.cout
    assert x.c == pc.cin_pad, "conv2d: input view has {} channels, packed weights expect {}".format(x.c, pc.cin_pad)
    assert y.c == pc.cout
    assert tuple(y.t.shape[:3]) == (n,) + _out_hw(h, w, pc.stride), (tuple(y.t.shape), (n,) + _out_hw(h, w, pc.stride))
    d.ksize, d.stride = pc.k, pc.stride
    d.relu_upto = (pc.cout if relu else 0) if relu_upto is None else relu_upto
    d.in_relu = int(in_relu)
    if in_affine is not None:
        d.in_scale, d.in_shift = in_affine[0].data_ptr(), in_affine[1].data_ptr()
    else:
        d.in_scale = d.in_shift = None


# ---- tile-variant autotuning (host side; the library itself stays stateless) -----------------------------------
FUSE_POOL = os.environ.get("CMK_FUSE_POOL", "1") != "0"      # eSE: average-pool partial sums from the aggregation conv's epilogue (A/B switch)
PAIR_TOWERS = os.environ.get("CMK_PAIR_TOWERS", "1") != "0"  # FCOS head: conv k of the cls and the bbox tower in one launch (A/B switch)
ALLOW_SPLIT_BF16 = os.environ.get("CMK_ALLOW_SPLIT_BF16", "0") == "1"   # OPT-IN: pack the bf16-split weights and let the tuner / tables use the
                          # pointwise GEMM's split form (fp32-accurate products from bf16 pieces, cmk.h tune_wm 10).  Off: nothing in the package uses it.
ALLOW_SPLIT_F16 = os.environ.get("CMK_ALLOW_SPLIT_F16", "0") == "1"   # OPT-IN: pack the fp16 two-piece weights and let the tuner / tables use the direct
                          # 3x3 form on fp16-split products (cmk.h tune_wm 11, conv_sp3.hip: 22-bit operands, three products, fp32 accumulation —
                          # the error of an fp32 accumulation).  Off: nothing in the package uses it.
PACK_WINO6 = True         # pack the F(4x4,3x3) weights too (4x the filter bank per 3x3 stride-1 conv)
ALLOW_WINOGRAD = True     # let the tuner pick the Winograd F(2x2,3x3) kernel where it is faster (fp32, differs by rounding only)
TUNE_LOG = []             # (key, {candidate: ms}) per tuned problem
TAIL_TILES = 0            # tests: the tile count of a variant's tail split-K (cmk.h splitk_tail_tiles); 0 = the library's plan for the device
FORCE_VARIANT = None      # (wm, sc, wn[, splitk[, tail ways]]) for every conv launched through the wrappers below (tests); None = table/tuner/default
TUNE_ONLY = None          # callable(key) -> [(wm, sc, wn, splitk), ...]: the tuner's candidates for that problem instead of the whole menu (targeted
                          # re-tuning: tools/tune_sp3.py); TUNE_REPS timed launches per candidate, best of TUNE_ROUNDS interleaved rounds
TUNE_REPS, TUNE_ROUNDS = 2, 1
AUTOTUNE = False          # when True, the first call of every distinct conv problem times the variant menu (needs an idle, non-capturing stream)
_TUNED = {}               # problem key -> plain tuple, Variant.stored(): (wm, sc, wn[, splitk[, tail ways]])


def set_autotune(flag: bool) -> None:
    global AUTOTUNE
    AUTOTUNE = bool(flag)


def tuned_variants() -> dict:
    return dict(_TUNED)


def _key_to_str(key) -> str:
    k, stride, cin, cout, xcs, ycs, res, shapes = key
    return "k{}s{}_cin{}_cout{}_xcs{}_ycs{}_res{}_".format(k, stride, cin, cout, xcs, ycs, res) + "+".join("{}x{}x{}".format(*s) for s in shapes)


def _str_to_key(s: str):
    head, shapes = s.rsplit("_", 1)
    f = head.split("_")
    k, stride = f[0][1:].split("s")
    vals = [int(f[1][3:]), int(f[2][4:]), int(f[3][3:]), int(f[4][3:]), int(f[5][3:])]
    return (int(k), int(stride), vals[0], vals[1], vals[2], vals[3], vals[4], tuple(tuple(int(v) for v in t.split("x")) for t in shapes.split("+")))


class Variant(NamedTuple):
    """A tile variant, canonical: tune_wm / tune_sc / tune_wn of cmk_conv_desc, split-K ways (1 = none), tail split-K ways (cmk.h splitk_tail; 0 = off)."""
    wm: int
    sc: int
    wn: int
    splitk: int = 1
    tail: int = 0

    @classmethod
    def of(cls, tv) -> "Variant":
        """From any accepted spelling: (wm, sc, wn[, splitk[, tail]]) as a tuple, a JSON list or a Variant; tail ways 0 and 1 both mean off."""
        wm, sc, wn, splitk, tail = (tuple(tv) + (1, 0))[:5]
        return cls(wm, sc, wn, splitk, int(tail) if tail > 1 else 0)

    def stored(self, least: int = 3) -> tuple:
        """The plain tuple _TUNED holds and save_tuned writes: (wm, sc, wn), (wm, sc, wn, splitk) or, with a tail, all five (least = 4: TUNE_LOG's names)."""
        return tuple(self) if self.tail else tuple(self[:max(least, 4 if self.splitk != 1 else 3)])


def _variant5(tv) -> tuple:
    """(wm, sc, wn[, splitk[, tail]]) -> (wm, sc, wn, splitk) or, with a tail, (wm, sc, wn, splitk, tail): a candidate's name in TUNE_LOG."""
    return Variant.of(tv).stored(4)


def save_tuned(path: str) -> None:
    """Write the measured variant table (problem -> [wm, sc, wn[, splitk[, tail ways]]]) as JSON; shipped tables live in centermask2_amd/tuned/."""
    import json
    with open(path, "w") as f:
        json.dump({_key_to_str(k): list(v) for k, v in sorted(_TUNED.items(), key=lambda kv: _key_to_str(kv[0]))}, f, indent=0)


def _variant_on_menu(tv) -> bool:
    """(wm, sc, wn[, splitk[, tail]]) names a kernel this library has (older tables may carry variants that were removed since)."""
    wm, sc, wn, sk, tail = Variant.of(tv)
    if tail and not (wm == 6 and sc in (16, 32) and wn == 2 and sk == 1 and tail in (2, 4, 8)):
        return False                  # the tail is a feature of the RoI-pair F(4x4) forms alone
    if wm == 6 and sc == 64:          # F(4x4,3x3), shared-V form (conv_wino6s.hip)
        return wn in (1, 2) and sk == 1
    if wm == 6:                       # F(4x4,3x3): 32 couts per workgroup (sc 16) or the paired form (sc 32, conv_wino6p_kernel)
        return sc in (16, 32) and wn in (1, 2) and sk in (1, 2, 4, 8)
    if wm == 10:                      # pointwise GEMM from bf16-split products: only where the caller opted in
        return ALLOW_SPLIT_BF16 and sc == 32 and wn == 4 and sk == 1
    if wm == 12:                      # pointwise GEMM from fp16-split products (two pieces, three products)
        return ALLOW_SPLIT_F16 and sc == 32 and wn == 4 and sk == 1
    if wm == 11:                      # direct 3x3 conv from bf16-split products (conv_sp3.hip): sc = pieces, wn = geometry
        return ALLOW_SPLIT_F16 and sc in (2, 21) and 0 <= wn <= 3 and sk == 1
    return (wm in (1, 2, 5, 6, 7, 8, 9) and sc in (16, 32) and 1 <= wn <= 7 and sk in (1, 2, 4, 8)) or (wm, sc, wn) == (0, 0, 0)


def load_tuned(path: str) -> int:
    """Read a measured variant table; entries naming a variant that is not on the menu are dropped (that problem falls back to the
    library default / the start-up tuner), so a stale table cannot break a run."""
    import json
    with open(path) as f:
        table = json.load(f)
    n = 0
    for k, v in table.items():
        if _variant_on_menu(v):
            _TUNED[_str_to_key(k)] = tuple(v)
            n += 1
    return n


def _out_pixels(d) -> int:
    ho, wo = _out_hw(d.H, d.W, d.stride)
    return d.N * ho * wo


def _set_variant(descs, n, tv, tail_tiles=None, dummy=None):
    """Write a variant (any spelling) into the descriptors; returns the split-K (or tail) workspace (keep it alive until the launch).
    tail_tiles: the tile count of a tail (cmk.h splitk_tail_tiles); None = TAIL_TILES.  dummy: the address that stands for every
    workspace of descriptors that are planned and never launched (_ConvLaunch.planned); nothing is allocated."""
    wm, sc, wn, sk, tail = Variant.of(tv)
    for i in range(n):
        descs[i].tune_wm, descs[i].tune_sc, descs[i].tune_wn = wm, sc, wn
        descs[i].splitk, descs[i].splitk_ws = 0, None
        descs[i].splitk_tail, descs[i].splitk_tail_tiles = 0, 0
    ws = None
    if dummy is not None:
        d = descs[0]
        if tail:
            d.splitk_tail, d.splitk_tail_tiles, d.splitk_ws = tail, TAIL_TILES if tail_tiles is None else tail_tiles, dummy
        if sk > 1:
            d.splitk, d.splitk_ws = sk, dummy
        return None
    if tail:
        d = descs[0]
        d.splitk_tail, d.splitk_tail_tiles = tail, TAIL_TILES if tail_tiles is None else tail_tiles
        floats = _lib.load().cmk_conv_tail_ws_floats(ctypes.byref(d))      # 0: no ragged round on this device, the launch runs without a tail
        if floats > 0:
            ws = torch.empty((floats,), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
            d.splitk_ws = ws.data_ptr()
    if sk > 1:
        d = descs[0]
        ws = torch.empty((sk * _out_pixels(d) * _lib.load().cmk_conv_cout_pad(d.Cout),), dtype=torch.float32,
                         device=torch.device("cuda", torch.cuda.current_device()))       # == the inputs' device (_need_current_device)
        d.splitk, d.splitk_ws = sk, ws.data_ptr()
    return ws


def _problem_key(descs, n):
    d = descs[0]
    # res slot: 0/1/2 = residual mode, +4 when the fused input affine is on (restricts the variants that may be chosen)
    return (d.ksize, d.stride, d.Cin, d.Cout, d.x_cs, d.y_cs, d.res_mode + (4 if d.in_scale else 0),
            tuple((descs[i].N, descs[i].H, descs[i].W) for i in range(n)))


def _plan(descs, n):
    """(kernel name, executed FLOPs, {sum, sumsq} records per image of each problem) of the launch of these filled descriptors, from the
    library's launchers (cmk_conv_plan); gn_groups without a gn_ws asks for the launch as with fused GroupNorm statistics."""
    name, flops, recs = ctypes.create_string_buffer(96), ctypes.c_double(), (ctypes.c_int * n)()
    check(_lib.load().cmk_conv_plan(descs, n, name, len(name), ctypes.byref(flops), recs), "cmk_conv_plan")
    return name.value.decode(), flops.value, list(recs)


class _ConvLaunch:
    """One conv launch of the wrappers below and of the tuner: the descriptors of problems (xs[i], pcs[i]) -> ys[i], the variant written into them, the
    split-K (or tail) workspace, which lives as long as this object, and the entry they go through (cmk_conv2d_nhwc if single, else the _multi one)."""

    def __init__(self, xs, pcs, ys, relu=False, relu_upto=None, res=None, res_upsample=False, in_relu=False, in_affine=None, single=False):
        self.xs, self.pcs, self.ys, self.n, self.single, self.ws, self.dummy = xs, pcs, ys, len(xs), single, None, None
        self.descs = (ConvDesc * self.n)()
        for i in range(self.n):
            _fill_desc(self.descs[i], xs[i], pcs[i], ys[i], relu, relu_upto, res, res_upsample, in_relu, in_affine[i] if in_affine is not None else None)

    @classmethod
    def planned(cls, shapes, cin, cout, k, stride=1, relu=False, res_mode=0, in_affine=False, single=False) -> "_ConvLaunch":
        """The launch of problems known by their shapes [(N, H, W)] alone, for _plan and cmk_conv_resolve on a machine without a GPU: dense
        views, every packing on offer, and one dummy aligned address for every pointer, which the library's front door never follows.
        set() and gn_stats() work as on a real launch; run() is refused."""
        self = cls.__new__(cls)
        self.xs = self.pcs = self.ys = self.ws = None
        self.n, self.single = len(shapes), single
        self._buf = (ctypes.c_float * 64)()
        self.dummy = ptr = (ctypes.addressof(self._buf) + 15) // 16 * 16
        self.descs = (ConvDesc * self.n)()
        cin_pad = (cin + 15) // 16 * 16
        for d, (n, h, w) in zip(self.descs, shapes):
            d.x = d.w = d.scale = d.shift = d.y = d.w_wino = d.w_wino6 = d.w_split = d.w_splith = ptr
            d.w_splith_scale = 1.0
            d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = n, h, w, cin_pad, cout, k, stride
            d.x_cs, d.y_cs, d.relu_upto = cin_pad, cout, cout if relu else 0
            d.res_mode = res_mode
            if res_mode:
                ho, wo = _out_hw(h, w, stride)
                d.res, d.res_cs, d.Hr, d.Wr = ptr, cout, (ho, (ho + 1) // 2)[res_mode - 1], (wo, (wo + 1) // 2)[res_mode - 1]
            if in_affine:
                d.in_scale = d.in_shift = ptr
        return self

    def set(self, v) -> None:
        self.ws = _set_variant(self.descs, self.n, v, dummy=self.dummy)

    def gn_stats(self, groups: int):
        """Ask the kernel of the variant that is set for the fused statistics of a GroupNorm over its outputs (_gn_records: the affine
        to call after the launch, or None where that kernel writes none).  A planned launch only puts the question (gn_groups, no workspace)."""
        if self.dummy is None:
            return _gn_records(self.descs, self.ys, groups)
        for i in range(self.n):
            self.descs[i].gn_groups = groups
        return None

    def choose(self, first=None, with_gn_stats=False) -> Variant:
        """Write an explicit variant into the descriptors and return it: FORCE_VARIANT, else the loaded table, else the start-up tuner, else
        the split-K default, with zero tune fields made explicit by the library (cmk_conv_resolve; with_gn_stats: as for a launch with fused
        GroupNorm statistics).  first = k: the first k problems alone name the problem and get the variant, and nothing is tuned."""
        descs, k = self.descs, self.n if first is None else first
        key = _problem_key(descs, k)
        tv = FORCE_VARIANT if FORCE_VARIANT is not None else _TUNED.get(key)
        if tv is None and first is None and AUTOTUNE and not torch.cuda.is_current_stream_capturing():
            _tune(self, key)
            tv = _TUNED[key]
        if tv is None:
            tv = _default_variant(descs[0]) if k == 1 else (0, 0, 0)
        v = Variant.of(tv)
        self.ws = _set_variant(descs, k, v)
        if v[:3] == (0, 0, 0):
            r = (ctypes.c_int * 3)()
            check(_lib.load().cmk_conv_resolve(descs, k, int(with_gn_stats), r), "cmk_conv_resolve")
            for i in range(k):
                descs[i].tune_wm, descs[i].tune_sc, descs[i].tune_wn = r
            v = v._replace(wm=r[0], sc=r[1], wn=r[2])
        return v

    def run(self) -> int:
        if self.dummy is not None:
            raise _lib.CmkError("a planned conv launch has no buffers: it can be planned, not run")
        lib = _lib.load()
        return lib.cmk_conv2d_nhwc(ctypes.byref(self.descs[0]), _stream()) if self.single else lib.cmk_conv2d_nhwc_multi(self.descs, self.n, _stream())

    def launch(self, what=None) -> None:
        """run(), checked.  When PROFILE is a list, the launch is timed and recorded under the kernel the library says it runs."""
        what = what or ("cmk_conv2d_nhwc" if self.single else "cmk_conv2d_nhwc_multi")
        if PROFILE is None:
            return check(self.run(), what)
        xs, ys, pcs, pc = self.xs, self.ys, self.pcs, self.pcs[0]
        kernel, executed, _ = _plan(self.descs, self.n)
        taps = pc.k * pc.k
        pix = lambda v: v.t.shape[0] * v.t.shape[1] * v.t.shape[2]
        flops = sum(2.0 * pix(y) * pc.cin * pc.cout * taps for y in ys)
        weights = len({p.w.data_ptr() for p in pcs})          # read once per launch each
        nbytes = sum(4.0 * (pix(x) * pc.cin + pix(y) * pc.cout) for x, y in zip(xs, ys)) + weights * 4.0 * pc.cin * pc.cout * taps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(self.run(), what)
        e1.record()
        shape = tuple(xs[0].nhw) + (pc.cin, pc.cout, pc.k, pc.stride) if self.single else None
        PROFILE.append((kernel, flops, nbytes, e0, e1, shape, executed))


def _tune(launch: _ConvLaunch, key) -> None:
    """Time every available variant on the real buffers and remember the fastest.  The direct variants (incl. the gather form and
    split-K, whose K order is unchanged up to the final sum) agree to rounding; variants the library rejects for this shape are skipped."""
    n, d0 = launch.n, launch.descs[0]
    small = n == 1 and d0.res_mode != 2 and _out_pixels(d0) <= 32768      # few M tiles: split-K / gather forms can pay
    sks = (1, 2, 4, 8) if small else (1,)
    cands = [(wm, sc, wn, sk) for wn in range(1, 8) for wm in (1, 2) for sc in (16, 32) for sk in sks]
    if small and d0.ksize == 3:
        cands += [(7, 32, wn, sk) for wn in (1, 2, 4) for sk in sks]      # gather form
    if d0.ksize in (1, 3):
        # pointwise GEMM kernel (conv_pw.hip), 256- or 128-pixel workgroups: a 1x1 conv (8; same K order, same bits) or the gather form of a 3x3 conv (9, GA)
        cands += [(8 if d0.ksize == 1 else 9, 32, mt, sk) for mt in (4, 2) for sk in sks]
        if ALLOW_SPLIT_BF16:
            cands += [(10, 32, 4, 1)]                               # ... its opt-in bf16-split form (the library refuses it where it does not apply)
        if ALLOW_SPLIT_F16:
            cands += [(12, 32, 4, 1)]                               # ... its opt-in fp16-split form (two pieces, three products)
        if ALLOW_SPLIT_F16 and d0.ksize == 3:                       # opt-in: direct 3x3 on two fp16 pieces per operand (conv_sp3.hip), four tile geometries,
            cands += [(11, sc, g, 1) for sc in (2, 21) for g in range(4)]      # two cout tiles per wave or one (21: less cout padding, more and smaller workgroups)
    if ALLOW_WINOGRAD:
        cands += [(5, 16, 2, 1)]                  # fused Winograd F(2x2,3x3)
        cands += [(6, 16, 1, 1), (6, 16, 2, 1)]   # fused Winograd F(4x4,3x3): map tiles / pairs of RoI maps (the library rejects what does not apply)
        cands += [(6, 64, 1, 1), (6, 64, 2, 1)]   # ... its shared-V form: 64 couts per workgroup from one frequency image (conv_wino6s.hip)
        cands += [(6, 32, 1, 1), (6, 32, 2, 1)]   # ... its paired form: 64 couts per workgroup sharing the halo loads and pass 1
        if n == 1 and d0.ksize == 3:
            for sc in (16, 32):                   # ... the RoI-pair forms with the ragged last round of workgroups split over K, where there is one
                launch.set((6, sc, 2, 1, 2))
                if _lib.load().cmk_conv_tail_ws_floats(ctypes.byref(d0)) > 0:
                    cands += [(6, sc, 2, 1, t) for t in (2, 4, 8)]
        if small and d0.ksize == 3:
            cands += [(6, sc, 1, sk) for sc in (16, 32) for sk in (2, 4)]      # ... with the chunk loop split over 2 / 4 workgroups (launches of about one round)
    if TUNE_ONLY is not None:
        cands = TUNE_ONLY(key)
    cands = [Variant.of(tv) for tv in cands]
    times = {}
    for _ in range(TUNE_ROUNDS):
        for v in cands:
            if times.get(v) == float("inf"):
                continue
            launch.set(v)
            if launch.run() != 0:
                times[v] = float("inf")           # not on the menu for this shape
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _r in range(TUNE_REPS):
                launch.run()
            e1.record()
            e1.synchronize()
            times[v] = min(times.get(v, float("inf")), e0.elapsed_time(e1) / TUNE_REPS)
    best, best_ms = Variant(0, 0, 0), float("inf")
    for v in cands:                               # first of equals wins, as before
        if times.get(v, float("inf")) < best_ms:
            best, best_ms = v, times[v]
    _TUNED[key] = best.stored()
    TUNE_LOG.append((key, {v.stored(4): times[v] for v in cands if v in times}))


def _default_variant(d) -> Variant:
    """No table entry and no tuner: library defaults, plus split-K for skinny 1x1 GEMMs (maskiou_fc1: 400 x 12544 x 1024)."""
    if d.ksize == 1 and d.res_mode != 2 and _out_pixels(d) <= 1024 and d.Cin >= 4096:
        chunks = d.Cin // 16
        for sk in (4, 2):
            if chunks % (2 * sk) == 0:
                return Variant(0, 0, 0, sk)
    return Variant(0, 0, 0)


def _new_outputs(xs: Sequence[View], pc: PackedConv) -> List[View]:
    return [View(torch.empty((x.t.shape[0],) + _out_hw(x.t.shape[1], x.t.shape[2], pc.stride) + (pc.cout,), dtype=torch.float32, device=x.t.device)) for x in xs]


def conv2d(x: View, pc: PackedConv, y: View, relu: bool = False, relu_upto: Optional[int] = None,
           res: Optional[View] = None, res_upsample: bool = False, in_relu: bool = False, pool: Optional[list] = None) -> None:
    """pool: a list that receives (partial sums, rows per record) when the kernel this conv runs on also leaves the average-pool partial
    sums of its output behind (cmk_conv_desc.pool_ws: the pointwise GEMM kernel, for the eSE gate); left empty otherwise."""
    launch = _ConvLaunch([x], [pc], [y], relu, relu_upto, res, res_upsample, in_relu, single=True)
    launch.choose()
    if pool is not None and FUSE_POOL:
        d = launch.descs[0]
        rows = _lib.load().cmk_conv_pool_rows(ctypes.byref(d))
        if rows > 0:
            pws = torch.empty((2 * (-(-(d.N * d.H * d.W) // rows)), pc.cout), dtype=torch.float32, device=y.t.device)
            d.pool_ws = pws.data_ptr()
            pool.append((pws, rows))
    launch.launch()


def conv2d_multi(xs: Sequence[View], pcs: Sequence[PackedConv], ys: Sequence[View], relu: bool = False,
                 relu_upto: Optional[int] = None, in_affine=None) -> None:
    """One launch over several inputs that share the packed weights (pcs[i].w is the same tensor; scale/shift may differ).
    in_affine[i] = (scale, shift) of shape (N, Cin): the producer's GroupNorm+ReLU applied while staging input i."""
    assert all(p.w.data_ptr() == pcs[0].w.data_ptr() for p in pcs)
    launch = _ConvLaunch(xs, pcs, ys, relu, relu_upto, in_affine=in_affine)
    launch.choose()
    launch.launch()


def _gn_records(descs, ys, groups):
    """Point the descriptors at a new workspace for the fused GroupNorm statistics that their kernel writes (records numbered over the problems
    in order), sized by the library's plan of the launch.  Returns affine(lo, hi, gamma, beta, eps) -> [(scale, shift)] of problems
    lo..hi-1, to be called after the launch (affine.records: the workspace itself); None, with the descriptors left without statistics, when that kernel writes none."""
    lib = _lib.load()
    nimg, cout, dev = ys[0].t.shape[0], ys[0].c, ys[0].t.device
    for i in range(len(ys)):
        descs[i].gn_groups = groups             # without a gn_ws: the question
    recs = _plan(descs, len(ys))[2]
    if not any(recs):
        for i in range(len(ys)):
            descs[i].gn_groups = 0
        return None
    gws = torch.empty((nimg * sum(recs), groups, 2), dtype=torch.float64, device=dev)
    for i in range(len(ys)):
        descs[i].gn_ws = gws.data_ptr()

    def affine(lo, hi, gamma, beta, eps):
        m = hi - lo
        out = [(torch.empty((nimg, cout), dtype=torch.float32, device=dev), torch.empty((nimg, cout), dtype=torch.float32, device=dev)) for _ in range(m)]
        hs, wss, rc = (ctypes.c_int * m)(*[y.t.shape[1] for y in ys[lo:hi]]), (ctypes.c_int * m)(*[y.t.shape[2] for y in ys[lo:hi]]), (ctypes.c_int * m)(*recs[lo:hi])
        ps, pb = (ctypes.c_void_p * m)(*[o[0].data_ptr() for o in out]), (ctypes.c_void_p * m)(*[o[1].data_ptr() for o in out])
        check(lib.cmk_groupnorm_affine_tiles(gws.data_ptr() + nimg * sum(recs[:lo]) * groups * 2 * 8, hs, wss, rc, m, gamma.data_ptr(), beta.data_ptr(), nimg, cout,
                                             groups, eps, ps, pb, _stream()), "cmk_groupnorm_affine_tiles")
        return out
    affine.records = gws
    return affine


def _gn_fusable(xs, cout, groups) -> bool:
    """The statistics of a GroupNorm can come from the conv's epilogue: a power-of-two group width <= 32 and one image count."""
    cpg = cout // groups if groups > 0 and cout % groups == 0 else 0
    return 0 < cpg <= 32 and (cpg & (cpg - 1)) == 0 and all(x.t.shape[0] == xs[0].t.shape[0] for x in xs)


def conv_gn_multi(xs: Sequence[View], pcs: Sequence[PackedConv], gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32,
                  eps: float = 1e-5, in_affine=None):
    """Tower conv (no activation) over several levels + the statistics of the GroupNorm that follows (fcos.py:182-186).
    Returns (raw conv outputs, [(scale, shift)] per level) — the affine is applied by the NEXT conv while staging.
    When the Winograd kernel runs the conv, its epilogue produces the statistics (no pass over the output)."""
    assert all(p.w.data_ptr() == pcs[0].w.data_ptr() for p in pcs)
    ys = _new_outputs(xs, pcs[0])
    launch = _ConvLaunch(xs, pcs, ys, in_affine=in_affine)
    fusable = _gn_fusable(xs, pcs[0].cout, groups)
    launch.choose(with_gn_stats=fusable)
    affine = _gn_records(launch.descs, ys, groups) if fusable else None
    launch.launch()
    if affine is None:
        return ys, groupnorm_affine_multi([y.t for y in ys], gamma, beta, groups, eps)
    return ys, affine(0, len(xs), gamma, beta, eps)


def conv_gn_multi_pair(xs_a: Sequence[View], pc_a: PackedConv, gn_a, xs_b: Sequence[View], pc_b: PackedConv, gn_b, groups: int = 32, eps: float = 1e-5,
                       in_affine_a=None, in_affine_b=None):
    """Two tower convs with DIFFERENT weights (the cls and the bbox tower of the FCOS head, fcos.py:227-231) over the same level shapes in
    ONE launch of up to 10 problems — half the launch ramps and tails of two launches — each followed by its own GroupNorm statistics
    (gn_x = (gamma, beta)).  Only the F(4x4) map kernels (and the opt-in direct fp16-split form) take per-problem weights: returns None when
    the measured / default variant of this problem is another kernel, splits K, or the fused statistics do not apply (the caller then runs
    the two towers separately).  Returns ((ys_a, affine_a), (ys_b, affine_b)) like two conv_gn_multi calls."""
    na, nb = len(xs_a), len(xs_b)
    n = na + nb
    if not PAIR_TOWERS or na != nb or n > 10 or pc_a.cout != pc_b.cout or pc_a.cin_pad != pc_b.cin_pad or not _gn_fusable(xs_a, pc_a.cout, groups):
        return None
    if (in_affine_a is None) != (in_affine_b is None) or any(tuple(a.t.shape) != tuple(b.t.shape) for a, b in zip(xs_a, xs_b)):
        return None
    xs, pcs = list(xs_a) + list(xs_b), [pc_a] * na + [pc_b] * nb
    ys = _new_outputs(xs, pc_a)
    launch = _ConvLaunch(xs, pcs, ys, in_affine=(list(in_affine_a) + list(in_affine_b)) if in_affine_a is not None else None)
    # the variant of ONE tower's launch (the table is keyed by the 5 level shapes, problems 0..na-1) decides; the 10-problem launch has no
    # entry of its own and is not timed by the tuner
    v = launch.choose(first=na, with_gn_stats=True)
    wino6 = v.wm == 6 and v.wn == 1 and pc_a.w_wino6 is not None and pc_b.w_wino6 is not None
    sp3 = v.wm == 11 and pc_a.w_splith is not None and pc_b.w_splith is not None      # opt-in direct fp16-split form
    if v.splitk > 1 or not (wino6 or sp3):
        return None
    launch.set(v._replace(tail=0))          # all 2 x levels problems; a launch of several problems has no tail
    affine = _gn_records(launch.descs, ys, groups)
    launch.launch("cmk_conv2d_nhwc_multi (tower pair)")
    return (ys[:na], affine(0, na, gn_a[0], gn_a[1], eps)), (ys[na:], affine(na, n, gn_b[0], gn_b[1], eps))


def conv_out_multi(xs: Sequence[View], pcs: Sequence[PackedConv], **kw) -> List[View]:  # kw: relu, relu_upto, in_affine
    ys = _new_outputs(xs, pcs[0])
    conv2d_multi(xs, pcs, ys, **kw)
    return ys


def conv_out(x: View, pc: PackedConv, **kw) -> View:
    y, = _new_outputs([x], pc)
    conv2d(x, pc, y, **kw)
    return y


def linear(x2d: torch.Tensor, pc: PackedConv, relu: bool = False) -> torch.Tensor:
    """y = x @ W^T + b as a 1x1 conv over the rows (maskiou_head.py:89-91, 116-119)."""
    r, k = x2d.shape
    y = torch.empty((1, 1, r, pc.cout), dtype=torch.float32, device=x2d.device)
    conv2d(View(x2d.reshape(1, 1, r, k)), pc, View(y), relu=relu)
    return y.reshape(r, pc.cout)


class PackedDeformConv:
    """Device-resident weights of a deformable 3x3 conv (DFConv3x3 '/conv', vovnet.py:132-201) in the direct conv packing, plus the
    folded FrozenBN scale/shift.  No Winograd forms: the deformable kernel samples its input per tap."""

    def __init__(self, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor], device):
        self.cout, self.cin, k, k2 = weight.shape
        assert k == k2 == 3, "deformable conv: 3x3 weights expected, got {}".format(tuple(weight.shape))
        if self.cin % 16:
            raise _lib.CmkError("deformable conv: Cin = {} must be a multiple of 16".format(self.cin))
        self.w = pack_conv_weight(weight).to(device)
        self.scale = (torch.ones(self.cout) if scale is None else scale.detach().float().cpu()).contiguous().to(device)
        self.shift = (torch.zeros(self.cout) if shift is None else shift.detach().float().cpu()).contiguous().to(device)


def deform_groups_supported(cin: int, dg: int) -> bool:
    """What cmk_deform_conv3x3_nhwc takes: dg in {1, 2, 4}, Cin % 16 == 0 and (Cin/dg) % 8 == 0."""
    return dg in (1, 2, 4) and cin % 16 == 0 and (cin // dg) % 8 == 0


def deform_conv3x3(x: View, offsets: torch.Tensor, packed: PackedDeformConv, y: View, dg: int, modulated: bool, relu: bool = True) -> None:
    """d2 DeformConv / ModulatedDeformConv 3x3 (stride 1, pad 1, no bias) + folded FrozenBN (+ ReLU) into the slice y.
    offsets: the offset conv's raw NHWC output (N,H,W,>= 18*dg | 27*dg) in d2's layout; with `modulated` its channels
    [18*dg, 27*dg) are mask logits, the sigmoid is applied by the kernel."""
    lib = _lib.load()
    _need_gpu(x.t, "deform_conv3x3")
    _need_gpu(offsets, "deform_conv3x3 offsets")
    n, h, w = x.nhw
    assert x.c == packed.cin and y.c == packed.cout, (x.c, y.c, packed.cin, packed.cout)
    assert y.nhw == (n, h, w) and offsets.dim() == 4 and tuple(offsets.shape[:3]) == (n, h, w) and offsets.is_contiguous()
    check(lib.cmk_deform_conv3x3_nhwc(x.t.data_ptr(), x.cs, x.co, offsets.data_ptr(), offsets.shape[3], packed.w.data_ptr(),
                                      packed.scale.data_ptr(), packed.shift.data_ptr(), y.t.data_ptr(), y.cs, y.co, n, h, w,
                                      packed.cin, packed.cout, dg, int(bool(modulated)), int(bool(relu)), _stream()),
          "cmk_deform_conv3x3_nhwc")


GROUP_CONV_CG = (4, 8, 16, 32, 64)     # channels per group that cmk_group_conv3x3_nhwc builds


def group_conv_supported(c: int, groups: int) -> bool:
    """What cmk_group_conv3x3_nhwc takes: groups >= 2 dividing C, with C / groups in {4, 8, 16, 32, 64}."""
    return groups >= 2 and c >= groups and c % groups == 0 and c // groups in GROUP_CONV_CG


def pack_group_weight(weight: torch.Tensor, groups: int) -> torch.Tensor:
    """(C, Cg, 3, 3) weight of a grouped 3x3 conv (C = groups * Cg) -> the 9*Cg*C floats cmk_group_conv3x3_nhwc reads (csrc/conv_group3.hip),
    tap = kh*3 + kw, ci the input channel inside the group:
      Cg in {4, 8}:        [tap][ci][C]:                        packed[(tap*Cg + ci)*C + cout] = weight[cout, ci, kh, kw]
      Cg in {16, 32, 64}:  [group][chunk][tap][tile][q][n][j]:  weight[group*Cg + tile*16 + n, chunk*16 + 4*q + j, kh, kw]
                           with chunk, tile < Cg/16, q < 4, n < 16, j < 4."""
    if weight.dim() != 4 or groups < 2 or weight.shape[0] % groups or tuple(weight.shape[1:]) != (weight.shape[0] // groups, 3, 3):
        raise _lib.CmkError("grouped conv: a (C, C/groups, 3, 3) weight is expected for groups = {}, got {}".format(groups, tuple(weight.shape)))
    c, cg = weight.shape[0], weight.shape[1]
    if cg not in GROUP_CONV_CG:
        raise _lib.CmkError("grouped conv: Cg = {} channels per group is not built ({} are)".format(cg, list(GROUP_CONV_CG)))
    w = weight.detach().float().cpu()
    if cg < 16:
        return w.permute(2, 3, 1, 0).reshape(-1).contiguous()
    t = cg // 16
    return w.reshape(groups, t, 16, t, 4, 4, 3, 3).permute(0, 3, 6, 7, 1, 4, 2, 5).reshape(-1).contiguous()


class PackedGroupConv:
    """Device-resident packed weight of a grouped 3x3 conv (ResNeXt conv2) plus the folded FrozenBN scale/shift."""

    def __init__(self, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor], device, groups: int, stride: int = 1):
        self.w = pack_group_weight(weight, groups).to(device)
        self.c, self.cg, self.groups, self.stride = weight.shape[0], weight.shape[1], groups, stride
        self.cin = self.cout = self.c
        if stride not in (1, 2):
            raise _lib.CmkError("grouped conv: stride {} must be 1 or 2".format(stride))
        self.scale = (torch.ones(self.c) if scale is None else scale.detach().float().cpu()).contiguous().to(device)
        self.shift = (torch.zeros(self.c) if shift is None else shift.detach().float().cpu()).contiguous().to(device)


def group_conv3x3(x: View, packed: PackedGroupConv, y: Optional[View] = None, relu: bool = False) -> View:
    """Grouped 3x3 conv (pad 1, packed.stride, no bias) + folded FrozenBN (+ ReLU): y = [relu](gconv3x3(x) * scale + shift)."""
    lib = _lib.load()
    _need_gpu(x.t, "group_conv3x3")
    n, h, w = x.nhw
    s = packed.stride
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    if y is None:
        y = View(torch.empty((n, ho, wo, packed.c), dtype=torch.float32, device=x.t.device))
    assert x.c == packed.c and y.c == packed.c and y.nhw == (n, ho, wo), (x.c, y.c, packed.c, y.nhw)
    check(lib.cmk_group_conv3x3_nhwc(x.t.data_ptr(), x.cs, x.co, packed.w.data_ptr(), packed.scale.data_ptr(), packed.shift.data_ptr(),
                                     y.t.data_ptr(), y.cs, y.co, n, h, w, packed.c, packed.groups, s, int(bool(relu)), _stream()),
          "cmk_group_conv3x3_nhwc")
    return y


# ---------------------------------------------------------------------------------------------------------------
# backbone pieces
# ---------------------------------------------------------------------------------------------------------------
def stem_conv(x_nchw: torch.Tensor, w27: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> View:
    lib = _lib.load()
    _need_gpu(x_nchw, "stem_conv")
    x_nchw = x_nchw.contiguous()
    n, c, h, w = x_nchw.shape
    assert c == 3
    cout = w27.shape[1]
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cout), dtype=torch.float32, device=x_nchw.device)
    check(lib.cmk_stem_conv_nchw3(x_nchw.data_ptr(), w27.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(),
                                  n, h, w, cout, _stream()), "cmk_stem_conv_nchw3")
    return View(y)


def pack_stem7_weight(weight: torch.Tensor) -> torch.Tensor:
    """(Cout,3,7,7) weight of d2's BasicStem conv -> [147][Cout] with k = (kh*7 + kw)*3 + ci (what cmk_stem7x7_bn_relu_maxpool_nchw3 reads)."""
    cout = weight.shape[0]
    assert tuple(weight.shape) == (cout, 3, 7, 7), "the ResNet stem weight must be (Cout,3,7,7)"
    return weight.detach().float().cpu().permute(2, 3, 1, 0).reshape(147, cout).contiguous()


def stem7x7_bn_relu_maxpool(x_nchw: torch.Tensor, w147: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, y: Optional[View] = None) -> View:
    """d2 BasicStem in one launch: max_pool2d(relu(conv7x7 s2 p3 (x) * scale + shift), 3, 2, 1) on the NCHW 3-channel image -> NHWC view
    (csrc/stem7_pool.hip; the conv map is never written to memory)."""
    lib = _lib.load()
    _need_gpu(x_nchw, "stem7x7_bn_relu_maxpool")
    x_nchw = x_nchw.contiguous()
    n, c, h, w = x_nchw.shape
    assert c == 3 and x_nchw.dtype == torch.float32
    cout = w147.shape[1]
    assert tuple(w147.shape) == (147, cout) and tuple(scale.shape) == tuple(shift.shape) == (cout,)
    hp, wp = ((h - 1) // 2) // 2 + 1, ((w - 1) // 2) // 2 + 1
    if y is None:
        y = View(torch.empty((n, hp, wp, cout), dtype=torch.float32, device=x_nchw.device))
    assert y.nhw == (n, hp, wp) and y.c == cout
    check(lib.cmk_stem7x7_bn_relu_maxpool_nchw3(x_nchw.data_ptr(), w147.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.t.data_ptr(), y.cs, y.co,
                                                n, h, w, cout, _stream()), "cmk_stem7x7_bn_relu_maxpool_nchw3")
    return y


def pack_dw_weight(weight: torch.Tensor) -> torch.Tensor:
    """(C,1,3,3) depth-wise weight -> tap-major [9][C] (the layout cmk_dwconv3x3_nhwc reads)."""
    c = weight.shape[0]
    assert tuple(weight.shape) == (c, 1, 3, 3), "depth-wise 3x3 weight must be (C,1,3,3)"
    return weight.detach().float().cpu().reshape(c, 9).t().contiguous()


def dwconv3x3(x: View, w9c: torch.Tensor, y: Optional[View] = None, stride: int = 1) -> View:
    """Depth-wise 3x3, pad 1, no bias / activation (vovnet.py:110-119)."""
    lib = _lib.load()
    _need_gpu(x.t, "dwconv3x3")
    n, h, w = x.nhw
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if y is None:
        y = View(torch.empty((n, ho, wo, x.c), dtype=torch.float32, device=x.t.device))
    assert y.nhw == (n, ho, wo) and y.c == x.c and tuple(w9c.shape) == (9, x.c)
    check(lib.cmk_dwconv3x3_nhwc(x.t.data_ptr(), x.cs, x.co, w9c.data_ptr(), y.t.data_ptr(), y.cs, y.co, n, h, w, x.c, stride, _stream()),
          "cmk_dwconv3x3_nhwc")
    return y


def dwconv3x3_bn_act(x: View, w9c: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, y: Optional[View] = None, stride: int = 1,
                     in_max: float = float("inf"), out_min: float = float("-inf"), out_max: float = float("inf")) -> View:
    """Depth-wise 3x3 (pad 1) of an inverted-residual block with its surroundings fused (mobilenet.py:38-76):
    y = clamp(dw3x3(min(x, in_max)) * scale + shift, out_min, out_max).  in_max = 6 finishes the producer's ReLU6 (its conv ran with the
    plain ReLU epilogue), scale/shift is the folded FrozenBN, [0, 6] the block's own ReLU6; the infinite defaults switch a clamp off."""
    lib = _lib.load()
    _need_gpu(x.t, "dwconv3x3_bn_act")
    n, h, w = x.nhw
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if y is None:
        y = View(torch.empty((n, ho, wo, x.c), dtype=torch.float32, device=x.t.device))
    assert y.nhw == (n, ho, wo) and y.c == x.c and tuple(w9c.shape) == (9, x.c) and tuple(scale.shape) == tuple(shift.shape) == (x.c,)
    check(lib.cmk_dwconv3x3_bn_act_nhwc(x.t.data_ptr(), x.cs, x.co, w9c.data_ptr(), scale.data_ptr(), shift.data_ptr(), in_max, out_min, out_max,
                                        y.t.data_ptr(), y.cs, y.co, n, h, w, x.c, stride, _stream()), "cmk_dwconv3x3_bn_act_nhwc")
    return y


def maxpool3x3s2_ceil(x: View, y: Optional[View] = None, gate: Optional[torch.Tensor] = None) -> View:
    lib = _lib.load()
    _need_gpu(x.t, "maxpool3x3s2_ceil")
    n, h, w = x.nhw
    ho = -(-(h - 3) // 2) + 1
    wo = -(-(w - 3) // 2) + 1
    if (ho - 1) * 2 >= h:
        ho -= 1
    if (wo - 1) * 2 >= w:
        wo -= 1
    if y is None:
        y = View(torch.empty((n, ho, wo, x.c), dtype=torch.float32, device=x.t.device))
    _need_same_geometry(y, n, ho, wo, x.c, x.t, "maxpool3x3s2_ceil output")
    if gate is not None:
        _need_gate(gate, n, x.c, x.t, "maxpool3x3s2_ceil")
    check(lib.cmk_maxpool3x3s2_ceil_nhwc(x.t.data_ptr(), x.cs, x.co, y.t.data_ptr(), y.cs, y.co, n, h, w, x.c,
                                         gate.data_ptr() if gate is not None else None, _stream()),
          "cmk_maxpool3x3s2_ceil_nhwc")
    return y


def maxpool1x1s2(x: View) -> View:
    """MaxPool2d(kernel_size=1, stride=2): every second pixel (d2 LastLevelMaxPool; vovnet.py:504-524)."""
    lib = _lib.load()
    _need_gpu(x.t, "maxpool1x1s2")
    n, h, w = x.nhw
    y = View(torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, x.c), dtype=torch.float32, device=x.t.device))
    check(lib.cmk_maxpool1x1s2_nhwc(x.t.data_ptr(), x.cs, x.co, y.t.data_ptr(), y.cs, y.co, n, h, w, x.c, _stream()), "cmk_maxpool1x1s2_nhwc")
    return y


def _ese_chunks(hw: int, c: int) -> int:
    """Pixel chunks per image for the eSE average pool: ~32K elements per workgroup so even the 25x40 stage fills the chip."""
    return max(1, min(256, (hw * c) // 32768))


def ese_gate(x: View, fc_w: torch.Tensor, fc_b: torch.Tensor) -> torch.Tensor:
    """gate (N,C) = hsigmoid(fc(mean_HW(x)))   (vovnet.py:255-259)."""
    lib = _lib.load()
    _need_gpu(x.t, "ese_gate")
    n, h, w = x.nhw
    hw, c = h * w, x.c
    chunks = _ese_chunks(hw, c)
    ws = torch.empty((n, chunks, c), dtype=torch.float32, device=x.t.device)
    gate = torch.empty((n, c), dtype=torch.float32, device=x.t.device)
    check(lib.cmk_ese_gate(x.t.data_ptr(), x.cs, x.co, fc_w.data_ptr(), fc_b.data_ptr(), gate.data_ptr(), ws.data_ptr(), chunks,
                           n, hw, c, _stream()), "cmk_ese_gate")
    return gate


def ese_gate_pooled(pooled, fc_w: torch.Tensor, fc_b: torch.Tensor, n: int, hw: int) -> torch.Tensor:
    """The same gate from the partial sums the producing conv left behind (conv2d(..., pool=[...])): no pass over the map."""
    lib = _lib.load()
    pws, rows = pooled
    c = pws.shape[1]
    gate = torch.empty((n, c), dtype=torch.float32, device=pws.device)
    check(lib.cmk_ese_gate_pooled(pws.data_ptr(), rows, fc_w.data_ptr(), fc_b.data_ptr(), gate.data_ptr(), n, hw, c, _stream()), "cmk_ese_gate_pooled")
    return gate


def ese(x: View, fc_w: torch.Tensor, fc_b: torch.Tensor, y: View, identity: Optional[View] = None, gate: Optional[torch.Tensor] = None) -> None:
    """y = x * hsigmoid(fc(mean_HW(x))) (+ identity)   (vovnet.py:255-260, :329-330).  gate: already computed (ese_gate_pooled)."""
    lib = _lib.load()
    _need_gpu(x.t, "ese")
    n, h, w = x.nhw
    hw, c = h * w, x.c
    _need_same_geometry(y, n, h, w, c, x.t, "ese output")
    if identity is not None:
        _need_same_geometry(identity, n, h, w, c, x.t, "ese identity")
    if gate is None:
        gate = ese_gate(x, fc_w, fc_b)
    _need_gate(gate, n, c, x.t, "ese")
    idp, idcs, idco = (identity.t.data_ptr(), identity.cs, identity.co) if identity is not None else (None, 0, 0)
    check(lib.cmk_ese_scale(x.t.data_ptr(), x.cs, x.co, gate.data_ptr(), idp, idcs, idco, y.t.data_ptr(), y.cs, y.co,
                            n, hw, c, _stream()), "cmk_ese_scale")


def _gn_chunks(hw: int) -> int:
    """Pixel chunks per image for the GroupNorm statistics of one map: 128 pixels per workgroup, at most 128 chunks."""
    return max(1, min(128, hw // 128))


def groupnorm_affine(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32, eps: float = 1e-5):
    """GroupNorm statistics of a dense NHWC tensor as per-(image, channel) (scale, shift); the consumer conv applies
    relu(x*scale + shift) while staging (cmk_conv_desc.in_scale/in_shift), so the normalised tensor is never written."""
    lib = _lib.load()
    _need_dense_nhwc(x, "groupnorm_affine")
    n, h, w, c = x.shape
    hw = h * w
    chunks = _gn_chunks(hw)
    ws = torch.empty((n, groups, chunks, 2), dtype=torch.float64, device=x.device)
    sc = torch.empty((n, c), dtype=torch.float32, device=x.device)
    sh = torch.empty((n, c), dtype=torch.float32, device=x.device)
    check(lib.cmk_groupnorm_affine(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), chunks, n, hw, c, groups, eps,
                                   sc.data_ptr(), sh.data_ptr(), _stream()), "cmk_groupnorm_affine")
    return sc, sh


def groupnorm_affine_multi(xs: Sequence[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32, eps: float = 1e-5):
    """groupnorm_affine for several dense NHWC tensors with the same (N, C) — the FPN levels — in two launches."""
    lib = _lib.load()
    nl = len(xs)
    n, c = xs[0].shape[0], xs[0].shape[3]
    dev = xs[0].device
    chunks = 64
    ws = torch.empty((nl, n, groups, chunks, 2), dtype=torch.float64, device=dev)
    out = [(torch.empty((n, c), dtype=torch.float32, device=dev), torch.empty((n, c), dtype=torch.float32, device=dev)) for _ in xs]
    px, ps, pb = (ctypes.c_void_p * nl)(), (ctypes.c_void_p * nl)(), (ctypes.c_void_p * nl)()
    hws = (ctypes.c_int * nl)()
    for i, x in enumerate(xs):
        _need_gpu(x, "groupnorm_affine_multi")
        assert x.is_contiguous() and x.shape[0] == n and x.shape[3] == c
        px[i], ps[i], pb[i] = x.data_ptr(), out[i][0].data_ptr(), out[i][1].data_ptr()
        hws[i] = x.shape[1] * x.shape[2]
    check(lib.cmk_groupnorm_affine_multi(px, hws, nl, gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), chunks, n, c, groups, eps, ps, pb,
                                         _stream()), "cmk_groupnorm_affine_multi")
    return out


def groupnorm_relu_(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32, eps: float = 1e-5, relu: bool = True) -> None:
    """GroupNorm (+ ReLU) in place on a dense NHWC tensor (fcos.py:182-186; relu=False: d2's get_norm("GN") behind a conv without activation)."""
    lib = _lib.load()
    _need_dense_nhwc(x, "groupnorm_relu_")
    n, h, w, c = x.shape
    hw = h * w
    chunks = _gn_chunks(hw)
    ws = torch.empty((n, groups, chunks, 2), dtype=torch.float64, device=x.device)
    fn = lib.cmk_groupnorm_relu_nhwc if relu else lib.cmk_groupnorm_nhwc
    check(fn(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), chunks, n, hw, c, groups, eps, _stream()), "cmk_groupnorm[_relu]_nhwc")


def upsample2x_add_(y: View, coarse: View) -> None:
    """y += nearest-2x-upsampling(coarse), dense NHWC tensors (d2 FPN top-down sum behind a norm)."""
    lib = _lib.load()
    _need_gpu(y.t, "upsample2x_add_")
    assert y.co == 0 and coarse.co == 0 and y.cs == y.c and coarse.cs == coarse.c and y.c == coarse.c, "upsample2x_add_ needs dense NHWC tensors"
    n, h, w = y.nhw
    check(lib.cmk_upsample2x_add_nhwc(y.t.data_ptr(), coarse.t.data_ptr(), n, h, w, coarse.t.shape[1], coarse.t.shape[2], y.c, _stream()), "cmk_upsample2x_add_nhwc")


# ---------------------------------------------------------------------------------------------------------------
# FCOS post-head: candidate selection, sort + NMS + top-k (all counts stay on the device)
# ---------------------------------------------------------------------------------------------------------------
def fcos_select(logits: Sequence[torch.Tensor], regctr: Sequence[torch.Tensor], strides: Sequence[int], thresh: float, cap: int,
                thresh_with_ctr: bool = False):
    """logits[l]: (N,H,W,C) dense NHWC; regctr[l]: (N,H,W,5).  Returns dict of candidate buffers (N,cap,...) + counts (N)."""
    lib = _lib.load()
    n, c = logits[0].shape[0], logits[0].shape[3]
    dev = logits[0].device
    _need_gpu(logits[0], "fcos_select")
    nl = len(logits)
    lv = (FcosLevel * nl)()
    for i, (lg, rc, s) in enumerate(zip(logits, regctr, strides)):
        assert lg.is_contiguous() and rc.is_contiguous() and rc.shape[3] == 5 and lg.shape[:3] == rc.shape[:3]
        lv[i].logits, lv[i].regctr = lg.data_ptr(), rc.data_ptr()
        lv[i].H, lv[i].W, lv[i].stride = lg.shape[1], lg.shape[2], int(s)
    wslen = lib.cmk_fcos_select_ws_len(lv, nl, n, c)
    assert wslen > 0
    ws = torch.empty((wslen,), dtype=torch.int32, device=dev)
    out = dict(box=torch.empty((n, cap, 4), dtype=torch.float32, device=dev),
               score=torch.empty((n, cap), dtype=torch.float32, device=dev),
               cls=torch.empty((n, cap), dtype=torch.int32, device=dev),
               loc=torch.empty((n, cap, 2), dtype=torch.float32, device=dev),
               counts=torch.empty((n,), dtype=torch.int32, device=dev), cap=cap)
    check(lib.cmk_fcos_select(lv, nl, n, c, float(thresh), int(bool(thresh_with_ctr)), out["box"].data_ptr(), out["score"].data_ptr(), out["cls"].data_ptr(),
                              out["loc"].data_ptr(), out["counts"].data_ptr(), ws.data_ptr(), wslen, cap, _stream()), "cmk_fcos_select")
    return out


NMS_METRICS = {"iou": 0, "ios": 1}       # include/cmk.h, cmk_nms_topk_metric


def nms_topk(cand: dict, iou_thr: float, topk: int, metric: str = "iou"):
    """metric "iou": the detector's NMS.  "ios": suppress on intersection over the smaller box > iou_thr (the merge of sliced inference)."""
    if metric not in NMS_METRICS:
        raise _lib.CmkError("nms_topk: metric must be one of {}, got {!r}".format(sorted(NMS_METRICS), metric))
    lib = _lib.load()
    n, cap = cand["score"].shape
    dev = cand["score"].device
    _need_gpu(cand["score"], "nms_topk")
    out = dict(box=torch.empty((n, topk, 4), dtype=torch.float32, device=dev),
               score=torch.empty((n, topk), dtype=torch.float32, device=dev),
               cls=torch.empty((n, topk), dtype=torch.int64, device=dev),
               loc=torch.empty((n, topk, 2), dtype=torch.float32, device=dev),
               idx=torch.empty((n, topk), dtype=torch.int32, device=dev),
               counts=torch.empty((n,), dtype=torch.int32, device=dev))
    ws = torch.empty((n, 4, cap), dtype=torch.int32, device=dev)
    check(lib.cmk_nms_topk_metric(cand["box"].data_ptr(), cand["score"].data_ptr(), cand["cls"].data_ptr(), cand["loc"].data_ptr(),
                                  cand["counts"].data_ptr(), n, cap, float(iou_thr), NMS_METRICS[metric], topk, out["box"].data_ptr(),
                                  out["score"].data_ptr(), out["cls"].data_ptr(), out["loc"].data_ptr(), out["idx"].data_ptr(),
                                  out["counts"].data_ptr(), ws.data_ptr(), _stream()), "cmk_nms_topk_metric")
    return out


# ---------------------------------------------------------------------------------------------------------------
# ROI heads
# ---------------------------------------------------------------------------------------------------------------
def roi_align_ratio(feats: Sequence[View], scales: Sequence[float], boxes: torch.Tensor, counts: torch.Tensor,
                    img_area: torch.Tensor, out_size: int, sampling_ratio: int, y: torch.Tensor, min_level: int,
                    aligned: bool = True, assign_by_area: bool = False, canonical_box_size: float = 224.0, canonical_level: int = 4):
    """feats: dense NHWC levels; boxes (N,topk,4); y: (N*topk,out,out,y_cs) receives channels [0,C).  Returns levels (N*topk) int32.
    aligned False = ROIAlign v1; assign_by_area = FPN Eqn.(1) instead of CenterMask's ratio rule (pooler.py:121-152)."""
    lib = _lib.load()
    _need_gpu(feats[0].t, "roi_align")
    nl = len(feats)
    n, topk = boxes.shape[0], boxes.shape[1]
    c = feats[0].c
    ptrs = (ctypes.c_void_p * nl)()
    hs, ws_ = (ctypes.c_int * nl)(), (ctypes.c_int * nl)()
    sc = (ctypes.c_float * nl)()
    for i, f in enumerate(feats):
        assert f.co == 0 and f.cs == c, "roi_align needs dense NHWC features"
        ptrs[i] = f.t.data_ptr()
        hs[i], ws_[i] = f.t.shape[1], f.t.shape[2]
        sc[i] = float(scales[i])
    levels = torch.empty((n * topk,), dtype=torch.int32, device=boxes.device)
    check(lib.cmk_roi_align_pool(ptrs, hs, ws_, sc, nl, min_level, c, boxes.data_ptr(), counts.data_ptr(), img_area.data_ptr(),
                                 n, topk, out_size, sampling_ratio, int(bool(aligned)), int(bool(assign_by_area)), float(canonical_box_size),
                                 int(canonical_level), y.data_ptr(), y.shape[3], levels.data_ptr(), _stream()),
          "cmk_roi_align_pool")
    return levels


def spatial_attention_(x: torch.Tensor, w: torch.Tensor, counts: torch.Tensor, topk: int) -> None:
    lib = _lib.load()
    _need_gpu(x, "spatial_attention")
    r, s, _, c = x.shape
    check(lib.cmk_spatial_attention(x.data_ptr(), w.data_ptr(), counts.data_ptr(), topk, r, s, c, _stream()), "cmk_spatial_attention")


def mask_predict(dec: torch.Tensor, pw: torch.Tensor, pb: torch.Tensor, cls: torch.Tensor, counts: torch.Tensor, topk: int,
                 want_logits: bool = False):
    """dec: (R,S,S,4*C) relu(deconv); returns masks (R,1,2S,2S) [, selected-class logits (R,2S,2S)]."""
    lib = _lib.load()
    _need_gpu(dec, "mask_predict")
    r, s = dec.shape[0], dec.shape[1]
    c = dec.shape[3] // 4
    masks = torch.empty((r, 1, 2 * s, 2 * s), dtype=torch.float32, device=dec.device)
    logits = torch.empty((r, 2 * s, 2 * s), dtype=torch.float32, device=dec.device) if want_logits else None
    check(lib.cmk_mask_predict(dec.data_ptr(), pw.data_ptr(), pb.data_ptr(), cls.data_ptr(), counts.data_ptr(), topk, r, s, c,
                               masks.data_ptr(), logits.data_ptr() if want_logits else None, _stream()), "cmk_mask_predict")
    return (masks, logits) if want_logits else masks


def mask_pool_concat_(masks: torch.Tensor, y: torch.Tensor, y_co: int) -> None:
    lib = _lib.load()
    r, s = y.shape[0], y.shape[1]
    check(lib.cmk_mask_pool_concat(masks.data_ptr(), y.data_ptr(), y.shape[3], y_co, r, s, _stream()), "cmk_mask_pool_concat")


def mask_iou_score(iou: torch.Tensor, scores: torch.Tensor, cls: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    r = iou.shape[0]
    out = torch.empty((r,), dtype=torch.float32, device=iou.device)
    check(lib.cmk_mask_iou_score(iou.data_ptr(), iou.shape[1], scores.data_ptr(), cls.data_ptr(), out.data_ptr(), r, _stream()),
          "cmk_mask_iou_score")
    return out


def keypoint_decode(dec: View, boxes: torch.Tensor, counts: torch.Tensor, num_keypoints: int) -> torch.Tensor:
    """Keypoint heatmap decode (keypoint_head.py:89-116, 219-224 -> d2 heatmaps_to_keypoints; cmk_keypoint_decode).  dec: the packed
    score_lowres output, a view (N*topk, S, S, >= 4K) with channel (2py+px)*K + k; boxes (N, topk, 4); counts (N,) int32 on the device.
    Returns (N, topk, K, 3) = (x, y, score); slots past counts[n] are zeros."""
    lib = _lib.load()
    _need_gpu(dec.t, "keypoint_decode")
    _need_gpu(boxes, "keypoint_decode boxes")
    n, topk = boxes.shape[0], boxes.shape[1]
    r, s = dec.t.shape[0], dec.t.shape[1]
    assert boxes.dim() == 3 and boxes.shape[2] == 4 and boxes.is_contiguous(), tuple(boxes.shape)
    assert counts.dtype == torch.int32 and counts.is_cuda and counts.numel() == n
    assert r == n * topk and dec.t.shape[2] == s and dec.c == 4 * num_keypoints, (tuple(dec.t.shape), dec.c, n, topk, num_keypoints)
    ws_len = lib.cmk_keypoint_decode_ws_len(r, num_keypoints)
    ws = torch.empty((max(ws_len, 1),), dtype=torch.float32, device=boxes.device)
    out = torch.empty((n, topk, num_keypoints, 3), dtype=torch.float32, device=boxes.device)
    check(lib.cmk_keypoint_decode(dec.t.data_ptr(), dec.cs, dec.co, s, num_keypoints, boxes.data_ptr(), counts.data_ptr(), n, topk,
                                  ws.data_ptr(), ws_len, out.data_ptr(), _stream()), "cmk_keypoint_decode")
    return out


# ---------------------------------------------------------------------------------------------------------------
# optional per-launch timing (bench.py's roofline leg): events on the launch stream around every conv
# ---------------------------------------------------------------------------------------------------------------
PROFILE = None       # when a list, conv2d appends (kernel_key, flops, algorithmic_bytes, start_event, end_event, shape, executed_flops)


def kernel_source_hash() -> str:
    """Hash of the conv kernel sources the loaded library was built from (the tree travels with the .so): PMC summaries under
    profiles/ carry it, so a summary of an older kernel is detected instead of quoted."""
    import hashlib
    import os
    h = hashlib.sha1()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    for f in ("conv_args.hpp", "conv_split.hpp", "wino6_common.hpp", "conv.hip", "conv_igemm.hip", "conv_wino4r.hip", "conv_wino6.hip", "conv_wino6s.hip", "conv_pw.hip", "conv_sp3.hip"):
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:12]


# ---------------------------------------------------------------------------------------------------------------
# before / after the model
# ---------------------------------------------------------------------------------------------------------------
def preprocess_images(images: Sequence[torch.Tensor], mean, std, size_divisibility: int = 32, fixed_size: Optional[int] = None):
    """CHW uint8/float32 images on the GPU -> (N,3,H,W) float32 normalised, zero-padded right/bottom; returns (batch, sizes).
    fixed_size=1344 reproduces deploy_utils.single_preprocessing; otherwise the batch max rounded up to the divisibility."""
    lib = _lib.load()
    sizes = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
    if fixed_size:
        H = W = int(fixed_size)
    else:
        d = max(1, size_divisibility)
        H = (max(s[0] for s in sizes) + d - 1) // d * d
        W = (max(s[1] for s in sizes) + d - 1) // d * d
    dev = images[0].device
    out = torch.empty((len(images), 3, H, W), dtype=torch.float32, device=dev)
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    for i, im in enumerate(images):
        if not im.is_cuda or im.dtype not in (torch.uint8, torch.float32) or im.dim() != 3 or im.shape[0] != 3:
            raise _lib.CmkError("preprocess_images: need (3,h,w) uint8/float32 CUDA tensors")
        im = im.contiguous()
        check(lib.cmk_preprocess_chw(im.data_ptr(), int(im.dtype == torch.uint8), out[i].data_ptr(), sizes[i][0], sizes[i][1], H, W,
                                     m3, s3, _stream()), "cmk_preprocess_chw")
    return out, sizes


def resize_shortest_edge_shape(h: int, w: int, short: int, max_size: int) -> Tuple[int, int]:
    """detectron2 ResizeShortestEdge.get_output_shape in Python floats -> (new_h, new_w).  Not postprocess.resize_scale: that one mirrors
    the floor-based rule of deploy_utils.py:138-142."""
    size = short * 1.0
    scale = size / min(h, w)
    if h < w:
        newh, neww = size, scale * w
    else:
        newh, neww = scale * h, size
    if max(newh, neww) > max_size:
        s = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * s, neww * s
    return int(newh + 0.5), int(neww + 0.5)


RESIZE_BITS = 22          # Pillow's PRECISION_BITS for 8-bit bands (Resample.c: 32 - 8 - 2)


def resize_coeffs(in_size: int, out_size: int):
    """Pillow's bilinear tables for one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc), in float64 on the host — each
    step a single IEEE operation in the order of the C source, nothing fused: (bounds (out, 2) int32 = first tap and tap count,
    kk (out, ksize) int32 = weights scaled by 2^22, ksize)."""
    import math
    import numpy as np
    if in_size < 1 or out_size < 1:
        raise _lib.CmkError("resize_coeffs: sizes must be positive, got {} -> {}".format(in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                 # (int) in C: truncation towards zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss))
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):                                                          # the C loop's order of additions
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = (0.5 + w * float(1 << RESIZE_BITS)).astype(np.int64).astype(np.int32)      # bilinear weights are never negative
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    return bounds, kk, ksize


_RESIZE_TABLES = {}       # (device index, in, out) -> (bounds, kk, ksize) on that device: a size pair is uploaded once


def _resize_tables(in_size: int, out_size: int, dev: torch.device):
    key = (dev.index, in_size, out_size)
    t = _RESIZE_TABLES.get(key)
    if t is None:
        bounds, kk, ksize = resize_coeffs(in_size, out_size)
        assert ksize == _lib.load().cmk_resize_ksize(in_size, out_size)
        t = _RESIZE_TABLES[key] = (torch.from_numpy(bounds).to(dev), torch.from_numpy(kk).to(dev), ksize)
    return t


def _need_u8_hwc(im, what: str) -> None:
    if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
        raise _lib.CmkError("{}: need (h,w,3) uint8 tensors, got {}".format(
            what, "{} {}".format(im.dtype, tuple(im.shape)) if torch.is_tensor(im) else type(im).__name__))
    if not im.is_cuda:
        raise _lib.CmkError("{}: tensor is on {}; the resize runs on the GPU (no CPU fallback)".format(what, im.device))
    _need_current_device(im, what)


def _resize_h(lib, im: torch.Tensor, new_w: int, ws: torch.Tensor) -> torch.Tensor:
    """Horizontal pass of one (h,w,3) image into the workspace ws (>= h*new_w*3 bytes); the image itself where the pass is skipped."""
    h, w = int(im.shape[0]), int(im.shape[1])
    if new_w == w:
        return im
    bx, kx, ksx = _resize_tables(w, new_w, im.device)
    check(lib.cmk_resize_h_u8(im.data_ptr(), h, w, new_w, bx.data_ptr(), kx.data_ptr(), ksx, ws.data_ptr(), _stream()), "cmk_resize_h_u8")
    return ws


def _resize_v_args(h: int, new_h: int, dev: torch.device):
    if new_h == h:
        return None, None, 0, None
    by, ky, ksy = _resize_tables(h, new_h, dev)
    return by.data_ptr(), ky.data_ptr(), ksy, (by, ky)


def resize_bilinear_u8(img: torch.Tensor, new_h: int, new_w: int) -> torch.Tensor:
    """(h,w,3) uint8 on the GPU -> (new_h,new_w,3) uint8, byte for byte PIL.Image.resize((new_w, new_h), BILINEAR) (what detectron2's
    ResizeTransform.apply_image runs on uint8 images)."""
    _need_u8_hwc(img, "resize_bilinear_u8")
    new_h, new_w = int(new_h), int(new_w)
    if new_h < 1 or new_w < 1:
        raise _lib.CmkError("resize_bilinear_u8: target size must be positive, got {}x{}".format(new_h, new_w))
    lib = _lib.load()
    img = img.contiguous()
    h = int(img.shape[0])
    ws = torch.empty((h * new_w * 3 + 3,), dtype=torch.uint8, device=img.device) if new_w != img.shape[1] else None
    mid = _resize_h(lib, img, new_w, ws)
    out = torch.empty((new_h, new_w, 3), dtype=torch.uint8, device=img.device)
    by, ky, ksy, keep = _resize_v_args(h, new_h, img.device)
    check(lib.cmk_resize_v_u8(mid.data_ptr(), h, new_h, new_w, by, ky, ksy, out.data_ptr(), _stream()), "cmk_resize_v_u8")
    del keep
    return out


def resize_preprocess_images(images: Sequence[torch.Tensor], short: int, max_size: int, mean, std, size_divisibility: int = 32,
                             fixed_size: Optional[int] = None, reverse_channels: bool = False):
    """Raw (h,w,3) uint8 images on the GPU -> (N,3,H,W) float32: ResizeShortestEdge(short, max_size) as detectron2 runs it on uint8
    images, then (x - mean) / std and zero padding right/bottom — the resize, preprocess_images' normalisation and its padding in two
    launches per image (one where a pass is skipped).  Returns (batch, sizes) with the RESIZED (new_h, new_w) per image; H, W as in
    preprocess_images.  reverse_channels: channel 2 of the image becomes plane 0 (BGR in, RGB model)."""
    if len(images) == 0:
        raise _lib.CmkError("resize_preprocess_images: no images")
    for im in images:
        _need_u8_hwc(im, "resize_preprocess_images")
    lib = _lib.load()
    dev = images[0].device
    sizes = [resize_shortest_edge_shape(int(im.shape[0]), int(im.shape[1]), short, max_size) for im in images]
    if fixed_size:
        H = W = int(fixed_size)
    else:
        d = max(1, size_divisibility)
        H = (max(s[0] for s in sizes) + d - 1) // d * d
        W = (max(s[1] for s in sizes) + d - 1) // d * d
    out = torch.empty((len(images), 3, H, W), dtype=torch.float32, device=dev)
    need = max([int(im.shape[0]) * s[1] * 3 for im, s in zip(images, sizes) if s[1] != im.shape[1]] or [0])
    ws = torch.empty((need + 3,), dtype=torch.uint8, device=dev) if need else None      # one workspace: the launches are ordered on the stream
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    for i, im in enumerate(images):
        im = im.contiguous()
        h = int(im.shape[0])
        new_h, new_w = sizes[i]
        mid = _resize_h(lib, im, new_w, ws)
        by, ky, ksy, keep = _resize_v_args(h, new_h, dev)
        check(lib.cmk_resize_v_preprocess(mid.data_ptr(), h, new_h, new_w, by, ky, ksy, out[i].data_ptr(), H, W, m3, s3,
                                          int(bool(reverse_channels)), _stream()), "cmk_resize_v_preprocess")
        del keep
    return out, sizes


# ---------------------------------------------------------------------------------------------------------------
# test-time augmentation (modeling/test_time_augmentation.py): the mirrored front end, the box maps and the mask average
# ---------------------------------------------------------------------------------------------------------------
def resize_preprocess_augmented(image: torch.Tensor, shapes: Sequence[Tuple[int, int]], flips, mean, std, size_divisibility: int = 32,
                                reverse_channels: bool = False) -> List[torch.Tensor]:
    """One raw (h,w,3) uint8 image on the GPU -> one canvas per entry of `shapes` ((new_h, new_w), e.g. from resize_shortest_edge_shape):
    (1 + flip, 3, H, W) float32 with the image resized to that shape in slot 0 — the bits resize_preprocess_images gives — and, where
    flips (a bool, or one per shape) says so, the mirror of the RESIZED bytes in slot 1 (detectron2 applies [resize, flip]); zero
    padding right/bottom in both.  The horizontal pass runs once per shape, the vertical pass once per slot."""
    _need_u8_hwc(image, "resize_preprocess_augmented")
    shapes = [(int(nh), int(nw)) for nh, nw in shapes]
    if len(shapes) == 0 or any(nh < 1 or nw < 1 for nh, nw in shapes):
        raise _lib.CmkError("resize_preprocess_augmented: need at least one positive (new_h, new_w), got {}".format(shapes))
    flips = [bool(flips)] * len(shapes) if isinstance(flips, (bool, int)) else [bool(f) for f in flips]
    if len(flips) != len(shapes):
        raise _lib.CmkError("resize_preprocess_augmented: {} flip flags for {} shapes".format(len(flips), len(shapes)))
    lib = _lib.load()
    dev = image.device
    image = image.contiguous()
    h, w = int(image.shape[0]), int(image.shape[1])
    d = max(1, size_divisibility)
    need = max([h * nw * 3 for _, nw in shapes if nw != w] or [0])
    ws = torch.empty((need + 3,), dtype=torch.uint8, device=dev) if need else None
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    out = []
    for (new_h, new_w), flip in zip(shapes, flips):
        H, W = (new_h + d - 1) // d * d, (new_w + d - 1) // d * d
        canvas = torch.empty((2 if flip else 1, 3, H, W), dtype=torch.float32, device=dev)
        mid = _resize_h(lib, image, new_w, ws)
        by, ky, ksy, keep = _resize_v_args(h, new_h, dev)
        check(lib.cmk_resize_v_preprocess(mid.data_ptr(), h, new_h, new_w, by, ky, ksy, canvas[0].data_ptr(), H, W, m3, s3,
                                          int(bool(reverse_channels)), _stream()), "cmk_resize_v_preprocess")
        if flip:
            check(lib.cmk_resize_v_preprocess_hflip(mid.data_ptr(), h, new_h, new_w, by, ky, ksy, canvas[1].data_ptr(), H, W, m3, s3,
                                                    int(bool(reverse_channels)), _stream()), "cmk_resize_v_preprocess_hflip")
        del keep
        out.append(canvas)
    return out


def tta_table(augs, h: int, w: int, to_image: bool, device) -> torch.Tensor:
    """The (A,5) float32 table of the box maps for augmentations [(new_h, new_w, flip)] of an h x w image: (new_w, new_h, rx, ry, flip)
    with rx, ry = w / new_w, h / new_h (to_image) or their inverses, each computed in double and rounded once to fp32."""
    import numpy as np
    rows = [(nw, nh, np.float32(w / nw if to_image else nw / w), np.float32(h / nh if to_image else nh / h), 1.0 if flip else 0.0)
            for nh, nw, flip in augs]
    return torch.tensor(np.asarray(rows, dtype=np.float32)).to(device)


def _need_tta(t, dtype, shape, what: str) -> None:
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _lib.CmkError("{}: need a contiguous {} tensor of shape {}, got {}".format(
            what, dtype, tuple(shape), "{} {}".format(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    if not t.is_cuda:
        raise _lib.CmkError("{}: tensor is on {}; the CenterMask2 HIP path needs a GPU (no CPU fallback)".format(what, t.device))
    _need_current_device(t, what)


def tta_boxes_to_image(det: dict, table: torch.Tensor, height: int, width: int) -> dict:
    """det: the padded detections of A augmentations (box (A,K,4), score (A,K), cls (A,K) int64, loc (A,K,2), counts (A) int32) and the
    to_image table -> one ops.nms_topk candidate set (1, A*K, ..) in the frame of the height x width image: flipped back, scaled,
    clipped; compacted in augmentation order, counts = [the sum]."""
    lib = _lib.load()
    a, k = int(det["score"].shape[0]), int(det["score"].shape[1])
    dev = det["score"].device
    for name, dt, shp in (("box", torch.float32, (a, k, 4)), ("score", torch.float32, (a, k)), ("cls", torch.int64, (a, k)),
                          ("loc", torch.float32, (a, k, 2)), ("counts", torch.int32, (a,))):
        _need_tta(det[name], dt, shp, "tta_boxes_to_image " + name)
    _need_tta(table, torch.float32, (a, 5), "tta_boxes_to_image table")
    cap = a * k
    cand = dict(box=torch.empty((1, cap, 4), dtype=torch.float32, device=dev), score=torch.empty((1, cap), dtype=torch.float32, device=dev),
                cls=torch.empty((1, cap), dtype=torch.int32, device=dev), loc=torch.empty((1, cap, 2), dtype=torch.float32, device=dev),
                counts=torch.empty((1,), dtype=torch.int32, device=dev), cap=cap)
    check(lib.cmk_tta_boxes_to_image(det["box"].data_ptr(), det["score"].data_ptr(), det["cls"].data_ptr(), det["loc"].data_ptr(),
                                     det["counts"].data_ptr(), table.data_ptr(), a, k, int(width), int(height), cand["box"].data_ptr(),
                                     cand["score"].data_ptr(), cand["cls"].data_ptr(), cand["loc"].data_ptr(), cand["counts"].data_ptr(),
                                     _stream()), "cmk_tta_boxes_to_image")
    return cand


def tta_boxes_to_aug(box: torch.Tensor, count: torch.Tensor, table: torch.Tensor):
    """Merged boxes (K,4) in the image frame, count (1) int32 and the to_aug table (A,5) -> (boxes (A,K,4) in every augmentation's frame
    with zero rows at and beyond the count, counts (A) int32)."""
    lib = _lib.load()
    k, a = int(box.shape[0]), int(table.shape[0])
    _need_tta(box, torch.float32, (k, 4), "tta_boxes_to_aug box")
    _need_tta(count, torch.int32, (1,), "tta_boxes_to_aug count")
    _need_tta(table, torch.float32, (a, 5), "tta_boxes_to_aug table")
    out = torch.empty((a, k, 4), dtype=torch.float32, device=box.device)
    counts = torch.empty((a,), dtype=torch.int32, device=box.device)
    check(lib.cmk_tta_boxes_to_aug(box.data_ptr(), count.data_ptr(), table.data_ptr(), a, k, out.data_ptr(), counts.data_ptr(), _stream()),
          "cmk_tta_boxes_to_aug")
    return out, counts


def tta_reduce_masks(masks: torch.Tensor, flips: torch.Tensor, mask_scores: Optional[torch.Tensor], count: torch.Tensor):
    """masks (A,K,S,S) soft masks, flips (A) int32, mask_scores (A,K) or None, count (1) int32 -> (masks (K,S,S), mask_scores (K) or
    None): the mean over the augmentations with the flipped ones mirrored along x, summed in augmentation order from 0 and divided once
    by float(A); zero rows at and beyond the count."""
    lib = _lib.load()
    if not torch.is_tensor(masks) or masks.dim() != 4 or masks.shape[2] != masks.shape[3]:
        raise _lib.CmkError("tta_reduce_masks: need (A,K,S,S) masks")
    a, k, s = int(masks.shape[0]), int(masks.shape[1]), int(masks.shape[2])
    _need_tta(masks, torch.float32, (a, k, s, s), "tta_reduce_masks masks")
    _need_tta(flips, torch.int32, (a,), "tta_reduce_masks flips")
    _need_tta(count, torch.int32, (1,), "tta_reduce_masks count")
    if mask_scores is not None:
        _need_tta(mask_scores, torch.float32, (a, k), "tta_reduce_masks mask_scores")
    out = torch.empty((k, s, s), dtype=torch.float32, device=masks.device)
    out_ms = torch.empty((k,), dtype=torch.float32, device=masks.device) if mask_scores is not None else None
    check(lib.cmk_tta_reduce_masks(masks.data_ptr(), flips.data_ptr(), mask_scores.data_ptr() if mask_scores is not None else None,
                                   count.data_ptr(), a, k, s, out.data_ptr(), out_ms.data_ptr() if out_ms is not None else None, _stream()),
          "cmk_tta_reduce_masks")
    return out, out_ms


# ---------------------------------------------------------------------------------------------------------------
# sliced inference (modeling/sliced_inference.py): the tile grid, the per-pass table and the map back into the image frame
# ---------------------------------------------------------------------------------------------------------------
def slice_grid(h: int, w: int, tile_h: int, tile_w: int, overlap: float) -> List[Tuple[int, int, int, int]]:
    """The tiles [(y0, x0, th, tw)] of an h x w image in row-major order.  th = min(tile_h, h), tw = min(tile_w, w); per axis the
    stride is max(1, int(t * (1 - overlap))), the starts are 0, stride, 2 * stride, .. while start + t < size, and the last start is
    size - t: the last tile is shifted back and ends on the image border.  Every tile has the same size; repeated windows are dropped."""
    h, w, tile_h, tile_w = int(h), int(w), int(tile_h), int(tile_w)
    if h < 1 or w < 1 or tile_h < 1 or tile_w < 1 or not 0.0 <= float(overlap) < 1.0:
        raise ValueError("slice_grid: need a positive image and tile and 0 <= overlap < 1, got {}x{}, tile {}x{}, overlap {}".format(
            h, w, tile_h, tile_w, overlap))

    def starts(size, t):
        stride = max(1, int(t * (1.0 - float(overlap))))
        out, s = [], 0
        while s + t < size:
            out.append(s)
            s += stride
        if size - t not in out:
            out.append(size - t)
        return out

    th, tw = min(tile_h, h), min(tile_w, w)
    return [(y0, x0, th, tw) for y0 in starts(h, th) for x0 in starts(w, tw)]


def slice_table(passes, device) -> torch.Tensor:
    """The (A,6) float32 table of slice_boxes_to_image for passes [(y0, x0, th, tw, new_h, new_w)]: (x0, y0, rx, ry, tw, th) with
    rx, ry = tw / new_w, th / new_h, each computed in double and rounded once to fp32."""
    import numpy as np
    rows = [(x0, y0, np.float32(tw / nw), np.float32(th / nh), tw, th) for y0, x0, th, tw, nh, nw in passes]
    return torch.tensor(np.asarray(rows, dtype=np.float32)).to(device)


def slice_boxes_to_image(det: dict, table: torch.Tensor, height: int, width: int) -> dict:
    """det: the padded detections of A passes (box (A,K,4), score (A,K), cls (A,K) int64, loc (A,K,2), counts (A) int32) and their
    slice_table -> one ops.nms_topk candidate set (1, A*K, ..) in the frame of the height x width image: scaled, shifted to the pass's
    corner, clipped to the pass's window; compacted in pass order, counts = [the sum]; src (A*K) int32 = the padded slot a*K + k of
    every candidate."""
    lib = _lib.load()
    if not torch.is_tensor(det["score"]) or det["score"].dim() != 2:
        raise _lib.CmkError("slice_boxes_to_image: need (A,K) scores")
    a, k = int(det["score"].shape[0]), int(det["score"].shape[1])
    dev = det["score"].device
    for name, dt, shp in (("box", torch.float32, (a, k, 4)), ("score", torch.float32, (a, k)), ("cls", torch.int64, (a, k)),
                          ("loc", torch.float32, (a, k, 2)), ("counts", torch.int32, (a,))):
        _need_tta(det[name], dt, shp, "slice_boxes_to_image " + name)
    _need_tta(table, torch.float32, (a, 6), "slice_boxes_to_image table")
    cap = a * k
    cand = dict(box=torch.empty((1, cap, 4), dtype=torch.float32, device=dev), score=torch.empty((1, cap), dtype=torch.float32, device=dev),
                cls=torch.empty((1, cap), dtype=torch.int32, device=dev), loc=torch.empty((1, cap, 2), dtype=torch.float32, device=dev),
                counts=torch.empty((1,), dtype=torch.int32, device=dev), src=torch.empty((cap,), dtype=torch.int32, device=dev), cap=cap)
    check(lib.cmk_slice_boxes_to_image(det["box"].data_ptr(), det["score"].data_ptr(), det["cls"].data_ptr(), det["loc"].data_ptr(),
                                       det["counts"].data_ptr(), table.data_ptr(), a, k, int(width), int(height), cand["box"].data_ptr(),
                                       cand["score"].data_ptr(), cand["cls"].data_ptr(), cand["loc"].data_ptr(), cand["src"].data_ptr(),
                                       cand["counts"].data_ptr(), _stream()), "cmk_slice_boxes_to_image")
    return cand


def paste_masks(masks: torch.Tensor, boxes: torch.Tensor, height: int, width: int, threshold: float = 0.5) -> torch.Tensor:
    """(R,S,S) float masks + (R,4) boxes -> (R,height,width) bool bitmasks."""
    lib = _lib.load()
    r, s = masks.shape[0], masks.shape[-1]
    out = torch.empty((r, height, width), dtype=torch.uint8, device=masks.device)
    if r:
        _need_gpu(masks, "paste_masks")
        check(lib.cmk_paste_masks(masks.contiguous().data_ptr(), boxes.contiguous().float().data_ptr(), r, s, height, width, float(threshold),
                                  out.data_ptr(), _stream()), "cmk_paste_masks")
    return out.bool()


def mask_rle(masks: torch.Tensor):
    """(R,H,W) bool bitmasks on the GPU -> (counts, strings): per mask the COCO run lengths (int32 CPU tensor, the uncompressed form)
    and the compressed string, byte for byte what wire.rle_counts / wire.rle_to_string give (coco_evaluation.py:362-427).
    Two host synchronisations: the run totals after the count phase, which size every output exactly (7 bytes bound the characters of
    one count), then one download of lengths, counts and bytes after the encode phase."""
    lib = _lib.load()
    if not torch.is_tensor(masks) or not masks.is_cuda:
        raise _lib.CmkError("mask_rle: masks are on {}; the device encoder needs a GPU (no CPU fallback; wire.rle_encode is the host codec)".format(
            masks.device if torch.is_tensor(masks) else type(masks).__name__))
    if masks.dtype != torch.bool or masks.dim() != 3:
        raise _lib.CmkError("mask_rle: expected (R,H,W) bool bitmasks, got {} {}".format(masks.dtype, tuple(masks.shape)))
    _need_current_device(masks, "mask_rle")
    masks = masks.contiguous()
    r, h, w = masks.shape
    if r == 0:
        return [], []
    dev = masks.device
    ws_bytes = lib.cmk_rle_ws_bytes(r, h, w)
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=dev)
    n_runs = torch.empty((r,), dtype=torch.int32, device=dev)
    check(lib.cmk_rle_count(masks.data_ptr(), r, h, w, ws.data_ptr(), ws_bytes, n_runs.data_ptr(), _stream()), "cmk_rle_count")
    n_host = n_runs.cpu().numpy().astype("int64")                      # synchronisation 1
    total = int(n_host.sum())
    # one buffer, one download: [lens R int64 | counts total int32 | bytes 7*total]
    out = torch.empty((8 * r + 11 * total,), dtype=torch.uint8, device=dev)
    starts = torch.empty((total,), dtype=torch.int32, device=dev)
    p = out.data_ptr()
    check(lib.cmk_rle_encode(masks.data_ptr(), r, h, w, ws.data_ptr(), ws_bytes, n_runs.data_ptr(), starts.data_ptr(), p + 8 * r,
                             p + 8 * r + 4 * total, p, _stream()), "cmk_rle_encode")
    host = out.cpu()                                                   # synchronisation 2
    lens = host[:8 * r].view(torch.int64).tolist()
    all_counts = host[8 * r:8 * r + 4 * total].view(torch.int32)
    data = host[8 * r + 4 * total:].numpy()
    counts, strings, off = [], [], 0
    for k in range(r):
        n = int(n_host[k])
        counts.append(all_counts[off:off + n].clone())
        strings.append(data[7 * off:7 * off + lens[k]].tobytes().decode("ascii"))
        off += n
    return counts, strings


def _need_bitmasks(masks, what: str) -> torch.Tensor:
    """The input check of the mask entries, as mask_rle makes it: (R,H,W) bool on the current GPU, made contiguous."""
    if not torch.is_tensor(masks) or not masks.is_cuda:
        raise _lib.CmkError("{}: masks are on {}; the device path needs a GPU (no CPU fallback; coco_eval.intersections_host is the host "
                            "path)".format(what, masks.device if torch.is_tensor(masks) else type(masks).__name__))
    if masks.dtype != torch.bool or masks.dim() != 3:
        raise _lib.CmkError("{}: expected (R,H,W) bool bitmasks, got {} {}".format(what, masks.dtype, tuple(masks.shape)))
    _need_current_device(masks, what)
    return masks.contiguous()


def mask_words(h: int, w: int) -> int:
    """64-bit words of one packed (h,w) mask."""
    return (int(h) * int(w) + 63) // 64


def _pack_bits_into(masks: torch.Tensor, words: torch.Tensor, areas: torch.Tensor) -> None:
    r, h, w = masks.shape
    check(_lib.load().cmk_mask_pack_bits(masks.data_ptr(), r, h, w, words.data_ptr(), areas.data_ptr(), _stream()), "cmk_mask_pack_bits")


def mask_pack_bits(masks: torch.Tensor):
    """(R,H,W) bool bitmasks on the GPU -> (words, areas) on the GPU: words (R, ceil(H*W/64)) int64 holding the 64-bit words of
    include/cmk.h's packed masks (bit p % 64 of word p / 64 is the row-major pixel p; unused high bits zero), areas (R,) int32."""
    masks = _need_bitmasks(masks, "mask_pack_bits")
    r, h, w = masks.shape
    if h < 1 or w < 1:
        raise _lib.CmkError("mask_pack_bits: empty {}x{} masks".format(h, w))
    words = torch.empty((r, mask_words(h, w)), dtype=torch.int64, device=masks.device)
    areas = torch.empty((r,), dtype=torch.int32, device=masks.device)
    if r:
        _pack_bits_into(masks, words, areas)
    return words, areas


def _rle_prefix_sums(counts_list, h: int, w: int, what: str):
    """COCO run lengths per mask (lists or int tensors) -> (cum int32 (T,), off int64 (M+1,)) as NumPy arrays, after the check the
    kernel relies on: no negative run and every mask's runs add up to h*w."""
    import numpy as np
    h, w = int(h), int(w)
    if h < 1 or w < 1 or h * w >= 2 ** 31 - 1:
        raise _lib.CmkError("{}: size {}x{} is outside what int32 positions hold".format(what, h, w))
    cums, off = [], [0]
    for k, c in enumerate(counts_list):
        c = (c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)).astype(np.int64).reshape(-1)
        if c.size == 0 or (c < 0).any() or int(c.sum()) != h * w:
            raise _lib.CmkError("{}: the runs of mask {} add up to {}, not to {}x{} = {} (or one is negative)".format(
                what, k, int(c.sum()), h, w, h * w))
        cums.append(np.cumsum(c).astype(np.int32))
        off.append(off[-1] + c.size)
    cum = np.concatenate(cums) if cums else np.zeros((0,), dtype=np.int32)
    return cum, np.asarray(off, dtype=np.int64)


def _rle_decode_pack(counts_list, h: int, w: int, want_bitmasks: bool, words: Optional[torch.Tensor] = None,
                     areas: Optional[torch.Tensor] = None):
    """-> (words, areas, bitmasks or None) on the current GPU; words/areas may be views to fill (mask_intersections)."""
    cum, off = _rle_prefix_sums(counts_list, h, w, "mask_rle_decode")
    m = len(off) - 1
    dev = torch.device("cuda", torch.cuda.current_device())
    if words is None:
        words = torch.empty((m, mask_words(h, w)), dtype=torch.int64, device=dev)
        areas = torch.empty((m,), dtype=torch.int32, device=dev)
    bits = torch.empty((m, int(h), int(w)), dtype=torch.uint8, device=dev) if want_bitmasks else None
    if m:
        # one upload: [off (m+1) int64 | cum T int32]
        host = torch.from_numpy(off).view(torch.uint8)
        buf = torch.cat([host, torch.from_numpy(cum).view(torch.uint8)]).to(dev)
        p = buf.data_ptr()
        check(_lib.load().cmk_rle_decode_pack(p + 8 * (m + 1), p, m, int(h), int(w), words.data_ptr(), areas.data_ptr(),
                                              bits.data_ptr() if want_bitmasks else None, _stream()), "cmk_rle_decode_pack")
    return words, areas, bits


def mask_rle_decode(counts_list, h: int, w: int, want_bitmasks: bool = True):
    """The inverse of mask_rle: per mask the COCO run lengths (lists or int32 tensors, as mask_rle returns them; column-major, zeros
    run first) -> (M,h,w) bool bitmasks on the current GPU.  With want_bitmasks=False the bitmaps are not written and the packed
    (words, areas) of mask_pack_bits come back instead.  Runs that do not add up to h*w are refused before the launch."""
    words, areas, bits = _rle_decode_pack(counts_list, h, w, want_bitmasks)
    return bits.bool() if want_bitmasks else (words, areas)


def mask_intersections(det_masks: torch.Tensor, gt_counts, h: int, w: int):
    """Detection bitmasks (N,h,w) bool on the GPU against M ground truths given as COCO run lengths -> (inter (N,M), det_areas (N,),
    gt_areas (M,)), int32 CPU tensors: pixels in both, and in each.  The bitmaps stay on the device; what crosses the host link is the
    runs up and N*M + N + M integers down, in one copy."""
    det_masks = _need_bitmasks(det_masks, "mask_intersections")
    n, m = int(det_masks.shape[0]), len(gt_counts)
    if tuple(det_masks.shape[1:]) != (int(h), int(w)):
        raise _lib.CmkError("mask_intersections: detections are {}x{}, the ground truth {}x{}".format(det_masks.shape[1], det_masks.shape[2], h, w))
    nw = mask_words(h, w)
    dev = det_masks.device
    out = torch.empty((n * m + n + m,), dtype=torch.int32, device=dev)
    inter, det_areas, gt_areas = out[:n * m], out[n * m:n * m + n], out[n * m + n:]
    words = torch.empty((n + m, nw), dtype=torch.int64, device=dev)
    if n:
        _pack_bits_into(det_masks, words[:n], det_areas)
    with torch.cuda.device(dev):
        _rle_decode_pack(gt_counts, h, w, False, words[n:], gt_areas)
    if n and m:
        check(_lib.load().cmk_mask_intersections(words.data_ptr(), n, words[n:].data_ptr(), m, int(h), int(w), inter.data_ptr(), _stream()),
              "cmk_mask_intersections")
    host = out.cpu()                                                   # the one download
    return host[:n * m].reshape(n, m), host[n * m:n * m + n], host[n * m + n:]


def boundary_dilation(h: int, w: int, ratio: float = 0.02) -> int:
    """The erosion distance of Boundary IoU (Cheng et al., CVPR 2021) for an (h,w) image, on the host:
    max(1, int(round(ratio * sqrt(h*h + w*w)))) with Python's round."""
    from . import coco_eval
    return coco_eval.boundary_dilation(h, w, ratio)


def _boundary_bits_into(words: torch.Tensor, h: int, w: int, dilation: int, bwords: torch.Tensor, bareas: torch.Tensor) -> None:
    check(_lib.load().cmk_mask_boundary_bits(words.data_ptr(), int(words.shape[0]), int(h), int(w), int(dilation), bwords.data_ptr(),
                                             bareas.data_ptr(), _stream()), "cmk_mask_boundary_bits")


def _need_words(words, h: int, w: int, what: str) -> torch.Tensor:
    if not torch.is_tensor(words) or not words.is_cuda:
        raise _lib.CmkError("{}: words are on {}; the device path needs a GPU (no CPU fallback; coco_eval.boundary_host is the host "
                            "path)".format(what, words.device if torch.is_tensor(words) else type(words).__name__))
    if int(h) < 1 or int(w) < 1:
        raise _lib.CmkError("{}: empty {}x{} masks".format(what, h, w))
    if words.dtype != torch.int64 or words.dim() != 2 or words.shape[1] != mask_words(h, w):
        raise _lib.CmkError("{}: expected (R, {}) int64 packed words of {}x{} masks, got {} {}".format(what, mask_words(h, w), h, w, words.dtype,
                                                                                                   tuple(words.shape)))
    _need_current_device(words, what)
    return words.contiguous()


def mask_boundary_bits(words: torch.Tensor, h: int, w: int, dilation: int):
    """Packed masks (R, mask_words(h,w)) int64 on the GPU, as mask_pack_bits and mask_rle_decode(.., want_bitmasks=False) give them ->
    (bwords, bareas) on the GPU in the same conventions: the packed boundary of each mask at erosion distance `dilation` (mask AND NOT
    its (2d+1)x(2d+1) square erosion, outside the image background; include/cmk.h) and its set pixels.  No bitmap is touched."""
    words = _need_words(words, h, w, "mask_boundary_bits")
    bwords = torch.empty_like(words)
    bareas = torch.empty((words.shape[0],), dtype=torch.int32, device=words.device)
    if words.shape[0]:
        _boundary_bits_into(words, h, w, dilation, bwords, bareas)
    return bwords, bareas


def mask_unpack_bits(words: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """The inverse of mask_pack_bits: (R, mask_words(h,w)) int64 on the GPU -> (R,h,w) bool."""
    words = _need_words(words, h, w, "mask_unpack_bits")
    r = int(words.shape[0])
    out = torch.empty((r, int(h), int(w)), dtype=torch.uint8, device=words.device)
    if r:
        check(_lib.load().cmk_mask_unpack_bits(words.data_ptr(), r, int(h), int(w), out.data_ptr(), _stream()), "cmk_mask_unpack_bits")
    return out.bool()


LABEL_MAX_COLS = 4096       # CMK_LABEL_MAX_COLS of include/cmk.h


def mask_label_counts(masks: torch.Tensor, cols, num_cols: int):
    """Bitmasks (N,h,w) bool on the GPU against one label image: cols (h,w) uint16 on the host, the column of each pixel ->
    (table (N,num_cols), areas (N,)), int32 CPU tensors: table[n, c] = the pixels of mask n whose column is c (a column >= num_cols is
    counted nowhere), areas[n] = the pixels of mask n.  The bitmaps stay on the device, packed to bits; what crosses the host link is
    the label image up and N*num_cols + N integers down, in one copy each."""
    import numpy as np
    masks = _need_bitmasks(masks, "mask_label_counts")
    n, h, w = (int(v) for v in masks.shape)
    cols = np.ascontiguousarray(cols)
    if cols.dtype != np.uint16 or cols.shape != (h, w):
        raise _lib.CmkError("mask_label_counts: expected ({}, {}) uint16 columns on the host, got {} {}".format(h, w, cols.dtype, cols.shape))
    c = int(num_cols)
    if not 1 <= c <= LABEL_MAX_COLS:
        raise _lib.CmkError("mask_label_counts: {} columns outside [1, {}]".format(c, LABEL_MAX_COLS))
    if h < 1 or w < 1:
        raise _lib.CmkError("mask_label_counts: empty {}x{} masks".format(h, w))
    if n == 0:
        return torch.zeros((0, c), dtype=torch.int32), torch.zeros((0,), dtype=torch.int32)
    dev = masks.device
    out = torch.empty((n * c + n,), dtype=torch.int32, device=dev)
    words = torch.empty((n, mask_words(h, w)), dtype=torch.int64, device=dev)
    _pack_bits_into(masks, words, out[n * c:])
    cols_dev = torch.from_numpy(cols.view(np.int16)).to(dev)          # the one upload (torch has no uint16 arithmetic; the bits are kept)
    check(_lib.load().cmk_mask_label_counts(words.data_ptr(), n, cols_dev.data_ptr(), h, w, c, out.data_ptr(), _stream()),
          "cmk_mask_label_counts")
    host = out.cpu()                                                   # the one download
    return host[:n * c].reshape(n, c), host[n * c:]


def mask_boundary(masks: torch.Tensor, dilation: Optional[int] = None) -> torch.Tensor:
    """(R,h,w) bool bitmasks on the GPU -> (R,h,w) bool, their boundaries: packed, eroded on the packed words and unpacked, all on the
    device.  dilation defaults to boundary_dilation(h, w)."""
    masks = _need_bitmasks(masks, "mask_boundary")
    h, w = int(masks.shape[1]), int(masks.shape[2])
    words, _ = mask_pack_bits(masks)
    bwords, _ = mask_boundary_bits(words, h, w, boundary_dilation(h, w) if dilation is None else dilation)
    return mask_unpack_bits(bwords, h, w)


def _contour_count(words: torch.Tensor, h: int, w: int):
    """Count phase of mask_contours_bits -> (ws, ws_bytes, n_corners on the device).  Launches only."""
    lib = _lib.load()
    r = int(words.shape[0])
    ws_bytes = lib.cmk_vis_contour_ws_bytes(r, int(h), int(w))
    if ws_bytes <= 0:
        raise _lib.CmkError("mask_contours_bits: {} masks of {}x{} are outside what the contour kernels take (include/cmk.h)".format(r, h, w))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=words.device)
    n_dev = torch.empty((r,), dtype=torch.int32, device=words.device)
    check(lib.cmk_vis_contour_count(words.data_ptr(), r, int(h), int(w), ws.data_ptr(), ws_bytes, n_dev.data_ptr(), _stream()),
          "cmk_vis_contour_count")
    return ws, ws_bytes, n_dev


def _contour_trace(words: torch.Tensor, h: int, w: int, ws: torch.Tensor, ws_bytes: int, n_host) -> torch.Tensor:
    """Trace phase of mask_contours_bits: n_host the totals as a contiguous int32 NumPy array, their sum T > 0 -> int32 (3 T,) on the
    device, [xy 2 T | head T].  Launches only."""
    lib = _lib.load()
    total = int(n_host.astype("int64").sum())
    scratch_bytes = lib.cmk_vis_contour_trace_ws_bytes(total)
    scratch = torch.empty((scratch_bytes,), dtype=torch.uint8, device=words.device)
    out = torch.empty((3 * total,), dtype=torch.int32, device=words.device)
    p = out.data_ptr()
    check(lib.cmk_vis_contour_trace(words.data_ptr(), int(words.shape[0]), int(h), int(w), ws.data_ptr(), ws_bytes, n_host.ctypes.data,
                                    scratch.data_ptr(), scratch_bytes, p, p + 8 * total, _stream()), "cmk_vis_contour_trace")
    return out


def _contour_split(host, n_host):
    """[xy 2 T | head T] on the host and the totals per mask -> per mask the list of its loops, (k,2) int32 arrays."""
    import numpy as np
    total = int(n_host.astype("int64").sum())
    xy, head = host[:2 * total].reshape(total, 2), host[2 * total:]
    starts = np.flatnonzero(head)
    out, off = [], 0
    for n in n_host.tolist():
        cuts = starts[np.searchsorted(starts, off):np.searchsorted(starts, off + n)]
        out.append([xy[a:b].copy() for a, b in zip(cuts, list(cuts[1:]) + [off + n])])
        off += n
    return out


def mask_contours_bits(words: torch.Tensor, h: int, w: int):
    """Packed masks (R, mask_words(h,w)) int64 on the GPU -> a list of R lists of np.int32 arrays (k,2): the closed loops of lattice
    vertices (x, y) that outline each mask exactly (include/cmk.h, DESIGN §3 "Contours": foreground 4-connected and on the right of the
    walk, right turn at a saddle, corners only, a loop starts at its smallest (y, x) vertex, loops sorted by start, outer boundaries
    with a positive doubled area and holes with a negative one).  No bitmap is touched.  Two host synchronisations: the corner totals
    after the count phase, which size every buffer exactly, then one download of vertices and loop heads."""
    import numpy as np
    words = _need_words(words, h, w, "mask_contours_bits")
    r = int(words.shape[0])
    if r == 0:
        return []
    ws, ws_bytes, n_dev = _contour_count(words, h, w)
    n_host = np.ascontiguousarray(n_dev.cpu().numpy(), dtype=np.int32)  # synchronisation 1
    if (n_host < 0).any() or int(n_host.astype("int64").sum()) > 2 ** 31 - 1:
        raise _lib.CmkError("mask_contours_bits: the corners of the masks do not fit int32")
    if int(n_host.sum()) == 0:
        return [[] for _ in range(r)]
    host = _contour_trace(words, h, w, ws, ws_bytes, n_host).cpu().numpy()   # synchronisation 2
    return _contour_split(host, n_host)


def mask_contours(masks: torch.Tensor):
    """(R,H,W) bool bitmasks on the GPU -> their contours as mask_contours_bits gives them, packed first (mask_pack_bits); the bitmaps
    are not downloaded.  wire.mask_contours_host is the host path, wire.contours_to_polygons turns the result into COCO polygons."""
    masks = _need_bitmasks(masks, "mask_contours")
    if masks.shape[0] == 0:
        return []
    words, _ = mask_pack_bits(masks)
    return mask_contours_bits(words, int(masks.shape[1]), int(masks.shape[2]))


def mask_boundary_intersections(det_masks: torch.Tensor, gt_counts, h: int, w: int, dilation: int):
    """mask_intersections and the same for the boundaries of the masks (Boundary IoU): -> (inter (N,M), det_areas (N,), gt_areas (M,),
    inter_b (N,M), det_areas_b (N,), gt_areas_b (M,)), int32 CPU tensors.  The detections are packed and the ground truths decoded once,
    both sets eroded on the packed words (cmk_mask_boundary_bits), the table kernel runs twice; one download of 2*(N*M + N + M) integers."""
    det_masks = _need_bitmasks(det_masks, "mask_boundary_intersections")
    n, m = int(det_masks.shape[0]), len(gt_counts)
    if tuple(det_masks.shape[1:]) != (int(h), int(w)):
        raise _lib.CmkError("mask_boundary_intersections: detections are {}x{}, the ground truth {}x{}".format(det_masks.shape[1], det_masks.shape[2],
                                                                                                         h, w))
    nw = mask_words(h, w)
    dev = det_masks.device
    one = n * m + n + m
    out = torch.empty((2 * one,), dtype=torch.int32, device=dev)
    words = torch.empty((2, n + m, nw), dtype=torch.int64, device=dev)           # the masks, then their boundaries
    if n:
        _pack_bits_into(det_masks, words[0, :n], out[n * m:n * m + n])
    with torch.cuda.device(dev):
        _rle_decode_pack(gt_counts, h, w, False, words[0, n:], out[n * m + n:one])
    if n + m:
        _boundary_bits_into(words[0], h, w, dilation, words[1], out[one + n * m:])
    if n and m:
        lib = _lib.load()
        for k in (0, 1):
            check(lib.cmk_mask_intersections(words[k].data_ptr(), n, words[k, n:].data_ptr(), m, int(h), int(w), out[k * one:].data_ptr(), _stream()),
                  "cmk_mask_intersections")
    host = out.cpu()                                                   # the one download
    return tuple(host[k * one + a:k * one + b].reshape(shape) for k in (0, 1)
                 for a, b, shape in ((0, n * m, (n, m)), (n * m, n * m + n, (n,)), (n * m + n, one, (m,))))


# ---- visualizer (csrc/visualize.hip; the contract is in include/cmk.h and DESIGN §3 "Visualizer") ------------------------------------
def _vis_prepare(entry: str, boxes, scores, classes, order, names, name_lens, num_names, palette, h, w, font_scale, color_by_class, color_ids):
    n = int(boxes.shape[0])
    for t, dt, what in ((boxes, torch.float32, "boxes"), (scores, torch.float32, "scores"), (classes, torch.int64, "classes"),
                        (order, torch.int64, "order"), (names, torch.uint8, "names"), (name_lens, torch.int32, "name_lens"),
                        (palette, torch.uint8, "palette")) + (((color_ids, torch.int32, "color_ids"),) if color_ids is not None else ()):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise _lib.CmkError("{}: {} must be contiguous {} on the GPU, got {} {} on {}".format(entry, what, dt, t.dtype, tuple(t.shape), t.device))
    if tuple(boxes.shape) != (n, 4) or scores.numel() != n or classes.numel() != n or order.numel() != n or palette.numel() != 192 \
            or names.numel() < 32 * num_names or name_lens.numel() < num_names:
        raise _lib.CmkError("{}: boxes {}, scores {}, classes {}, order {}, palette {}, names {} do not fit {} instances and {} names".format(
            entry, tuple(boxes.shape), tuple(scores.shape), tuple(classes.shape), tuple(order.shape), tuple(palette.shape), tuple(names.shape), n, num_names))
    if color_ids is not None and (tuple(color_ids.shape) != (n,) or color_ids.device != boxes.device):
        raise _lib.CmkError("{}: color_ids {} on {} do not fit {} instances on {}".format(entry, tuple(color_ids.shape), color_ids.device, n, boxes.device))
    _need_current_device(boxes, entry)
    lib = _lib.load()
    records = torch.empty((max(n, 1), lib.cmk_vis_record_ints()), dtype=torch.int32, device=boxes.device)
    args = (boxes.data_ptr(), scores.data_ptr(), classes.data_ptr(), order.data_ptr(), names.data_ptr(), name_lens.data_ptr(), int(num_names),
            palette.data_ptr(), n, int(h), int(w), int(font_scale), 1 if color_by_class else 0)
    if color_ids is None:
        check(lib.cmk_vis_prepare(*args, records.data_ptr(), _stream()), "cmk_vis_prepare")
    else:
        check(lib.cmk_vis_prepare_ids(*args, color_ids.data_ptr(), records.data_ptr(), _stream()), "cmk_vis_prepare_ids")
    return records


def vis_prepare(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, order: torch.Tensor, names: torch.Tensor,
                name_lens: torch.Tensor, num_names: int, palette: torch.Tensor, h: int, w: int, font_scale: int, color_by_class: bool) -> torch.Tensor:
    """Per-instance draw records in draw order, (max(n,1), cmk_vis_record_ints()) int32 on the boxes' device.  boxes (n,4) float32,
    scores (n,) float32, classes and order (n,) int64, names (rows,32) uint8 glyph indices, name_lens int32, palette (64,3) uint8."""
    return _vis_prepare("vis_prepare", boxes, scores, classes, order, names, name_lens, num_names, palette, h, w, font_scale, color_by_class, None)


def vis_prepare_ids(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, order: torch.Tensor, names: torch.Tensor,
                    name_lens: torch.Tensor, num_names: int, palette: torch.Tensor, h: int, w: int, font_scale: int, color_by_class: bool,
                    color_ids: torch.Tensor) -> torch.Tensor:
    """vis_prepare with the colour index of every instance given: color_ids (n,) int32 by original instance (track ids);
    col = palette[color_ids[k] mod 64], the remainder non-negative; color_by_class is not consulted."""
    if not torch.is_tensor(color_ids):
        raise _lib.CmkError("vis_prepare_ids: color_ids must be an (n,) int32 tensor on the GPU, got {}".format(type(color_ids).__name__))
    return _vis_prepare("vis_prepare_ids", boxes, scores, classes, order, names, name_lens, num_names, palette, h, w, font_scale, color_by_class, color_ids)


def vis_compose(image: torch.Tensor, words: Optional[torch.Tensor], records: torch.Tensor, n: int, font: torch.Tensor, line_width: int,
                font_scale: int, alpha256: int) -> torch.Tensor:
    """The picture of n records on a contiguous (h,w,3) uint8 GPU image -> a new tensor.  words: mask_pack_bits's (n, mask_words(h,w))
    int64 by original instance, or None for no masks."""
    if not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or not image.is_contiguous():
        raise _lib.CmkError("vis_compose: need a contiguous (h,w,3) uint8 image on the GPU, got {} {} on {}".format(image.dtype, tuple(image.shape), image.device))
    _need_current_device(image, "vis_compose")
    h, w = int(image.shape[0]), int(image.shape[1])
    lib = _lib.load()
    if n and (records.dtype != torch.int32 or records.numel() < n * lib.cmk_vis_record_ints() or records.device != image.device or font.numel() != 41 * 7
              or font.dtype != torch.uint8 or font.device != image.device):
        raise _lib.CmkError("vis_compose: records {} {} / font {} {} do not fit {} instances".format(records.dtype, tuple(records.shape), font.dtype,
                                                                                                   tuple(font.shape), n))
    if words is not None and (words.dtype != torch.int64 or tuple(words.shape) != (n, mask_words(h, w)) or not words.is_contiguous()
                              or words.device != image.device):
        raise _lib.CmkError("vis_compose: words must be contiguous ({}, {}) int64 on {}, got {} {}".format(n, mask_words(h, w), image.device, words.dtype,
                                                                                                       tuple(words.shape)))
    out = torch.empty_like(image)
    check(lib.cmk_vis_compose(image.data_ptr(), out.data_ptr(), h, w, None if words is None else words.data_ptr(), records.data_ptr(), int(n),
                              font.data_ptr(), int(line_width), int(font_scale), int(alpha256), _stream()), "cmk_vis_compose")
    return out


def vis_keypoints(image: torch.Tensor, keypoints: torch.Tensor, records: torch.Tensor, skeleton: Optional[torch.Tensor], threshold: float,
                  line_width: int, keypoint_color: int) -> None:
    """Skeleton segments and keypoint discs of (n,K,3) float32 keypoints, in place on the composed (h,w,3) image.  skeleton: (S,2) int32
    on the GPU or None; keypoint_color: bytes 0..2 are the image's channels."""
    if not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or not image.is_contiguous():
        raise _lib.CmkError("vis_keypoints: need a contiguous (h,w,3) uint8 image on the GPU, got {} {} on {}".format(image.dtype, tuple(image.shape), image.device))
    if keypoints.dim() != 3 or keypoints.shape[2] != 3 or keypoints.dtype != torch.float32 or not keypoints.is_contiguous() or keypoints.device != image.device:
        raise _lib.CmkError("vis_keypoints: need contiguous (n,K,3) float32 keypoints on {}, got {} {} on {}".format(image.device, keypoints.dtype,
                                                                                                                  tuple(keypoints.shape), keypoints.device))
    _need_current_device(image, "vis_keypoints")
    n, k = int(keypoints.shape[0]), int(keypoints.shape[1])
    nseg = 0 if skeleton is None else int(skeleton.shape[0])
    lib = _lib.load()
    if n and (records.dtype != torch.int32 or records.numel() < n * lib.cmk_vis_record_ints() or records.device != image.device):
        raise _lib.CmkError("vis_keypoints: records {} {} do not fit {} instances".format(records.dtype, tuple(records.shape), n))
    if nseg and (skeleton.dtype != torch.int32 or tuple(skeleton.shape) != (nseg, 2) or not skeleton.is_contiguous() or skeleton.device != image.device):
        raise _lib.CmkError("vis_keypoints: the skeleton must be contiguous (S,2) int32 on {}, got {} {}".format(image.device, skeleton.dtype, tuple(skeleton.shape)))
    h, w = int(image.shape[0]), int(image.shape[1])
    winner = torch.empty((h, w), dtype=torch.int32, device=image.device)
    check(lib.cmk_vis_keypoints(image.data_ptr(), h, w, keypoints.data_ptr(), records.data_ptr(), n, k, skeleton.data_ptr() if nseg else None, nseg,
                                float(threshold), int(line_width), int(keypoint_color), winner.data_ptr(), _stream()), "cmk_vis_keypoints")


# ---- video (csrc/visualize.hip; include/cmk.h and DESIGN §3 "Video") -----------------------------------------------------------------
MAX_TRACKS = 1024


def _need_track(t, dt, shape, dev, entry: str, what: str) -> None:
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != tuple(shape) or (dev is not None and t.device != dev):
        raise _lib.CmkError("{}: {} must be contiguous {} {} on {}, got {}".format(
            entry, what, dt, tuple(shape), dev if dev is not None else "the GPU",
            "{} {} on {}".format(t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))


def vis_track_iou_boxes(old_boxes: torch.Tensor, rows: int, new_boxes: torch.Tensor, iou: torch.Tensor) -> None:
    """Box mode: iou[:rows * n] (float64, row-major (rows, n)) of the first `rows` rows of a track table's boxes (max_tracks,4) float32
    against the new (n,4) float32 boxes.  iou: a flat float64 workspace of at least rows * n elements."""
    if not torch.is_tensor(old_boxes) or old_boxes.dim() != 2:
        raise _lib.CmkError("vis_track_iou_boxes: old_boxes must be a (max_tracks,4) tensor")
    cap, n, rows = int(old_boxes.shape[0]), int(new_boxes.shape[0]) if torch.is_tensor(new_boxes) and new_boxes.dim() == 2 else -1, int(rows)
    if not 1 <= cap <= MAX_TRACKS or not 0 <= n <= cap or not 0 <= rows <= cap:
        raise _lib.CmkError("vis_track_iou_boxes: max_tracks = {} (in [1, {}]), n = {}, rows = {} (both in [0, max_tracks])".format(cap, MAX_TRACKS, n, rows))
    _need_track(old_boxes, torch.float32, (cap, 4), None, "vis_track_iou_boxes", "old_boxes")
    dev = old_boxes.device
    _need_track(new_boxes, torch.float32, (n, 4), dev, "vis_track_iou_boxes", "new_boxes")
    if not torch.is_tensor(iou) or iou.dtype != torch.float64 or iou.device != dev or not iou.is_contiguous() or iou.numel() < rows * n:
        raise _lib.CmkError("vis_track_iou_boxes: iou must be contiguous float64 with at least {} elements on {}".format(rows * n, dev))
    _need_current_device(old_boxes, "vis_track_iou_boxes")
    check(_lib.load().cmk_vis_track_iou_boxes(old_boxes.data_ptr(), rows, new_boxes.data_ptr(), n, iou.data_ptr(), _stream()), "cmk_vis_track_iou_boxes")


def vis_track_assign(old: dict, out: dict, new_boxes: torch.Tensor, new_classes: torch.Tensor, rows: int, ttl: int, threshold: float,
                     src: torch.Tensor, counters: torch.Tensor, iou: Optional[torch.Tensor] = None, inter: Optional[torch.Tensor] = None,
                     new_areas: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One frame of the association rule (include/cmk.h) -> track_ids (n,) int32.  old / out: the two halves of the track table, dicts of
    boxes (max_tracks,4) float32, classes (max_tracks,) int64, ids and ttl (max_tracks,) int32 and, in mask mode, areas (max_tracks,) int32;
    src (max_tracks,) int32 and counters (4,) int32 (n_tracks, next_id, dropped, spare) on the same device.  Give `iou` (box mode, the
    workspace vis_track_iou_boxes filled) or `inter` with new_areas (mask mode, the table of cmk_mask_intersections).  Nothing is read back."""
    e = "vis_track_assign"
    if not isinstance(old, dict) or not isinstance(out, dict) or not torch.is_tensor(old.get("boxes")) or old["boxes"].dim() != 2:
        raise _lib.CmkError("vis_track_assign: old and out must be dicts of the table's tensors (boxes, classes, ids, ttl)")
    cap = int(old["boxes"].shape[0])
    n = int(new_boxes.shape[0]) if torch.is_tensor(new_boxes) and new_boxes.dim() == 2 else -1
    rows, ttl, threshold = int(rows), int(ttl), float(threshold)
    if not 1 <= cap <= MAX_TRACKS:
        raise _lib.CmkError("vis_track_assign: max_tracks = {} outside [1, {}]".format(cap, MAX_TRACKS))
    if not 0 <= n <= cap:
        raise _lib.CmkError("vis_track_assign: {} instances (boxes {}) outside [0, max_tracks = {}]".format(
            n, tuple(new_boxes.shape) if torch.is_tensor(new_boxes) else None, cap))
    if not 0 <= rows <= cap or not 1 <= ttl <= 255 or not 0.0 <= threshold <= 1.0:
        raise _lib.CmkError("vis_track_assign: rows = {} (in [0, {}]), ttl = {} (in [1, 255]), threshold = {} (in [0, 1])".format(rows, cap, ttl, threshold))
    dev = old["boxes"].device
    for half, name in ((old, "old"), (out, "out")):
        for key, dt, shape in (("boxes", torch.float32, (cap, 4)), ("classes", torch.int64, (cap,)), ("ids", torch.int32, (cap,)), ("ttl", torch.int32, (cap,))):
            _need_track(half.get(key), dt, shape, dev, e, name + "." + key)
    if any(old[k].data_ptr() == out[k].data_ptr() for k in ("boxes", "classes", "ids", "ttl")):
        raise _lib.CmkError("vis_track_assign: out is old; the update is out of place (two halves of a ping-pong pair)")
    _need_track(new_boxes, torch.float32, (n, 4), dev, e, "new_boxes")
    _need_track(new_classes, torch.int64, (n,), dev, e, "new_classes")
    _need_track(src, torch.int32, (cap,), dev, e, "src")
    _need_track(counters, torch.int32, (4,), dev, e, "counters")
    if n and rows:
        if (iou is None) == (inter is None):
            raise _lib.CmkError("vis_track_assign: give exactly one of iou (box mode) and inter (mask mode)")
        table, dt = (iou, torch.float64) if iou is not None else (inter, torch.int32)
        if not torch.is_tensor(table) or table.dtype != dt or table.device != dev or not table.is_contiguous() or table.numel() < rows * n:
            raise _lib.CmkError("vis_track_assign: the {} table must be contiguous {} with at least {} elements on {}".format(
                "iou" if iou is not None else "inter", dt, rows * n, dev))
        if inter is not None:
            _need_track(old.get("areas"), torch.int32, (cap,), dev, e, "old.areas")
            _need_track(new_areas, torch.int32, (n,), dev, e, "new_areas")
    _need_current_device(old["boxes"], e)
    track_ids = torch.empty((n,), dtype=torch.int32, device=dev)
    use = bool(n and rows)
    check(_lib.load().cmk_vis_track_assign(
        iou.data_ptr() if use and iou is not None else None, inter.data_ptr() if use and inter is not None else None,
        old["areas"].data_ptr() if use and inter is not None else None, new_areas.data_ptr() if use and inter is not None else None, rows,
        old["boxes"].data_ptr(), old["classes"].data_ptr(), old["ids"].data_ptr(), old["ttl"].data_ptr(),
        new_boxes.data_ptr() if n else None, new_classes.data_ptr() if n else None, n, cap, ttl, threshold,
        out["boxes"].data_ptr(), out["classes"].data_ptr(), out["ids"].data_ptr(), out["ttl"].data_ptr(), src.data_ptr(),
        track_ids.data_ptr() if n else None, counters.data_ptr(), _stream()), "cmk_vis_track_assign")
    return track_ids


def vis_track_gather(src: torch.Tensor, counters: torch.Tensor, old: dict, out: dict, new_words: torch.Tensor, new_areas: torch.Tensor,
                     rows: int, h: int, w: int) -> None:
    """Mask mode, after vis_track_assign: the words (max_tracks, mask_words(h,w)) int64 and areas (max_tracks,) int32 of `out` from the new
    instances' (n, mask_words(h,w)) words / (n,) areas and the `old` half, following src.  rows: an upper bound of the new n_tracks."""
    e = "vis_track_gather"
    h, w, rows = int(h), int(w), int(rows)
    if h < 1 or w < 1 or h * w >= 2 ** 31 - 1:
        raise _lib.CmkError("vis_track_gather: size {}x{} is outside what int32 positions hold".format(h, w))
    if not isinstance(old, dict) or not isinstance(out, dict) or not torch.is_tensor(old.get("words")) or old["words"].dim() != 2:
        raise _lib.CmkError("vis_track_gather: old and out must be dicts with the table's words and areas")
    cap, nw = int(old["words"].shape[0]), mask_words(h, w)
    n = int(new_words.shape[0]) if torch.is_tensor(new_words) and new_words.dim() == 2 else -1
    if not 1 <= cap <= MAX_TRACKS or not 0 <= n <= cap or not 0 <= rows <= cap:
        raise _lib.CmkError("vis_track_gather: max_tracks = {} (in [1, {}]), n = {}, rows = {} (both in [0, max_tracks])".format(cap, MAX_TRACKS, n, rows))
    _need_track(old["words"], torch.int64, (cap, nw), None, e, "old.words")
    dev = old["words"].device
    _need_track(old.get("areas"), torch.int32, (cap,), dev, e, "old.areas")
    _need_track(out.get("words"), torch.int64, (cap, nw), dev, e, "out.words")
    _need_track(out.get("areas"), torch.int32, (cap,), dev, e, "out.areas")
    _need_track(new_words, torch.int64, (n, nw), dev, e, "new_words")
    _need_track(new_areas, torch.int32, (n,), dev, e, "new_areas")
    _need_track(src, torch.int32, (cap,), dev, e, "src")
    _need_track(counters, torch.int32, (4,), dev, e, "counters")
    if old["words"].data_ptr() == out["words"].data_ptr() or old["areas"].data_ptr() == out["areas"].data_ptr():
        raise _lib.CmkError("vis_track_gather: out is old; the gather is out of place (two halves of a ping-pong pair)")
    _need_current_device(src, e)
    check(_lib.load().cmk_vis_track_gather(src.data_ptr(), counters.data_ptr(), old["words"].data_ptr(), old["areas"].data_ptr(),
                                           new_words.data_ptr() if n else None, new_areas.data_ptr() if n else None, n, rows, cap, h, w,
                                           out["words"].data_ptr(), out["areas"].data_ptr(), _stream()), "cmk_vis_track_gather")
