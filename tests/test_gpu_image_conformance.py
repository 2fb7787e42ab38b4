"""-m gpu: every row of the image-side conformance table (tests/image_cases.py) through the C ABI on real buffers, one test id per entry.

An accepted row is launched and checked for: its outputs against the reference of its entry; nothing written outside the outputs (every
buffer, inputs included, is the middle of a larger allocation of filler bytes: 0xFF for float buffers, which reads as NaN, 0x5A for the
others; the parts of an output the call must leave alone are checked for that filler too); every input bit-unchanged, its guards
included; the same call again into fresh buffers giving the same bits (the point of it for the atomics of mask_inter_kernel and
mask_boundary_kernel).  A refused row returns CMK_EINVAL with an error text and leaves every buffer it was handed untouched; a row with a
count of 0 returns OK and does the same.

References, none of them the code under test: tests/resize_ref.py (the int64 NumPy pass on the tables; for a damaged table the same sum
with the clamps include/cmk.h promises, which equals resize_ref on undamaged tables), one rounded fp32 NumPy operation per step for the
normalisation, tests/tta_ref.py, run lengths known by construction (mask_from_counts) or counted by np.diff on the column-major bitmap
and wire.rle_to_string, np.packbits, the int64 matrix product, tests/boundary_ref.py (the literal 3x3 iteration).  Every comparison is ==
(NaN where the reference has NaN) or bit-equality: there is no tolerance in this table."""
import ctypes

import numpy as np
import pytest
import torch

from centermask2_amd import ops, wire
from tests import boundary_ref as BR
from tests import conformance as C
from tests import image_cases as ic
from tests import resize_ref as RR
from tests import tta_ref as TR
from tests.test_gpu_rle import mask_from_counts, mask_set as rle_mask_set

pytestmark = pytest.mark.gpu

F = np.float32
CASES = ic.all_cases()
INDEX = {c["id"]: i for i, c in enumerate(CASES)}
SIZES = ("h", "w", "new_h", "new_w", "hp", "wp", "a", "k", "s", "r", "m", "n", "img_w", "img_h")
LONG_HEAD = [0, 1, 70000, 2, 40000, 33, 1, 1, 600000, 31, 32, 1023, 1024, 32767, 32768, 5]      # test_mask_rle_long_runs_and_signed_deltas
_SEEN = {}            # tta_reduce: (geometry, data) -> out_masks of the first row that ran it: the scalar kernel must give the vector kernel's bits


def _rng(c, k=0):
    return np.random.RandomState(7000 + 13 * INDEX[c["id"]] + k)


def _sane(c):
    """The row with a geometry that can be allocated (a refused row may say H = 0, K = 65536 or R = -1; an accepted one R = 0): it only
    sizes and fills the buffers, every one at least as large as an accepted call of the row's own arguments would need."""
    g, d = dict(c), ic.DEFAULTS[c["entry"]]
    for k in SIZES:
        if k in g and not 1 <= g[k] <= 5000:
            g[k] = d[k]
    if "d" in g and (c["answer"] == "refuse" or g["d"] < 1):
        g["d"] = d["d"]
    if "hp" in g:
        g["hp"], g["wp"] = max(g["hp"], g["new_h"]), max(g["wp"], g["new_w"])
    if "counts" in g and len(g["counts"]) != g["a"]:
        g["counts"] = [g["k"]] * g["a"]
    if "flips" in g and len(g["flips"]) != g["a"]:
        g["flips"] = ic.mixed(g["a"])
    return g


def _eq(got, ref, what):
    """== with NaN exactly where the reference has NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if ref.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN elsewhere than in the reference"
        ok = ~np.isnan(ref)
        assert np.array_equal(got[ok], ref[ok]), what + ": {} of {} values differ".format(int((got[ok] != ref[ok]).sum()), int(ok.sum()))
    else:
        assert np.array_equal(got, ref), what + ": {} of {} values differ".format(int((got != ref).sum()), ref.size)


class Bufs(C.Bufs):
    """The row's buffers from NumPy arrays: on the device they are bytes, on the host they come back in the array's own dtype."""
    TORCH = {"f4": torch.float32, "u1": torch.uint8, "i4": torch.int32, "i8": torch.int64, "u8": torch.int64}

    def __init__(self, dev):
        super().__init__(dev)
        self.np = {}               # output name -> its NumPy dtype

    def put(self, name, arr, **kw):
        arr = np.ascontiguousarray(arr)
        as_torch = self.TORCH[arr.dtype.str[1:]]
        return super().put(name, torch.from_numpy(arr.view(np.int64) if arr.dtype == np.uint64 else arr).view(as_torch), guard=kw.pop("guard", 256), **kw)

    def out(self, name, dtype, shape, **kw):
        self.np[name] = np.dtype(dtype)
        return super().out(name, shape, self.TORCH[self.np[name].str[1:]], guard=256, **kw)

    def host(self, got):
        return {name: t.numpy().view(self.np[name]) for name, t in got.items()}


# ---------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------
def _tables(in_size, out_size, damaged):
    """Pillow's tables of one axis; damaged: six rows of the bounds table broken, each by a few taps only (the guards are wider)."""
    bounds, kk, ks = ops.resize_coeffs(in_size, out_size)
    bounds = bounds.copy()
    if damaged:
        assert out_size >= 13
        bounds[1, 0] = -2                                   # lo < 0
        bounds[3, 0] = in_size + 3                          # lo > in
        bounds[5, 1] = -2                                   # n < 0
        bounds[7, 1] = ks + 3                               # n > ksize
        bounds[9] = (in_size - 1, 3)                        # lo + n > in
        bounds[11] = (-3, ks + 2)                           # both
    return bounds, kk, ks


def _resample_clamped(img, bounds, kk, ks, axis):
    """The sum of resize_ref.resample_pass over the tap ranges clamped as include/cmk.h says: lo into [0, in], n into [0, ksize] and in - lo."""
    in_size = img.shape[axis]
    lo = np.clip(bounds[:, 0].astype(np.int64), 0, in_size)
    n = np.minimum(np.clip(bounds[:, 1].astype(np.int64), 0, ks), in_size - lo)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(lo),) + src.shape[1:], dtype=np.uint8)
    for i in range(len(lo)):
        acc = (1 << (ops.RESIZE_BITS - 1)) + (src[lo[i]:lo[i] + n[i]] * kk[i, :n[i]].astype(np.int64)[:, None, None]).sum(axis=0)
        out[i] = np.clip(acc >> ops.RESIZE_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def _pass_ref(c, img, out_size, axis, tables):
    bounds, kk, ks = tables
    if c["data"] == "damaged":
        clean = ops.resize_coeffs(img.shape[axis], out_size)
        assert np.array_equal(_resample_clamped(img, clean[0], clean[1], ks, axis), RR.resample_pass(img, out_size, axis)), "the clamped sum is resize_ref on clean tables"
        ref = _resample_clamped(img, bounds, kk, ks, axis)
        assert not np.array_equal(ref, RR.resample_pass(img, out_size, axis)), "the damage must show in the answer"
        return ref
    return RR.resample_pass(img, out_size, axis)


def _build_rh(c, g, dev, B):
    h, w, nw = g["h"], g["w"], g["new_w"]
    img = _rng(c).randint(0, 256, (h, w, 3)).astype(np.uint8)
    tables = _tables(w, nw, c["data"] == "damaged")
    B.put("src", img)
    B.put("bounds", tables[0])
    B.put("kk", tables[1])
    B.out("dst", np.uint8, (h, nw, 3))
    B.regard = "src" if c["data"] == "damaged" else None

    def check(got):
        assert tables[2] == ic.ksize_of(w, nw)
        _eq(got["dst"], _pass_ref(c, img, nw, 1, tables), c["id"])
    return check


def _build_rv(c, g, dev, B):
    e = c["entry"]
    h, nh, nw = g["h"], g["new_h"], g["new_w"]
    img = _rng(c).randint(0, 256, (h, nw, 3)).astype(np.uint8)
    tables = _tables(h, nh, c["data"] == "damaged")
    B.put("src", img, guard=1024)                          # a damaged lo is at most 6 rows of 3 * new_w <= 24 bytes away
    B.put("bounds", tables[0])
    B.put("kk", tables[1])
    B.regard = "src" if c["data"] == "damaged" else None
    if e == ic.RV:
        B.out("dst", np.uint8, (nh, nw, 3))
    else:
        B.out("dst", F, (3, g["hp"], g["wp"]))
    src, bounds, kk = B.ins["src"], B.ins["bounds"], B.ins["kk"]
    use = bool(g["tables"])
    ks = tables[2] if use else 0
    mean, std = (ctypes.c_float * 3)(*ic.MEAN), (ctypes.c_float * 3)(*ic.STD)

    def resized():
        return _pass_ref(c, img, nh, 0, tables) if use else img

    def check(got):
        assert c["data"] != "damaged" or 6 * 3 * nw < 256
        v = resized()
        assert v.shape == (nh, nw, 3)
        if e == ic.RV:
            return _eq(got["dst"], v, c["id"])
        if e == ic.RVF:
            v = v[:, ::-1]
        chw = v.transpose(2, 0, 1)
        if g["reverse"]:
            chw = chw[::-1]
        ref = np.zeros((3, g["hp"], g["wp"]), dtype=F)
        ref[:, :nh, :nw] = (chw.astype(F) - np.array(ic.MEAN, dtype=F)[:, None, None]) / np.array(ic.STD, dtype=F)[:, None, None]      # one rounded fp32 operation per step
        assert ref.dtype == F
        _eq(got["dst"], ref, c["id"])

    def extra(lib, stream, first):
        """Either form == cmk_preprocess_chw fed the cmk_resize_v_u8 output; the hflip form == the plain entry on the column-mirrored source."""
        t = lambda use_, b: b.ptr() if use_ else None
        u8 = torch.empty((nh, nw, 3), dtype=torch.uint8, device=dev)
        assert lib.cmk_resize_v_u8(src.ptr(), h, nh, nw, t(use, bounds), t(use, kk), ks, u8.data_ptr(), stream) == 0
        x = u8.flip(1) if e == ic.RVF else u8
        x = x.permute(2, 0, 1)
        x = (x.flip(0) if g["reverse"] else x).contiguous()
        dst = torch.full((3, g["hp"], g["wp"]), float("nan"), device=dev)
        assert lib.cmk_preprocess_chw(x.data_ptr(), 1, dst.data_ptr(), nh, nw, g["hp"], g["wp"], mean, std, stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst.view(torch.int32), first["dst"].view(torch.uint8).view(torch.int32).view(dst.shape)), c["id"] + ": not the bits of cmk_preprocess_chw on the cmk_resize_v_u8 output"
        if e == ic.RVF:
            mirrored = torch.from_numpy(img[:, ::-1].copy()).to(dev)
            dst.fill_(float("nan"))
            assert lib.cmk_resize_v_preprocess(mirrored.data_ptr(), h, nh, nw, t(use, bounds), t(use, kk), ks, dst.data_ptr(), g["hp"], g["wp"], mean, std,
                                               g["reverse"], stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(dst.view(torch.int32), first["dst"].view(torch.uint8).view(torch.int32).view(dst.shape)), c["id"] + ": not the bits of the plain entry on the mirrored source"
    if e != ic.RV:
        B.extra = extra
    return check


# ---------------------------------------------------------------------------------------------------------------
# test-time augmentation
# ---------------------------------------------------------------------------------------------------------------
def _augs(g, h, w):
    scales = (0.75, 1.0, 1.5, 1.25, 0.6)
    return [(max(1, int(round(h * scales[i % 5]))), max(1, int(round(w * scales[i % 5]))), bool(g["flips"][i])) for i in range(g["a"])]


def _table(augs, h, w, to_image):
    rows = []
    for aug in augs:
        rx, ry = TR.ratios(aug, h, w, to_image)
        rows.append([aug[1], aug[0], rx, ry, 1.0 if aug[2] else 0.0])
    return np.array(rows, dtype=F)


def _boxes(rng, n, w, h, wild=False):
    """n boxes inside (0, w) x (0, h); wild: reaching past both edges on both axes."""
    x0, y0 = rng.uniform(0, 0.7 * w, n), rng.uniform(0, 0.7 * h, n)
    b = np.stack([x0, y0, x0 + rng.uniform(1, 0.3 * w, n), y0 + rng.uniform(1, 0.3 * h, n)], axis=1)
    if wild:
        b[0::3] = np.stack([rng.uniform(-80, -1, n), rng.uniform(-80, -1, n), w + rng.uniform(1, 90, n), h + rng.uniform(1, 90, n)], axis=1)[0::3]
        b[1::3, 0] -= w
        b[1::3, 3] += h
    return b.astype(F)


def _build_timg(c, g, dev, B):
    a, k, h, w = g["a"], g["k"], g["img_h"], g["img_w"]
    rng = _rng(c)
    augs = _augs(g, h, w)
    box, score, loc = np.full((a, k, 4), np.nan, dtype=F), np.full((a, k), np.nan, dtype=F), np.full((a, k, 2), np.nan, dtype=F)
    cls = np.full((a, k), 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    clamped = [min(max(v, 0), k) for v in g["counts"]]
    for i, (nh, nw, _) in enumerate(augs):
        n = clamped[i]
        box[i, :n] = _boxes(rng, n, nw, nh, wild=c["data"] == "clip")
        score[i, :n], loc[i, :n], cls[i, :n] = rng.rand(n), rng.uniform(0, nw, (n, 2)), rng.randint(0, 80, n)
    if c["data"] == "nonfinite":
        box[0, 0], box[0, 1], box[1, 2], box[1, 3] = (np.nan, 10, 50, np.inf), (-np.inf, np.nan, 30, 40), (np.inf, -np.inf, np.nan, 7), (5, 6, np.inf, np.nan)
        loc[0, 3, 0], loc[1, 4], score[1, 1], score[0, 2] = np.nan, (np.inf, np.nan), np.nan, np.inf
    for name, t in (("det_box", box), ("det_score", score), ("det_cls", cls), ("det_loc", loc), ("det_counts", np.array(g["counts"], dtype=np.int32)),
                    ("table", _table(augs, h, w, True))):
        B.put(name, t)
    cap = a * k
    B.out("cand_box", F, (cap, 4))
    B.out("cand_score", F, (cap,))
    B.out("cand_cls", np.int32, (cap,))
    B.out("cand_loc", F, (cap, 2))
    B.out("cand_count", np.int32, (1,))

    def check(got):
        what = c["id"]
        ref = TR.boxes_to_image(box, score, cls, loc, g["counts"], augs, h, w)
        m = sum(clamped)
        assert ref["box"].shape == (m, 4) and int(got["cand_count"][0]) == m, (what, int(got["cand_count"][0]), m)
        if c["data"] == "clip":
            assert (ref["box"][:, 0] == 0).any() and (ref["box"][:, 2] == w).any() and (ref["box"][:, 1] == 0).any() and (ref["box"][:, 3] == h).any()
            assert ((ref["box"][:, 0] == 0) & (ref["box"][:, 2] == w)).any(), what + ": a box must clip at both edges"
        if c["data"] == "nonfinite":
            assert not np.isnan(ref["box"]).any() and np.isnan(ref["loc"]).sum() == 2 and np.isnan(ref["score"]).sum() == 1, what + ": fmin / fmax drop the NaN of a box"
        for name, key in (("cand_box", "box"), ("cand_score", "score"), ("cand_cls", "cls"), ("cand_loc", "loc")):
            _eq(got[name][:m], ref[key].astype(got[name].dtype), what + " " + name)
            assert C.is_filler(got[name][m:]), what + ": {} written past the compacted total".format(name)
    return check


def _build_taug(c, g, dev, B):
    a, k, h, w = g["a"], g["k"], 480, 640
    rng = _rng(c)
    augs = _augs(g, h, w)
    n = min(max(g["count"], 0), k)
    box = np.full((k, 4), np.nan, dtype=F)
    box[:n] = _boxes(rng, n, w, h)
    if c["data"] == "nonfinite":
        box[0], box[1], box[2] = (np.nan, 1, np.inf, 4), (-np.inf, np.inf, 3, np.nan), (1, 2, np.nan, -np.inf)
    B.put("box", box)
    B.put("count", np.array([g["count"]], dtype=np.int32))
    B.put("table", _table(augs, h, w, False))
    B.out("out_box", F, (a, k, 4))
    B.out("out_counts", np.int32, (a,))

    def check(got):
        ref = TR.boxes_to_aug(box, g["count"], augs, h, w)
        if c["data"] == "nonfinite":
            assert np.isnan(ref).any() and np.isinf(ref).any()
        _eq(got["out_box"], ref, c["id"])
        assert (ref[:, n:] == 0).all() and got["out_counts"].tolist() == [n] * a, (c["id"], got["out_counts"].tolist(), n)
    return check


def _build_tred(c, g, dev, B):
    a, k, s = g["a"], g["k"], g["s"]
    rng = np.random.RandomState(100000 * a + 1000 * k + s)           # by geometry: the unaligned rows get the data of the aligned census row
    masks = rng.rand(a, k, s, s).astype(F)
    scores = rng.rand(a, k).astype(F)
    n = min(max(g["count"], 0), k)
    masks[:, n:] = np.nan
    scores[:, n:] = np.nan
    if c["data"] == "nonfinite":
        masks[0, 0, 1, 2], masks[a - 1, 1, 0, s - 1], scores[0, 2] = np.nan, np.inf, np.nan
    B.put("masks", masks, off=g["masks_off"])
    B.put("flips", np.array(g["flips"], dtype=np.int32))
    B.put("mask_scores", scores)
    B.put("count", np.array([g["count"]], dtype=np.int32))
    B.out("out_masks", F, (k, s, s), off=g["out_off"])
    B.out("out_scores", F, (k,))

    def check(got):
        what = c["id"]
        ref_m, ref_s = TR.reduce_masks(masks, g["flips"], scores if g["scores"] else None, g["count"])
        if c["data"] == "nonfinite":
            x = s - 1 - 2 if g["flips"][0] else 2
            assert np.argwhere(np.isnan(ref_m)).tolist() == [[0, 1, x]], what + ": the NaN stays in its own pixel, mirrored under flip"
            assert np.isinf(ref_m).sum() == 1 and np.isnan(ref_s).tolist() == [False, False, True]
        assert not np.isnan(ref_m[n:]).any()
        _eq(got["out_masks"], ref_m, what)
        if g["scores"]:
            _eq(got["out_scores"], ref_s, what + " scores")
        else:
            assert C.is_filler(got["out_scores"]), what + ": out_scores was not handed in"
        key = (a, k, s, g["count"], tuple(g["flips"]), g["scores"], c["data"])
        bits = got["out_masks"].view(np.uint32)
        assert np.array_equal(_SEEN.setdefault(key, bits), bits), what + ": other bits than the first row on the same data gave"
    return check


# ---------------------------------------------------------------------------------------------------------------
# RLE, packed masks
# ---------------------------------------------------------------------------------------------------------------
def _runs(m):
    """COCO run lengths of a bitmap: column-major, zeros first."""
    flat = np.asarray(m, dtype=np.int8).reshape(-1, order="F")
    edges = np.concatenate(([0], np.flatnonzero(np.diff(flat)) + 1, [flat.size]))
    return ([0] if flat[0] else []) + np.diff(edges).tolist()


def _random_masks(rng, r, h, w):
    p = rng.rand(r, 1, 1)
    p[0], p[min(1, r - 1)] = 1.0, 0.0 if r > 1 else 1.0          # a full and an empty mask among them
    return (rng.rand(r, h, w) < p).astype(np.uint8)


def _build_rle(c, g, dev, B):
    r, h, w = g["r"], g["h"], g["w"]
    rng = _rng(c)
    known = {}
    if c["data"] == "long":
        a = LONG_HEAD + [h * w - sum(LONG_HEAD)]
        b = LONG_HEAD[1:] + [h * w - sum(LONG_HEAD[1:])]
        masks = np.stack([mask_from_counts(a, h, w), mask_from_counts(b, h, w)])
        known = {0: a, 1: b}
    elif c["data"] == "random":
        masks = _random_masks(rng, r, h, w)
    else:
        masks = rle_mask_set(h, w, seed=h * 1000 + w)
        known = {0: [h * w], 1: [0, h * w], 5: [0] + [1] * (h * w)}
    assert masks.shape == (r, h, w) and masks.dtype == np.uint8 and masks.max() <= 1
    runs = [_runs(m) for m in masks]
    for i, want in known.items():
        assert runs[i] == want, (c["id"], i, "the run lengths are known by construction")
    if "2145" in c["why"]:
        assert len(runs[4]) == 2145 and len(runs[5]) == 2146
    if c["data"] == "long":
        assert max(len(wire.rle_to_string([v])) for v in runs[0]) == 5 and len(wire.rle_to_string(runs[0])) == 53
    n_runs = np.array([len(x) for x in runs], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(n_runs)))
    total = int(off[-1])
    B.put("masks", masks, off=g["off"])
    B.out("ws", np.uint8, (ic.rle_ws_bytes(r, h, w),))
    B.out("n_runs", np.int32, (r,))
    B.out("starts", np.int32, (total,))
    B.out("counts", np.int32, (total,))
    B.out("bytes", np.uint8, (7 * total,))
    B.out("lens", np.int64, (r,))
    if c["answer"] == "accept" and c["kernels"]:
        B.steps = [dict(c, phase="count"), dict(c, phase="encode")]

    def between(got):
        """After the count phase: the encode phase sizes its stores by these numbers, so it runs only if they are the reference's."""
        assert got["n_runs"].tolist() == n_runs.tolist(), c["id"] + ": n_runs"
        assert got["ws"][:8 * (r + 1)].view(np.int64).tolist() == off.tolist(), c["id"] + ": the run offsets in the workspace"
        for name in ("starts", "counts", "bytes", "lens"):
            assert C.is_filler(got[name]), (c["id"], name, "written by the count phase")
    B.between = between

    def check(got):
        what = c["id"]
        assert got["counts"].tolist() == [v for x in runs for v in x], what + ": run lengths"
        text = got["bytes"].tobytes()
        for i, x in enumerate(runs):
            want = wire.rle_to_string(x)
            assert int(got["lens"][i]) == len(want), (what, i, int(got["lens"][i]), len(want))
            assert text[7 * off[i]:7 * off[i] + len(want)].decode("latin-1") == want, (what, i, "the string")
    return check


def _build_pack(c, g, dev, B):
    r, h, w = g["r"], g["h"], g["w"]
    masks = _random_masks(_rng(c), r, h, w)
    nw = ic.nwords(h, w)
    if c["entry"] == ic.PACK:
        B.put("masks", masks, off=g["off"])
        B.out("words", np.uint64, (r, nw))
        B.out("areas", np.int32, (r,))
    else:
        B.put("words", BR.packed(masks))
        B.out("masks", np.uint8, (r, h, w), off=g["off"])

    def check(got):
        if c["entry"] == ic.PACK:
            _eq(got["words"], BR.packed(masks), c["id"])
            assert got["areas"].tolist() == masks.reshape(r, -1).sum(1).tolist(), c["id"] + ": areas"
        else:
            _eq(got["masks"], masks, c["id"])
    return check


def _with_zero_runs(rng, runs):
    """The same mask with zero-length runs put into the middle of its list: a run x becomes a, 0, x - a (and once a, 0, 0, 0, x - a)."""
    out = []
    for i, x in enumerate(runs):
        if rng.rand() < 0.5 or i in (0, len(runs) - 1):
            cut = int(rng.randint(0, x + 1))
            out += [cut, 0, 0, 0, x - cut] if i % 4 == 1 else [cut, 0, x - cut]
        else:
            out.append(x)
    return out


def _build_dec(c, g, dev, B):
    m, h, w = g["m"], g["h"], g["w"]
    hw = h * w
    rng = _rng(c)
    if c["data"] == "middle":
        lists = [[3, 0, 2, 0, 0, 5, 55], [0, 0, 0, hw], [hw, 0, 0]]
    else:
        rand = [_runs(x) for x in (rng.rand(2, h, w) < 0.4).astype(np.uint8)]
        lists = [[hw], [0, hw], [0] + [1] * hw, _with_zero_runs(rng, rand[0]), rand[1]]      # one run; a zero-length first run; H*W + 1 runs; zeros in the middle
    assert len(lists) == m and all(sum(x) == hw for x in lists)
    masks = np.stack([mask_from_counts(x, h, w) for x in lists])
    if c["data"] != "middle":
        assert 0 in lists[3][1:-1] and np.array_equal(masks[3], mask_from_counts(rand[0], h, w)), "a zero-length run in the middle changes nothing"
    B.put("cum", np.concatenate([np.cumsum(x) for x in lists]).astype(np.int32))
    B.put("off", np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64))
    B.out("words", np.uint64, (m, ic.nwords(h, w)))
    B.out("areas", np.int32, (m,))
    B.out("bitmasks", np.uint8, (m, h, w), off=g["off"])

    def check(got):
        _eq(got["words"], BR.packed(masks), c["id"])
        assert got["areas"].tolist() == masks.reshape(m, -1).sum(1).tolist(), c["id"] + ": areas"
        if g["bitmasks"]:
            _eq(got["bitmasks"], masks, c["id"] + " bitmasks")
        else:
            assert C.is_filler(got["bitmasks"]), c["id"] + ": bitmasks was not handed in"
    return check


def _build_inter(c, g, dev, B):
    n, m, h, w = g["n"], g["m"], g["h"], g["w"]
    rng = _rng(c)
    det, gt = _random_masks(rng, n, h, w), _random_masks(rng, m, h, w)
    B.put("det", BR.packed(det))
    B.put("gt", BR.packed(gt))
    B.out("inter", np.int32, (n, m))                      # pre-filled with filler: the entry zeroes it

    def check(got):
        ref = det.reshape(n, -1).astype(np.int64) @ gt.reshape(m, -1).astype(np.int64).T
        assert ref.max() > 0
        _eq(got["inter"], ref.astype(np.int32), c["id"])
    return check


def _solid(rng, h, w, d, r):
    """Masks that survive a (2d+1)-square: the full mask; a rectangle over every row cut by the left edge; one cut by the bottom and right
    edges and two overlapping ones inside, each with a few pixels knocked out."""
    side = 2 * d + 1
    out = [np.ones((h, w), dtype=np.uint8)]
    out.append(BR.rect(h, w, 0, h, 0, min(w, side + max(1, (w - side) // 2))))
    m = BR.rect(h, w, h - min(h, side + (h - side + 1) // 2), h, w - min(w, side + (w - side + 1) // 2), w)
    out.append(m)
    out.append(np.maximum(BR.rect(h, w, 1, min(h - 1, side + 2), 1, min(w - 1, side + 3)), BR.rect(h, w, max(1, h - side - 4), h - 1, max(1, w - side - 9), w - 1)))
    for m in out[2:]:
        ys, xs = np.nonzero(m)
        pick = rng.choice(len(ys), 4, replace=False)
        m[ys[pick], xs[pick]] = 0
    return np.stack([out[i % 4] for i in range(r)])


def _build_bnd(c, g, dev, B):
    r, h, w, d = g["r"], g["h"], g["w"], g["d"]
    masks = _solid(_rng(c), h, w, d, r) if c["data"].startswith("solid") else BR.mask_set(h, w, seed=h * 1000 + w)
    assert masks.shape == (r, h, w)
    nw = ic.nwords(h, w)
    B.put("words", BR.packed(masks))
    B.out("bwords", np.uint64, (r, nw))
    B.out("bareas", np.int32, (r,))
    ref = {}
    if c["answer"] == "accept" and c["kernels"]:
        # before the launch, on the reference alone: the row must not be one whose every answer is "the boundary is the mask"
        ref["b"] = BR.boundary_ref(masks, d)
        area, barea = masks.reshape(r, -1).sum(1), ref["b"].reshape(r, -1).sum(1)
        partly = int(((barea > 0) & (barea < area)).sum())
        if ic.geometry(c)["fits"]:
            need = 1 if (h, w, d) == (131, 131, 65) else 2      # a 131-pixel square on 131 x 131: only the full mask survives, by one pixel
            assert partly >= need, (c["id"], "masks with 0 < boundary area < mask area", partly)
        else:
            assert np.array_equal(ref["b"], masks.astype(bool))

    def check(got):
        _eq(got["bwords"], BR.packed(ref["b"].astype(np.uint8)), c["id"])
        assert got["bareas"].tolist() == ref["b"].reshape(r, -1).sum(1).tolist(), c["id"] + ": areas"
    return check


BUILD = {ic.RH: _build_rh, ic.RV: _build_rv, ic.RVP: _build_rv, ic.RVF: _build_rv, ic.TIMG: _build_timg, ic.TAUG: _build_taug, ic.TRED: _build_tred,
         ic.RLE: _build_rle, ic.PACK: _build_pack, ic.UNPACK: _build_pack, ic.DEC: _build_dec, ic.INTER: _build_inter, ic.BND: _build_bnd}


def _conform(c, dev, lib):
    B = Bufs(dev)
    check = BUILD[c["entry"]](c, _sane(c), dev, B)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    between, extra = B.between, B.extra
    B.between = between and (lambda got: between(B.host(got)))
    B.extra = extra and (lambda first: extra(lib, stream, first))

    def launch(row):
        rc = ic.call(lib, row, B.p, stream)
        err = lib.cmk_last_error().decode() if rc != 0 else ""
        torch.cuda.synchronize()
        return rc, err
    return C.run_row(c, B, launch, lambda got: check(B.host(got)), einval=ic.CMK_EINVAL, launches=bool(c["kernels"]))


@pytest.mark.parametrize("entry", ic.ENTRIES)
def test_image_conformance(dev, cmk_lib, entry):
    """Every row of one entry.  Everything is exact; nothing to measure.  A row with a count of 0 is accepted and launches nothing: the
    rows are counted by their kernels."""
    C.run_entry(entry, [c for c in CASES if c["entry"] == entry and not c["host_only"]], lambda c: _conform(c, dev, cmk_lib), count="kernels", report=False)
