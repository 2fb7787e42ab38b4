"""Keypoint heatmap decode without a GPU: the C ABI's argument checks (cmk_keypoint_decode refuses before any launch) and known answers
for the tests' float64 restatement (tests/keypoint_ref.py), plus its resampling matrices against torch's own interpolation."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests import keypoint_ref as KR


def test_keypoint_decode_abi_argument_validation_without_gpu():
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert lib.cmk_keypoint_decode_ws_len(400, 17) == 400 * 17 * 36
    assert lib.cmk_keypoint_decode_ws_len(0, 17) == 0 and lib.cmk_keypoint_decode_ws_len(4, 0) == 0

    def call(dec=p, cs=68, co=0, s=14, k=17, boxes=p, counts=p, n=1, topk=2, ws=p, ws_len=2 * 17 * 36, out=p):
        rc = lib.cmk_keypoint_decode(dec, cs, co, s, k, boxes, counts, n, topk, ws, ws_len, out, None)
        return rc, lib.cmk_last_error()

    for kw in (dict(dec=None), dict(boxes=None), dict(counts=None), dict(ws=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"null" in msg, kw
    for kw, what in ((dict(k=0), b"K = 0"), (dict(s=0), b"resolution 0"), (dict(s=17), b"resolution 17"),
                     (dict(cs=67), b"bad shape"), (dict(co=4, cs=70), b"bad shape"), (dict(n=0), b"bad shape"), (dict(topk=0), b"bad shape"),
                     (dict(ws_len=2 * 17 * 36 - 1), b"workspace"), (dict(k=1 << 21, cs=4 << 21, ws_len=1 << 40), b"too many")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg, (kw, msg)


def test_depth_to_space_layout():
    k, s = 3, 2
    packed = torch.arange(s * s * 4 * k, dtype=torch.float64).reshape(1, s, s, 4 * k)
    m = KR.depth_to_space(packed, k)
    assert tuple(m.shape) == (1, k, 2 * s, 2 * s)
    for a in range(s):
        for b in range(s):
            for py in range(2):
                for px in range(2):
                    for kk in range(k):
                        assert m[0, kk, 2 * a + py, 2 * b + px] == packed[0, a, b, (2 * py + px) * k + kk]


@pytest.mark.parametrize("n_in,n_out", [(56, 1), (56, 3), (56, 34), (56, 56), (56, 111), (56, 1201), (28, 56)])
def test_resampling_matrices_match_torch_interpolate(n_in, n_out):
    """The explicit matrices against F.interpolate in float64 (an independent check of the restatement, not used by it)."""
    g = torch.Generator().manual_seed(n_out)
    x = torch.randn((1, 1, n_in, n_in), generator=g, dtype=torch.float64)
    want = F.interpolate(x, size=(n_out, n_out), mode="bicubic", align_corners=False)[0, 0]
    got = KR.bicubic_matrix(n_in, n_out) @ x[0, 0] @ KR.bicubic_matrix(n_in, n_out).t()
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    if n_out == 2 * n_in:
        want = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)[0, 0]
        assert torch.allclose(KR.heatmaps(x[0, 0]), want, rtol=0, atol=1e-12)


def test_keypoint_ref_known_answers():
    s, k = 14, 2
    # all-zero logits: every pixel is a maximum -> the first one; score 1 / (56 * 56)
    zero = torch.zeros((k, 2 * s, 2 * s))
    box = torch.tensor([10.25, 20.5, 43.65, 38.0])                  # w = 33.4 -> Wc = 34, h = 17.5 -> Hc = 18
    res = KR.decode_one(zero, box)
    for r in res:
        x, y, score = r["xys"]
        assert (r["row"], r["col"]) == (0, 0)
        assert x == pytest.approx(0.5 * float(torch.tensor(33.4, dtype=torch.float32)) / 34 + 10.25, abs=1e-6)
        assert y == pytest.approx(0.5 * 17.5 / 18 + 20.5, abs=1e-9) and score == pytest.approx(1 / 3136, rel=1e-12)
    # a single peak at map28 (a, b) = (5, 9): the bilinear x2 spreads it to the 2x2 block (2a..2a+1, 2b..2b+1) at 0.75^2 of its value;
    # on a 56 x 56 box (scale 1, the bicubic resize is the identity) the first maximum is (2a, 2b)
    peak = torch.zeros((k, 2 * s, 2 * s))
    peak[0, 5, 9] = 4.0
    res = KR.decode_one(peak, torch.tensor([0.0, 0.0, 56.0, 56.0]))
    assert (res[0]["row"], res[0]["col"]) == (10, 18) and res[0]["value"] == pytest.approx(4.0 * 0.5625, abs=1e-12)
    x, y, score = res[0]["xys"]
    assert (x, y) == (18.5, 10.5)
    m56 = KR.heatmaps(peak[0])
    assert score == pytest.approx(1.0 / float(torch.exp(m56 - 2.25).sum()), rel=1e-12) and res[0]["gap"] == 0.0
    # fractional widths: x = (xi + 0.5) * w / ceil(w) + x0
    res = KR.decode_one(peak, torch.tensor([3.3, 4.4, 40.9, 21.65]))
    x0, y0, w, h, wc, hc = KR.box_geometry(torch.tensor([3.3, 4.4, 40.9, 21.65]))
    assert (wc, hc) == (38, 18)
    x, y, _ = res[0]["xys"]
    assert x == pytest.approx((res[0]["col"] + 0.5) * w / wc + x0, abs=1e-12) and KR.pixel_of(x, y, torch.tensor([3.3, 4.4, 40.9, 21.65])) == (res[0]["row"], res[0]["col"])
    # a box under one pixel: w and h clamp to 1 -> a 1 x 1 map, x = x0 + 0.5
    tiny = torch.tensor([7.0, 9.0, 7.4, 9.3])
    res = KR.decode_one(peak, tiny)
    assert res[0]["map"].shape == (1, 1) and res[0]["xys"][:2] == (7.5, 9.5)
    assert math.isinf(res[0]["gap"])
