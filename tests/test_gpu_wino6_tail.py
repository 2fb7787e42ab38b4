"""-m gpu: tail split-K of the RoI-pair F(4x4,3x3) Winograd launches (tune_wm 6 / tune_wn 2, cmk.h splitk_tail): the last spatial tiles
of a launch run as several short workgroups per (tile, cout tile) that share the chunk loop and leave raw partial sums for a reduce
launch over the tail's images.  The tail is forced with splitk_tail_tiles (ops.TAIL_TILES), so the device's CU count plays no part.

Harness, data and tolerance are those of test_gpu_backbone_ops.test_conv_winograd6_split_k (unit-variance input, He weights, scale in
[0.5, 1.5), ReLU; 2e-4 * max(1, max|ref|), never looser than 1e-3); the reference is torch's conv2d on the CPU, here evaluated in
float64.  Images outside the tail must carry the bits of the same launch without a tail."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from centermask2_amd import _lib, ops
from centermask2_amd.ops import View
from tests.helpers import raw_conv, relaunch
from tests.test_gpu_backbone_ops import _close, _rand, _run_variant

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout, tail tiles, ways)
CASES = [
    pytest.param((7, 14, 14, 64, 40, 1, 2), id="odd-batch-cout40"),         # the last pair's second image is empty, and it sits in the tail; 2 cout tiles, the second ragged
    pytest.param((8, 14, 14, 64, 64, 1, 4), id="n8-tail1"),
    pytest.param((8, 14, 14, 64, 64, 2, 2), id="n8-tail2"),
    pytest.param((8, 14, 14, 64, 64, 4, 4), id="n8-tail-all"),
    pytest.param((6, 14, 14, 48, 40, 2, 2), id="cin48-pieces-1+2"),         # 3 chunk pairs in 2 ways
    pytest.param((4, 14, 14, 272, 64, 1, 4), id="cin272-ways4"),            # 17 chunk pairs
    pytest.param((3, 14, 14, 272, 40, 1, 8), id="cin272-ways8"),
    pytest.param((5, 16, 14, 64, 64, 2, 2), id="map16x14"),
]


def _problem(case):
    n, h, w, cin, cout = case[:5]
    x = _rand((n, cin, h, w), 181)
    wt = _rand((cout, cin, 3, 3), 182, (2.0 / (cin * 9)) ** 0.5)
    scale = torch.rand(cout, generator=torch.Generator().manual_seed(183)) + 0.5
    shift = _rand((cout,), 184, 0.1)
    ref = F.relu(F.conv2d(x.double(), wt.double(), None, padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    return x, wt, scale, shift, ref.float()


def _run(dev, monkeypatch, prob, tv, tail_tiles=0):
    monkeypatch.setattr(ops, "TAIL_TILES", tail_tiles)
    x, wt, scale, shift, _ = prob
    rc, y = _run_variant(dev, x, wt, scale, shift, tv)
    assert rc == 0, _lib.load().cmk_last_error()
    return y


@pytest.mark.parametrize("case", CASES)
def test_tail_split_k(dev, case, monkeypatch):
    n, h, w, cin, cout, tiles, ways = case
    prob = _problem(case)
    ref = prob[4]
    first_tail = 2 * ((n + 1) // 2 - tiles)          # the first image of the tail
    ys = {}
    for sc in (16, 32):
        off = _run(dev, monkeypatch, prob, (6, sc, 2))
        on = _run(dev, monkeypatch, prob, (6, sc, 2, 1, ways), tiles)
        assert torch.equal(on.t[:first_tail], off.t[:first_tail]), "images outside the tail changed"
        _close(on.nchw()[first_tail:], ref[first_tail:])
        _close(on.nchw(), ref)                                          # (and nothing was left unwritten)
        again = _run(dev, monkeypatch, prob, (6, sc, 2, 1, ways), tiles)
        assert torch.equal(on.t, again.t), "two runs differ"
        ys[sc] = on
    assert torch.equal(ys[16].t, ys[32].t), "the paired form's tail differs from conv_wino6's"


@pytest.mark.parametrize("case", [(8, 14, 14, 64, 64, 4), (5, 14, 14, 272, 40, 8), (6, 14, 14, 48, 40, 2)])
@pytest.mark.parametrize("sc", [16, 32])
def test_tail_of_every_tile_is_split_k(dev, case, sc, monkeypatch):
    """splitk = ways on the RoI-pair geometry (accepted now, also where the chunks do not split evenly) is the tail that takes every
    tile: the same bits."""
    n, h, w, cin, cout, ways = case
    prob = _problem(case)
    sk = _run(dev, monkeypatch, prob, (6, sc, 2, ways))
    tail = _run(dev, monkeypatch, prob, (6, sc, 2, 1, ways), (n + 1) // 2)
    _close(sk.nchw(), prob[4])
    assert torch.equal(sk.t, tail.t)
    more = _run(dev, monkeypatch, prob, (6, sc, 2, 1, ways), n)           # a tile count past the launch's is capped
    assert torch.equal(sk.t, more.t)


@pytest.mark.parametrize("sc", [16, 32])
def test_tail_channel_view(dev, sc, monkeypatch):
    """The mask head's first conv reads 256 of the 272 channels of the MaskIoU input buffer (x_cs 272) and the output goes into a channel
    slice; neighbours stay untouched, images outside the tail keep their bits."""
    monkeypatch.setattr(ops, "TAIL_TILES", 1)
    n, h, w, cin, cout = 5, 14, 14, 256, 40
    big = _rand((n, h, w, 272), 5).to(dev)
    wt = _rand((cout, cin, 3, 3), 6, (2.0 / (cin * 9)) ** 0.5)
    pc = ops.PackedConv(wt, None, _rand((cout,), 8, 0.1), dev)
    outs = []
    for tv in ((6, sc, 2), (6, sc, 2, 1, 4)):
        out = torch.full((n, h, w, 96), -7.0, device=dev)
        rc, d, keep = raw_conv(View(big, 0, cin), pc, View(out, 16, cout), tv, relu_upto=4)
        assert (keep["ws"] is not None) == (len(tv) == 5)
        _lib.check(rc, "wino6 tail views")
        outs.append(out)
    off, on = outs
    ref = F.conv2d(big[..., :cin].permute(0, 3, 1, 2).cpu().double(), wt.double(), pc.shift.cpu().double(), padding=1)
    ref[:, :4] = F.relu(ref[:, :4])
    _close(on[..., 16:56].permute(0, 3, 1, 2), ref.float())
    assert torch.equal(on[:4], off[:4])                                # 3 tiles, the last (image 4 and an empty one) is the tail
    assert float(on[..., :16].max()) == -7.0 and float(on[..., 56:].min()) == -7.0


def test_tail_refusals(dev, cmk_lib, monkeypatch):
    monkeypatch.setattr(ops, "TAIL_TILES", 1)
    n, h, w, cin, cout = 4, 14, 14, 64, 64
    x = ops.as_view(_rand((n, cin, h, w), 1).to(dev))
    pc = ops.PackedConv(_rand((cout, cin, 3, 3), 2, 0.05), None, None, dev)
    ys = [View(torch.empty((n, h, w, cout), device=dev)) for _ in range(3)]
    _, d, keep = raw_conv(x, pc, ys[0], (6, 16, 2, 1, 2), launch=False)
    ws = keep["ws"]
    assert ws is not None and ws.numel() == cmk_lib.cmk_conv_tail_ws_floats(ctypes.byref(d[0])) == 2 * 2 * h * w * 64
    assert relaunch(d) == 0                                             # the descriptor itself is fine
    gws = torch.zeros((64, 32, 2), dtype=torch.float64, device=dev)     # ... but not with fused GroupNorm statistics
    d[0].gn_ws, d[0].gn_groups = gws.data_ptr(), 32
    assert relaunch(d) != 0
    d[0].gn_ws, d[0].gn_groups = None, 0
    d[0].splitk_ws = None                                               # ... nor without its workspace
    assert relaunch(d) != 0 and b"tail" in cmk_lib.cmk_last_error()
    d[0].splitk_ws = ws.data_ptr()
    d[0].splitk_tail = 8                                                # ... nor more ways than chunk pairs (64 channels: 4)
    big = torch.empty((8 * 2 * h * w * 64,), device=dev)
    d[0].splitk_ws = big.data_ptr()
    assert relaunch(d) != 0 and b"tail" in cmk_lib.cmk_last_error()
    d[0].splitk_tail = 2
    d[0].tune_wn = 1                                                    # ... nor on the map geometry
    assert relaunch(d) != 0 and b"tail" in cmk_lib.cmk_last_error()
    d[0].tune_wn, d[0].tune_sc = 2, 64                                  # ... nor on the shared-V form
    assert cmk_lib.cmk_conv_tail_ws_floats(ctypes.byref(d[0])) == 0
    assert relaunch(d) != 0 and b"tail" in cmk_lib.cmk_last_error()
    d[0].tune_sc = 16
    d[0].splitk, d[0].splitk_tail = 2, 2                                # ... nor beside split-K
    assert relaunch(d) != 0 and b"tail" in cmk_lib.cmk_last_error()
    d[0].splitk = 0
    assert relaunch(d) == 0
    # several problems in one launch
    _, d2, keep2 = raw_conv([x, x], [pc, pc], ys[1:], (6, 16, 2, 1, 2), launch=False)
    d2[1].splitk_tail, d2[1].splitk_tail_tiles, d2[1].splitk_ws = 2, 1, keep2["ws"].data_ptr()
    assert relaunch(d2) != 0


def test_tail_off_unless_named(dev, cmk_lib, monkeypatch):
    """A variant without the fifth element, and tail ways 0 / 1, are the launch as it always was: no workspace, the same bits."""
    case = (6, 14, 14, 64, 64)
    prob = _problem(case)
    base = _run(dev, monkeypatch, prob, (6, 16, 2))
    for tv in ((6, 16, 2, 1), (6, 16, 2, 1, 0), (6, 16, 2, 1, 1)):
        assert torch.equal(_run(dev, monkeypatch, prob, tv, 2).t, base.t)
    assert ops._variant_on_menu((6, 16, 2, 1, 8)) and ops._variant_on_menu((6, 32, 2, 1, 2)) and ops._variant_on_menu((6, 16, 2))
    assert not ops._variant_on_menu((6, 64, 2, 1, 2)) and not ops._variant_on_menu((6, 16, 1, 1, 2)) and not ops._variant_on_menu((1, 16, 2, 1, 2))
