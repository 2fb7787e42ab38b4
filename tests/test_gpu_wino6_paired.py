"""-m gpu: the paired form of the F(4x4,3x3) Winograd kernel (tune_wm 6 / tune_sc 32, conv_wino6p_kernel: 64 couts per workgroup, halo
loads and pass 1 shared by the two cout tiles) does the arithmetic of conv_wino6_kernel (tune_sc 16) in the same order: every output,
GroupNorm record and split-K partial result must be bit-identical to it."""
import pytest
import torch

from centermask2_amd import _lib, ops
from centermask2_amd.ops import View

from .helpers import raw_conv
from .test_gpu_backbone_ops import WINO6_CASES as MAP_CASES, _rand, _tower_pair

pytestmark = pytest.mark.gpu

# the F(4x4) shapes of test_gpu_backbone_ops.py (test_conv_winograd6_variant: MAP_CASES; test_conv_winograd6_roi_pair_geometry)
ROI_CASES = [(6, 14, 14, 256, 80), (5, 14, 14, 272, 256), (3, 16, 14, 32, 64), (2, 7, 7, 64, 32), (1, 14, 14, 64, 33)]


def _conv(dev, x, wt, tv, seed=0, aff=None):
    """One conv through the C ABI with variant tv (scale, shift and a partial ReLU from seed); returns (rc, output)."""
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    scale = torch.rand(cout, generator=torch.Generator().manual_seed(seed)) + 0.5
    pc = ops.PackedConv(wt, scale, _rand((cout,), seed + 1, 0.1), dev)
    y = View(torch.full((n, h, w, cout), -5.0, device=dev))
    return raw_conv(ops.as_view(x.to(dev)), pc, y, tv, relu_upto=cout // 2, in_affine=aff)[0], y.t


def _same(dev, x, wt, tv16, tv32, seed=0, aff=None):
    rc16, y16 = _conv(dev, x, wt, tv16, seed, aff)
    rc32, y32 = _conv(dev, x, wt, tv32, seed, aff)
    assert rc16 == 0 and rc32 == 0, _lib.load().cmk_last_error()
    assert torch.equal(y16, y32), "paired form differs from conv_wino6: max |d| {}".format(float((y16 - y32).abs().max()))


@pytest.mark.parametrize("case", MAP_CASES)
def test_paired_map_tiles_equal_wino6(dev, case):
    n, h, w, cin, cout = case
    _same(dev, _rand((n, cin, h, w), 81), _rand((cout, cin, 3, 3), 82, (2.0 / (cin * 9)) ** 0.5), (6, 16, 1), (6, 32, 1), 83)


@pytest.mark.parametrize("case", ROI_CASES)
def test_paired_roi_pairs_equal_wino6(dev, case):
    n, h, w, cin, cout = case
    _same(dev, _rand((n, cin, h, w), 91), _rand((cout, cin, 3, 3), 92, (2.0 / (cin * 9)) ** 0.5), (6, 16, 2), (6, 32, 2), 93)


@pytest.mark.parametrize("cout", [160, 224, 80, 5])
@pytest.mark.parametrize("geo", [1, 2])
def test_paired_odd_cout_tiles(dev, cout, geo):
    """An odd number of 32-cout tiles: the upper half of the last workgroup has no tile of its own and must store nothing."""
    n, h, w, cin = (2, 25, 41, 64) if geo == 1 else (3, 14, 14, 64)
    _same(dev, _rand((n, cin, h, w), 11), _rand((cout, cin, 3, 3), 12, 0.05), (6, 16, geo), (6, 32, geo), 13)


@pytest.mark.parametrize("geo", [1, 2])
def test_paired_fused_input_affine(dev, geo):
    n, h, w, cin, cout = (2, 25, 40, 256, 96) if geo == 1 else (4, 14, 14, 256, 96)
    aff = ((torch.rand((n, cin), generator=torch.Generator().manual_seed(21)) + 0.5).to(dev), _rand((n, cin), 22, 0.5).to(dev))
    _same(dev, _rand((n, cin, h, w), 23) + 0.3, _rand((cout, cin, 3, 3), 24, 0.03), (6, 16, geo), (6, 32, geo), 25, aff)


def test_paired_channel_views(dev):
    """Reading a channel slice of a wider buffer and writing into a slice of another: the same bits, neighbours untouched."""
    n, h, w, cin, cout = 2, 23, 47, 64, 48
    big = _rand((n, h, w, 160), 5).to(dev)
    pc = ops.PackedConv(_rand((cout, cin, 3, 3), 6, 0.06), None, _rand((cout,), 8, 0.1), dev)
    outs = []
    for sc in (16, 32):
        out = torch.full((n, h, w, 96), -7.0, device=dev)
        _lib.check(raw_conv(View(big, 32, cin), pc, View(out, 16, cout), (6, sc, 1), relu_upto=4)[0], "wino6 views")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert float(outs[1][..., :16].max()) == -7.0 and float(outs[1][..., 64:].min()) == -7.0


@pytest.mark.parametrize("cout,groups", [(256, 32), (96, 3), (80, 5)])
@pytest.mark.parametrize("with_affine", [False, True])
def test_paired_groupnorm_records(dev, cout, groups, with_affine):
    """The fused GroupNorm {sum, sumsq} records of a multi-problem launch (FCOS tower levels), with and without the fused input affine:
    every record and every output bit as conv_wino6 writes them."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(31)
    shapes = [(2, 25, 41), (2, 13, 20), (2, 7, 10), (2, 4, 5), (2, 2, 3)]
    cin = 256
    pc = ops.PackedConv(torch.randn((cout, cin, 3, 3), generator=g) * 0.03, None, torch.randn((cout,), generator=g) * 0.1, dev)
    xs = [ops.as_view(torch.randn((n, cin, h, w), generator=g).to(dev)) for n, h, w in shapes]
    affs = [((torch.rand((n, cin), generator=g) + 0.5).to(dev), (torch.randn((n, cin), generator=g) * 0.3).to(dev)) for n, _, _ in shapes]
    recs = sum(n * lib.cmk_conv_gn_records(h, w, 6) for n, h, w in shapes)
    res = []
    for sc in (16, 32):
        ys = [View(torch.full((n, h, w, cout), -5.0, device=dev)) for n, h, w in shapes]
        gws = torch.full((recs, groups, 2), -1.0, dtype=torch.float64, device=dev)
        _lib.check(raw_conv(xs, [pc] * len(shapes), ys, (6, sc, 1), in_affine=affs if with_affine else None, gn=(gws, groups))[0], "wino6 gn records")
        res.append((ys, gws))
    for y16, y32 in zip(res[0][0], res[1][0]):
        assert torch.equal(y16.t, y32.t)
    assert torch.equal(res[0][1], res[1][1]), "GroupNorm records differ"


@pytest.mark.parametrize("case", [(2, 25, 40, 768, 224, 4), (1, 50, 80, 512, 192, 2), (2, 13, 41, 64, 33, 2), (1, 12, 40, 128, 256, 8)])
def test_paired_split_k(dev, case):
    n, h, w, cin, cout, sk = case
    _same(dev, _rand((n, cin, h, w), 181), _rand((cout, cin, 3, 3), 182, (2.0 / (cin * 9)) ** 0.5), (6, 16, 1, sk), (6, 32, 1, sk), 183)
    rc, _ = _conv(dev, _rand((1, 48, 12, 40), 185), _rand((32, 48, 3, 3), 186, 0.05), (6, 32, 1, 4))      # 6 chunks % 8 != 0
    assert rc != 0


@pytest.mark.parametrize("with_affine", [False, True])
def test_paired_tower_pair_launch(dev, with_affine, monkeypatch):
    """ops.conv_gn_multi_pair (the cls and bbox towers' conv k as ONE launch of 10 problems with per-problem weights) on the paired form:
    outputs and GroupNorm affines bit-identical to the same launch on conv_wino6."""
    groups = 32
    pca, pcb, gn, xs, aff_a, aff_b = _tower_pair(dev, [(2, 25, 41), (2, 13, 20), (2, 7, 10), (2, 4, 5), (2, 2, 3)], 256, with_affine)
    res = []
    for sc in (16, 32):
        monkeypatch.setattr(ops, "FORCE_VARIANT", (6, sc, 1))
        pair = ops.conv_gn_multi_pair(xs, pca, gn[0], xs, pcb, gn[1], groups, 1e-5, in_affine_a=aff_a, in_affine_b=aff_b)
        assert pair is not None
        torch.cuda.synchronize()
        res.append(pair)
    for (ys, affs), (ys_ref, affs_ref) in zip(res[1], res[0]):
        for y, yr, (sc_, sh_), (scr, shr) in zip(ys, ys_ref, affs, affs_ref):
            assert torch.equal(y.t, yr.t) and torch.equal(sc_, scr) and torch.equal(sh_, shr)
