"""-m gpu: the deformable 3x3 kernel (cmk_deform_conv3x3_nhwc via ops.deform_conv3x3) against the float64 restatement of
tests/deform_ref.py.  Tolerance as test_gpu_backbone_ops: 2e-4 * max(1, max|ref|), never looser than 1e-3 absolute."""
import pytest
import torch

from centermask2_amd import ops
from centermask2_amd.ops import View
from tests.deform_ref import deform_conv3x3_ref

pytestmark = pytest.mark.gpu


def _close(got, ref, rel=2e-4):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    bound = min(1e-3, rel * max(1.0, ref.abs().max().item()))
    assert err <= bound, "max abs err {} > {}".format(err, bound)


def _offsets(kind, n, h, w, dg, modulated, seed):
    g = torch.Generator().manual_seed(seed)
    c = (27 if modulated else 18) * dg
    off = torch.randn((n, c, h, w), generator=g) * 2.0                  # fractional, a few pixels
    o = off[:, :18 * dg]
    if kind == "int":
        o.copy_(torch.randint(-3, 4, o.shape, generator=g).float())
    elif kind == "far":                                                  # a third of the samples far outside the map
        far = torch.rand(o.shape, generator=g) < 0.33
        o[far] = (torch.randint(0, 2, (int(far.sum()),), generator=g).float() * 2 - 1) * (max(h, w) + 5.5)
    elif kind == "edge":                                                 # samples exactly at -1 and at H-1+eps / W-1+eps
        hh = torch.arange(h).view(1, 1, h, 1).float()
        ww = torch.arange(w).view(1, 1, 1, w).float()
        for gi in range(dg):
            for k in range(9):
                i, j = divmod(k, 3)
                dy, dx = off[:, gi * 18 + 2 * k:gi * 18 + 2 * k + 1], off[:, gi * 18 + 2 * k + 1:gi * 18 + 2 * k + 2]
                if k % 2 == 0:
                    dy.copy_((-1.0 - (hh - 1 + i)).expand_as(dy))
                    dx.copy_(((w - 1 + 1e-3) - (ww - 1 + j)).expand_as(dx))
                else:
                    dy.copy_(((h - 1 + 1e-3) - (hh - 1 + i)).expand_as(dy))
                    dx.copy_((-1.0 - (ww - 1 + j)).expand_as(dx) + (k % 3) * 0.37)
    if modulated:                                                        # mask logits: O(1), some at +-large
        m = off[:, 18 * dg:]
        big = torch.rand(m.shape, generator=g)
        m[big < 0.1] = 60.0
        m[big > 0.9] = -60.0
    return off


def _run(x_nchw, off_nchw, weight, scale, shift, dg, modulated, relu=True, x_pad=0, dev="cuda"):
    n, c, h, w = x_nchw.shape
    xt = torch.zeros((n, h, w, c + 2 * x_pad), dtype=torch.float32)
    xt[..., x_pad:x_pad + c] = x_nchw.permute(0, 2, 3, 1)
    x = View(xt.to(dev), x_pad, c)
    off = off_nchw.permute(0, 2, 3, 1).contiguous().to(dev)
    pd = ops.PackedDeformConv(weight, scale, shift, dev)
    y = View(torch.empty((n, h, w, weight.shape[0]), dtype=torch.float32, device=dev))
    ops.deform_conv3x3(x, off, pd, y, dg, modulated, relu=relu)
    torch.cuda.synchronize()
    return y.nchw()


CASES = [
    # N, H, W, Cin, Cout, dg, modulated, offsets
    (2, 13, 21, 128, 128, 1, False, "frac"),
    (1, 17, 23, 160, 160, 2, True, "frac"),
    (1, 11, 19, 224, 224, 4, True, "int"),
    (1, 9, 14, 768, 224, 2, True, "far"),
    (2, 7, 9, 160, 64, 4, False, "edge"),
    (1, 8, 11, 128, 96, 1, True, "edge"),
    (1, 15, 10, 96, 256, 4, True, "frac"),       # Cin/dg = 24; two cout tiles of 128
    (1, 25, 40, 80, 80, 2, True, "frac"),        # V-19-slim stage 3: 40 channels per group
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_deform_conv_matches_float64_restatement(dev, case):
    n, h, w, cin, cout, dg, modulated, kind = case
    g = torch.Generator().manual_seed(100 + CASES.index(case))
    x = torch.randn((n, cin, h, w), generator=g)
    weight = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    scale = torch.rand((cout,), generator=g) + 0.5
    shift = torch.randn((cout,), generator=g) * 0.1
    off = _offsets(kind, n, h, w, dg, modulated, seed=7)
    got = _run(x, off, weight, scale, shift, dg, modulated, x_pad=16 if kind == "frac" else 0)
    ref = deform_conv3x3_ref(x, off, weight, dg, modulated, scale, shift, relu=True)
    _close(got, ref)
    nr = deform_conv3x3_ref(x, off, weight, dg, modulated, scale, shift, relu=False)
    _close(_run(x, off, weight, scale, shift, dg, modulated, relu=False), nr)


@pytest.mark.parametrize("dg,modulated", [(1, False), (2, True), (4, True)])
def test_zero_offsets_unit_mask_equal_plain_conv(dev, dg, modulated):
    """Offsets 0 and mask 1 (logit +60) turn the deformable conv into ops.conv2d of the same weights, up to fp32 rounding."""
    n, h, w, cin, cout = 2, 19, 26, 160, 160
    g = torch.Generator().manual_seed(11)
    x = torch.randn((n, h, w, cin), generator=g).to(dev)
    weight = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    scale, shift = torch.rand((cout,), generator=g) + 0.5, torch.randn((cout,), generator=g) * 0.1
    off = torch.zeros((n, h, w, (27 if modulated else 18) * dg), device=dev)
    off[..., 18 * dg:] = 60.0
    y = View(torch.empty((n, h, w, cout), device=dev))
    ops.deform_conv3x3(View(x), off, ops.PackedDeformConv(weight, scale, shift, dev), y, dg, modulated, relu=True)
    ref = View(torch.empty((n, h, w, cout), device=dev))
    ops.conv2d(View(x), ops.PackedConv(weight, scale, shift, dev), ref, relu=True)
    torch.cuda.synchronize()
    err = (y.t - ref.t).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.t.abs().max().item()), err


def test_writes_only_its_channel_slice(dev):
    """The output slice of a wider (concat) buffer is written; the neighbouring channels stay bit-identical."""
    n, h, w, cin, cout = 1, 12, 17, 128, 96
    g = torch.Generator().manual_seed(5)
    buf = torch.randn((n, h, w, cin + cout + 32), generator=g).to(dev)
    before = buf.clone()
    weight = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    off = _offsets("frac", n, h, w, 2, True, seed=3)
    ops.deform_conv3x3(View(buf, 0, cin), off.permute(0, 2, 3, 1).contiguous().to(dev), ops.PackedDeformConv(weight, None, None, dev),
                       View(buf, cin, cout), 2, True, relu=False)
    torch.cuda.synchronize()
    assert torch.equal(buf[..., :cin], before[..., :cin]) and torch.equal(buf[..., cin + cout:], before[..., cin + cout:])
    ref = deform_conv3x3_ref(before[..., :cin].permute(0, 3, 1, 2).cpu(), off, weight, 2, True)
    _close(buf[..., cin:cin + cout].permute(0, 3, 1, 2), ref)


def test_graph_capture_replay_equals_eager(dev):
    """Offset conv (ops.conv_out) + deformable conv captured in one torch.cuda.graph: no host sync, replay == eager."""
    n, h, w, cin, cout, dg = 2, 20, 30, 128, 128, 2
    g = torch.Generator().manual_seed(9)
    x = torch.randn((n, h, w, cin), generator=g).to(dev)
    off_w = torch.randn((27 * dg, cin, 3, 3), generator=g) * (1.5 / (cin * 9) ** 0.5)
    pc_off = ops.PackedConv(off_w, None, torch.randn(27 * dg, generator=g) * 0.5, dev)
    pd = ops.PackedDeformConv(torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5, None, None, dev)

    def step(y):
        ops.deform_conv3x3(View(x), ops.conv_out(View(x), pc_off).t, pd, y, dg, True, relu=True)

    eager = View(torch.empty((n, h, w, cout), device=dev))
    step(eager)
    torch.cuda.synchronize()
    out = View(torch.zeros((n, h, w, cout), device=dev))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(out)                                                       # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.t, eager.t)
