"""-m gpu: the keypoint heatmap decode (cmk_keypoint_decode via ops.keypoint_decode) against the tests' float64 restatement
(tests/keypoint_ref.py) on seeded packed-deconv maps read through a channel-slice view: boxes under a pixel, fractional, one of
1333 x 800 px and one of 1200 x 1055 px (eight row bands each), a wide flat box (two bands), zero width, padded slots holding NaN boxes.
Comparison rule, per (RoI, keypoint), with m the maximum of the float64 map and eps = 1e-4 max(1, |m|): where m lies more than eps above
every other pixel the kernel's position is that maximum exactly; elsewhere the kernel's pixel lies within eps of m.  Scores within 1e-5
(relative), coordinates within 1e-3 px of the restatement's at the same pixel."""
import pytest
import torch

from centermask2_amd import ops
from centermask2_amd.ops import View
from tests import keypoint_ref as KR

pytestmark = pytest.mark.gpu

K, S = 17, 14
CS, CO = 4 * K + 12, 5                 # the packed output as a channel slice [5, 73) of an 80-channel buffer
COUNTS = [6, 0, 4]
TOPK = 6
NAN = float("nan")


def _boxes():
    b = torch.full((len(COUNTS), TOPK, 4), NAN)
    b[0] = torch.tensor([[10.0, 20.0, 10.4, 20.3],            # under one pixel: a 1 x 1 map
                         [3.3, 4.4, 40.9, 21.65],             # fractional sides
                         [-10.5, 5.25, 1189.5, 1060.5],       # 1200 x 1055.25 px: eight bands
                         [100.0, 100.0, 100.0, 300.0],        # zero width
                         [0.0, 0.0, 56.0, 56.0],              # scale 1
                         [7.7, 8.8, 1307.7, 15.8]])           # 1300 x 7 px: two bands of four and three rows
    b[1] = torch.tensor([[0.0, 0.0, 50.0, 50.0]] * TOPK)     # image without detections: every slot is padding
    b[2, :4] = torch.tensor([[0.0, 0.0, 1333.0, 800.0], [50.0, 60.0, 51.5, 90.25], [5.0, 5.0, 117.0, 229.0], [1.0, 2.0, 3.0, 4.0]])
    return b


def _decode(dec, boxes, counts, dev):
    buf = dec.to(dev).contiguous()
    out = ops.keypoint_decode(View(buf, CO, 4 * K), boxes.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), K)
    torch.cuda.synchronize()
    return out.cpu()


def _check(got, dec, boxes, counts):
    """The comparison rule of the module docstring; returns (positions equal to a unique maximum, all valid positions)."""
    logits = KR.depth_to_space(dec[..., CO:CO + 4 * K].double(), K).reshape(len(counts), TOPK, K, 2 * S, 2 * S)
    exact = total = 0
    for n, cnt in enumerate(counts):
        assert torch.equal(got[n, cnt:], torch.zeros_like(got[n, cnt:])), "slots past counts must be zeros"
        for s in range(cnt):
            ref = KR.decode_one(logits[n, s], boxes[n, s])
            for k, r in enumerate(ref):
                x, y, score = (float(v) for v in got[n, s, k])
                row, col = KR.pixel_of(x, y, boxes[n, s])
                eps = 1e-4 * max(1.0, abs(r["value"]))
                assert 0 <= row < r["map"].shape[0] and 0 <= col < r["map"].shape[1], (n, s, k, row, col)
                if r["gap"] > eps:
                    assert (row, col) == (r["row"], r["col"]), (n, s, k, (row, col), (r["row"], r["col"]), r["gap"])
                    exact += 1
                else:
                    assert float(r["map"][row, col]) >= r["value"] - eps, (n, s, k)
                total += 1
                assert abs(score - r["xys"][2]) <= 1e-5 * r["xys"][2], (n, s, k, score, r["xys"][2])
                if (row, col) == (r["row"], r["col"]):
                    assert abs(x - r["xys"][0]) <= 1e-3 and abs(y - r["xys"][1]) <= 1e-3, (n, s, k, x, y, r["xys"])
    return exact, total


def test_keypoint_decode_matches_float64_restatement(dev):
    g = torch.Generator().manual_seed(11)
    dec = torch.randn((len(COUNTS) * TOPK, S, S, CS), generator=g) * 2.0
    boxes = _boxes()
    got = _decode(dec, boxes, COUNTS, dev)
    exact, total = _check(got, dec, boxes, COUNTS)
    print("keypoint decode: {} of {} positions equal the restatement's unique maximum".format(exact, total))
    assert total == (COUNTS[0] + COUNTS[2]) * K and exact >= total // 2
    assert torch.equal(_decode(dec, boxes, COUNTS, dev), got), "two launches on the same input must agree bit for bit"


def test_keypoint_decode_all_zero_maps_give_the_first_pixel(dev):
    dec = torch.zeros((len(COUNTS) * TOPK, S, S, CS))
    boxes = _boxes()
    got = _decode(dec, boxes, COUNTS, dev)
    for n, cnt in enumerate(COUNTS):
        for s in range(cnt):
            x0, y0, w, h, wc, hc = KR.box_geometry(boxes[n, s])
            assert torch.allclose(got[n, s, :, 0], torch.full((K,), 0.5 * w / wc + x0), rtol=0, atol=1e-4), (n, s)
            assert torch.allclose(got[n, s, :, 1], torch.full((K,), 0.5 * h / hc + y0), rtol=0, atol=1e-4), (n, s)
            assert torch.allclose(got[n, s, :, 2], torch.full((K,), 1.0 / 3136), rtol=1e-6, atol=0), (n, s)


def test_keypoint_decode_replays_in_a_captured_graph(dev):
    """The launch does not depend on the boxes: a graph captured on one set of boxes / counts / maps decodes another set written into
    the same buffers exactly as an eager call does."""
    g = torch.Generator().manual_seed(12)
    dec = torch.randn((len(COUNTS) * TOPK, S, S, CS), generator=g).to(dev)
    boxes = torch.tensor([[[0.0, 0.0, 30.0, 20.0]] * TOPK] * len(COUNTS)).to(dev)
    counts = torch.tensor([1, 1, 1], dtype=torch.int32, device=dev)
    ops.keypoint_decode(View(dec, CO, 4 * K), boxes, counts, K)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.keypoint_decode(View(dec, CO, 4 * K), boxes, counts, K)
    new_dec = torch.randn(dec.shape, generator=g) * 3.0
    new_boxes = _boxes().nan_to_num(0.0)
    dec.copy_(new_dec.to(dev))
    boxes.copy_(new_boxes.to(dev))
    counts.copy_(torch.tensor(COUNTS, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _decode(new_dec, new_boxes, COUNTS, dev))
