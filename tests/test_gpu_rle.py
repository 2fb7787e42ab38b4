"""-m gpu: the device COCO RLE encoder (csrc/rle.hip through ops.mask_rle / wire.rle_encode_batch) against the host codec of wire.py on
the same bitmaps.  Every comparison is exact: strings with ==, counts as lists of ints.  No tolerance anywhere."""
import json

import numpy as np
import pytest
import torch

from centermask2_amd import _lib, ops, wire
from centermask2_amd.structures import Boxes, Instances

pytestmark = pytest.mark.gpu

# the kernel walks 64-row chunks and 256-column tiles (4 columns per lane) and scans 1024 columns at a time: the last shape passes each
# of them by a non-multiple, with an odd W so that every row starts at another alignment
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 65), (64, 64), (257, 130), (97, 131), (131, 1031)]


def mask_from_counts(counts, h, w):
    """The (h,w) bitmask whose column-major runs are `counts` (zeros first): the expected counts are known by construction."""
    flat = np.zeros(h * w, dtype=np.uint8)
    pos, val = 0, 0
    for c in counts:
        flat[pos:pos + c] = val
        pos += c
        val ^= 1
    assert pos == h * w
    return flat.reshape((h, w), order="F")


def mask_set(h, w, seed):
    z, o = np.zeros((h, w), dtype=np.uint8), np.ones((h, w), dtype=np.uint8)
    out = [z.copy(), o.copy()]
    m = z.copy(); m[0, 0] = 1; out.append(m)
    m = z.copy(); m[h - 1, w - 1] = 1; out.append(m)
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(((yy + xx) & 1).astype(np.uint8))                       # checkerboard
    out.append(mask_from_counts([0] + [1] * (h * w), h, w))            # every pixel its own run, h*w + 1 counts
    m = z.copy(); m[:, w // 2] = 1; out.append(m)                      # one full column
    m = z.copy(); m[h // 2, :] = 1; out.append(m)                      # one full row: every run crosses a column boundary
    x = (w - 1) // 2
    pair = z.copy(); pair[h - 1, x] = 1; pair[0, min(x + 1, w - 1)] = 1   # bottom of column x and top of x+1: one run
    out.append(pair)
    out.append(o - pair)
    rng = np.random.RandomState(seed)
    for p in (0.02, 0.5, 0.98):
        out.append((rng.rand(h, w) < p).astype(np.uint8))
    return np.stack(out)


def host_codec(masks_np):
    return [wire.rle_counts(m) for m in masks_np], [wire.rle_encode(m)["counts"] for m in masks_np]


def check_against_host(masks_gpu):
    """ops.mask_rle of bool GPU masks == the host codec on the same bitmaps copied to the host."""
    counts, strings = ops.mask_rle(masks_gpu)
    host = masks_gpu.cpu().numpy()
    want_counts, want_strings = host_codec(host)
    assert len(counts) == len(strings) == host.shape[0]
    for k in range(host.shape[0]):
        assert counts[k].dtype == torch.int32 and not counts[k].is_cuda
        assert counts[k].tolist() == want_counts[k], k
        assert strings[k] == want_strings[k], k
    return counts, strings


@pytest.mark.parametrize("h,w", SHAPES)
def test_mask_rle_shapes_and_patterns(dev, h, w):
    masks = mask_set(h, w, seed=h * 1000 + w)
    assert masks.shape[0] == 13
    counts, strings = check_against_host(torch.from_numpy(masks).bool().to(dev))
    assert counts[0].tolist() == [h * w] and counts[1].tolist() == [0, h * w]
    assert counts[5].tolist() == [0] + [1] * (h * w)
    if w > 1:
        assert counts[8].tolist() == [((w - 1) // 2 + 1) * h - 1, 2, h * w - ((w - 1) // 2 + 1) * h - 1]   # the pair stays one run


def test_mask_rle_unaligned_buffer(dev):
    """A batch that starts at an odd byte offset of its allocation: the first and last rows are read byte by byte."""
    for h, w in ((5, 3), (97, 131)):
        masks = torch.from_numpy(mask_set(h, w, seed=5)).bool().to(dev)
        part = masks[1:]
        assert part.is_contiguous() and part.data_ptr() % 4 == (h * w) % 4 != 0
        check_against_host(part)


def test_mask_rle_long_runs_and_signed_deltas(dev):
    h, w = 1100, 1000
    head = [0, 1, 70000, 2, 40000, 33, 1, 1, 600000, 31, 32, 1023, 1024, 32767, 32768, 5]
    a = head + [h * w - sum(head)]
    b = head[1:] + [h * w - sum(head[1:])]
    masks = np.stack([mask_from_counts(a, h, w), mask_from_counts(b, h, w)])
    assert wire.rle_counts(masks[0]) == a and wire.rle_counts(masks[1]) == b
    assert len(wire.rle_to_string(a)) == 53
    counts, strings = check_against_host(torch.from_numpy(masks).bool().to(dev))
    assert counts[0].tolist() == a and counts[1].tolist() == b
    assert wire.rle_from_string(strings[0]) == a and wire.rle_from_string(strings[1]) == b


@pytest.mark.parametrize("r", [1, 2, 70])
def test_mask_rle_batch_sizes(dev, r):
    g = torch.Generator().manual_seed(r)
    p = torch.rand((r, 1, 1), generator=g)
    check_against_host((torch.rand((r, 33, 65), generator=g) < p).to(dev))


def test_mask_rle_consecutive_calls_on_one_stream(dev):
    """Different R and (H,W) back to back: nothing of an earlier call's workspace may show in a later one."""
    g = torch.Generator().manual_seed(11)
    first = (torch.rand((5, 97, 131), generator=g) < 0.5).to(dev)
    second = (torch.rand((2, 7, 1), generator=g) < 0.5).to(dev)
    third = (torch.rand((9, 33, 65), generator=g) < 0.1).to(dev)
    got = [ops.mask_rle(m) for m in (first, second, third, first)]
    for m, (counts, strings) in zip((first, second, third, first), got):
        want_counts, want_strings = host_codec(m.cpu().numpy())
        assert [c.tolist() for c in counts] == want_counts and strings == want_strings
    assert ops.mask_rle(torch.zeros((0, 7, 9), dtype=torch.bool, device=dev)) == ([], [])


def _pasted(dev, h, w, n, seed):
    g = torch.Generator().manual_seed(seed)
    soft = torch.rand((n, 28, 28), generator=g)
    xy = torch.rand((n, 2), generator=g) * torch.tensor([w * 0.7, h * 0.7])
    boxes = torch.cat([xy, xy + torch.rand((n, 2), generator=g) * torch.tensor([w * 0.6, h * 0.6]) + 2], dim=1)
    boxes[0] = torch.tensor([-20.0, -10.0, w * 0.4, h * 0.5])                  # partly outside, top left
    boxes[1] = torch.tensor([w * 0.6, h * 0.5, w + 30.0, h + 15.0])            # partly outside, bottom right
    boxes[2] = torch.tensor([0.0, 0.0, float(w), float(h)])                    # the whole image
    boxes[3] = torch.tensor([w * 0.5, 3.0, w * 0.5 + 0.6, h - 3.0])            # narrower than one pixel
    soft[2] = 0.5 + 0.5 * soft[2]                                              # the inside of the whole-image box is foreground
    return ops.paste_masks(soft.to(dev), boxes.to(dev), h, w), boxes


@pytest.fixture(scope="module")
def pasted(dev):
    return [_pasted(dev, 97, 131, 9, 21), _pasted(dev, 257, 130, 5, 22)]


def test_mask_rle_of_pasted_masks(dev, pasted):
    for masks, _ in pasted:
        assert masks.dtype == torch.bool and masks.is_cuda
        host = masks.cpu().numpy()
        assert all(0 < m.sum() for m in host[:3]) and host.sum() < host.size
        _, strings = check_against_host(masks)
        for k, s in enumerate(strings):
            assert np.array_equal(wire.rle_decode({"size": list(host.shape[1:]), "counts": s}), host[k])
        assert wire.rle_encode_batch(masks) == [wire.rle_encode(m) for m in host]


def test_coco_json_of_gpu_instances_equals_cpu_instances(dev, pasted):
    for (masks, boxes), img_id in zip(pasted, (3, 4)):
        n, h, w = masks.shape
        g = torch.Generator().manual_seed(n)
        inst = Instances((h, w), pred_boxes=Boxes(boxes.to(dev)), scores=torch.rand(n, generator=g).to(dev),
                         pred_classes=torch.randint(0, 80, (n,), generator=g).to(dev), pred_masks=masks,
                         mask_scores=torch.rand(n, generator=g).to(dev))
        got = wire.instances_to_coco_json(inst, img_id)
        assert got == wire.instances_to_coco_json(inst.to("cpu"), img_id)
        assert len(got) == n and all(isinstance(r["segmentation"]["counts"], str) and r["segmentation"]["size"] == [h, w] for r in got)
        assert json.loads(json.dumps(got)) == got


def test_mask_rle_input_handling(dev):
    g = torch.Generator().manual_seed(31)
    masks = (torch.rand((4, 66, 37), generator=g) < 0.3).to(dev)
    part = masks[:, ::2]
    assert not part.is_contiguous()
    check_against_host(part)
    for bad in (masks.to(torch.uint8), masks.float(), masks[0]):
        with pytest.raises(_lib.CmkError):
            ops.mask_rle(bad)
