"""-m gpu: the mask IoU kernels of COCO evaluation (csrc/mask_iou.hip through ops.mask_pack_bits / ops.mask_rle_decode /
ops.mask_intersections) against NumPy on the same bitmaps, and evaluation.COCOEvaluator on GPU Instances against the same Instances on
the host.  Every result is an integer (or a float formed from identical integers): every comparison is ==, no tolerance anywhere.

Tiles of the kernels: pack and decode take 8 words (512 pixels) per wave and 32 words (2048 pixels) per workgroup; the intersection
kernel takes 512 words (32768 pixels) and 16 detections per workgroup and stages 16 ground truths per LDS tile.  97x131 is 199 words
(7 pack workgroups, the last partial, a partial last word), 257x130 is 523 words (two intersection chunks, the second of 11 words);
64x64 is exactly 64 words, 1x1 and 7x9 are a single partial word; N = 17 and 70 pass 16 detections by non-multiples, M = 17 and 33 pass
the LDS tile likewise."""
import numpy as np
import pytest
import torch

from centermask2_amd import _lib, ops, wire
from centermask2_amd.evaluation import COCOEvaluator
from tests import coco_cases as C

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 9), (64, 64), (33, 65), (97, 131), (257, 130)]


def mask_set(h, w, seed):
    z = np.zeros((h, w), dtype=np.uint8)
    out = [z.copy(), 1 - z]                                             # empty, full
    m = z.copy(); m[0, 0] = 1; out.append(m)                            # the first pixel (a zero-length first run)
    m = z.copy(); m[h - 1, w - 1] = 1; out.append(m)                    # the last pixel
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(((yy + xx) & 1).astype(np.uint8))                        # checkerboard
    m = z.copy(); m[h // 2, :] = 1; out.append(m)                       # one row: every run crosses a column boundary
    m = z.copy(); m[:, w // 2] = 1; out.append(m)                       # one column
    x = (w - 1) // 2
    m = z.copy(); m[h - 1, x] = 1; m[0, min(x + 1, w - 1)] = 1          # bottom of a column and top of the next: one run
    out.append(m)
    rng = np.random.RandomState(seed)
    for p in (0.02, 0.5, 0.98):
        out.append((rng.rand(h, w) < p).astype(np.uint8))
    return np.stack(out)


def packed(masks_np):
    """(R,H,W) 0/1 -> (R, ceil(HW/64)) uint64, bit p % 64 of word p / 64 = row-major pixel p."""
    r = masks_np.shape[0]
    flat = masks_np.reshape(r, -1).astype(np.uint8)
    nw = (flat.shape[1] + 63) // 64
    pad = np.zeros((r, nw * 64), dtype=np.uint8)
    pad[:, :flat.shape[1]] = flat
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view(np.uint64)


def words_of(t):
    return t.cpu().numpy().view(np.uint64)


def check_pack(masks_gpu):
    words, areas = ops.mask_pack_bits(masks_gpu)
    host = masks_gpu.cpu().numpy()
    r, h, w = host.shape
    assert words.dtype == torch.int64 and areas.dtype == torch.int32 and words.is_cuda and areas.is_cuda
    assert tuple(words.shape) == (r, (h * w + 63) // 64) and tuple(areas.shape) == (r,)
    got = words_of(words)
    assert np.array_equal(got, packed(host))
    assert areas.cpu().tolist() == host.reshape(r, -1).sum(1).tolist()
    if (h * w) % 64 and r:
        assert not (got[:, -1] >> np.uint64((h * w) % 64)).any()        # the unused high bits of the last word
    return words, areas


@pytest.fixture(scope="module")
def sets(dev):
    """Per shape the pattern set on the host and on the device, shared by the tests below and never modified."""
    out = {}
    for h, w in SHAPES:
        m = mask_set(h, w, seed=h * 1000 + w)
        out[(h, w)] = (m, torch.from_numpy(m).bool().to(dev))
    return out


@pytest.mark.parametrize("h,w", SHAPES)
def test_pack_bits_shapes_and_patterns(sets, h, w):
    host, gpu = sets[(h, w)]
    assert host.shape[0] == 11
    words, areas = check_pack(gpu)
    assert areas.cpu().tolist()[:4] == [0, h * w, 1, 1]


@pytest.mark.parametrize("h,w", SHAPES)
def test_rle_decode_inverts_the_encoder(sets, h, w):
    host, gpu = sets[(h, w)]
    counts, strings = ops.mask_rle(gpu)
    back = ops.mask_rle_decode(counts, h, w)
    assert back.dtype == torch.bool and back.is_cuda and tuple(back.shape) == host.shape
    assert torch.equal(back, gpu)
    for k, s in enumerate(strings):
        assert np.array_equal(back[k].cpu().numpy(), wire.rle_decode({"size": [h, w], "counts": s})), k
    assert counts[0].tolist() == [h * w] and counts[2].tolist()[0] == 0          # a single run; a zero-length first run
    # the same runs as plain lists, and the packed form without the bitmaps
    words, areas = ops.mask_rle_decode([c.tolist() for c in counts], h, w, want_bitmasks=False)
    assert np.array_equal(words_of(words), packed(host)) and areas.cpu().tolist() == host.reshape(len(host), -1).sum(1).tolist()


def test_rle_decode_refuses_counts_with_a_wrong_total(dev):
    good = ops.mask_rle(torch.ones((1, 7, 9), dtype=torch.bool, device=dev))[0]
    assert torch.equal(ops.mask_rle_decode(good, 7, 9), torch.ones((1, 7, 9), dtype=torch.bool, device=dev))
    for bad in ([[62]], [[0, 64]], [[10, 20, 30]], [[]], good + [[5]]):
        with pytest.raises(_lib.CmkError, match="add up"):
            ops.mask_rle_decode(bad, 7, 9)
    with pytest.raises(_lib.CmkError):
        ops.mask_rle_decode(good, 9, 8)
    assert tuple(ops.mask_rle_decode([], 7, 9).shape) == (0, 7, 9)


def _random_masks(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand((n, 1, 1), generator=g) if n else torch.zeros((0, 1, 1))
    return torch.rand((n, h, w), generator=g) < p


def check_intersections(dev, n, m, h, w, seed):
    a, b = _random_masks(n, h, w, seed), _random_masks(m, h, w, seed + 1)
    inter, a_dt, a_gt = ops.mask_intersections(a.to(dev), [wire.rle_counts(x) for x in b.numpy()], h, w)
    for t in (inter, a_dt, a_gt):
        assert t.dtype == torch.int32 and not t.is_cuda
    an, bn = a.numpy().reshape(n, h * w).astype(np.int64), b.numpy().reshape(m, h * w).astype(np.int64)
    assert tuple(inter.shape) == (n, m) and np.array_equal(inter.numpy().astype(np.int64), an @ bn.T)
    assert a_dt.tolist() == an.sum(1).tolist() and a_gt.tolist() == bn.sum(1).tolist()


@pytest.mark.parametrize("n,m", [(0, 3), (3, 0), (1, 1), (3, 17), (70, 5), (17, 33)])
def test_intersections_against_the_integer_matrix_product(dev, n, m):
    for h, w in ((97, 131), (257, 130)):
        check_intersections(dev, n, m, h, w, seed=100 * n + m)


def test_intersections_of_the_pattern_sets(dev, sets):
    """Every pattern against every pattern, at every shape: full against full is H*W, the checkerboard against a row half of it."""
    for (h, w), (host, gpu) in sets.items():
        inter, a_dt, a_gt = ops.mask_intersections(gpu, [wire.rle_counts(m) for m in host], h, w)
        flat = host.reshape(len(host), -1).astype(np.int64)
        assert np.array_equal(inter.numpy().astype(np.int64), flat @ flat.T), (h, w)
        assert a_dt.tolist() == a_gt.tolist() == flat.sum(1).tolist()


def test_back_to_back_calls_of_different_shapes_on_one_stream(dev):
    """Nothing of an earlier call (the zeroed table, the packed words) may show in a later one."""
    for n, m, h, w in ((17, 33, 257, 130), (1, 1, 1, 1), (70, 5, 33, 65), (3, 17, 97, 131), (17, 33, 257, 130)):
        check_intersections(dev, n, m, h, w, seed=n + m + h)
    g = _random_masks(5, 97, 131, 3).to(dev)
    first = ops.mask_pack_bits(g)
    ops.mask_pack_bits(_random_masks(9, 33, 65, 4).to(dev))
    again = ops.mask_pack_bits(g)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert tuple(ops.mask_pack_bits(torch.zeros((0, 7, 9), dtype=torch.bool, device=dev))[0].shape) == (0, 1)


def test_input_handling(dev, sets):
    for h, w in ((7, 9), (97, 131)):
        gpu = sets[(h, w)][1]
        part = gpu[1:]                                                   # a batch that starts at an odd byte offset
        assert part.is_contiguous() and part.data_ptr() % 2 == 1
        check_pack(part)
        counts = [wire.rle_counts(m) for m in sets[(h, w)][0][:3]]
        inter = ops.mask_intersections(part, counts, h, w)[0]
        flat = sets[(h, w)][0].reshape(11, -1).astype(np.int64)
        assert np.array_equal(inter.numpy().astype(np.int64), flat[1:] @ flat[:3].T)
    masks = _random_masks(4, 66, 37, 31).to(dev)
    part = masks[:, ::2]
    assert not part.is_contiguous()
    check_pack(part)
    for bad in (masks.to(torch.uint8), masks.float(), masks[0]):
        with pytest.raises(_lib.CmkError):
            ops.mask_pack_bits(bad)
        with pytest.raises(_lib.CmkError):
            ops.mask_intersections(bad, [[66 * 37]], 66, 37)
    with pytest.raises(_lib.CmkError, match="97x131"):
        ops.mask_intersections(masks, [[97 * 131]], 97, 131)


def _pasted(dev, h, w, n, seed):
    """Masks as the model's output side makes them: boxes partly outside the image, the whole image, narrower than one pixel."""
    g = torch.Generator().manual_seed(seed)
    soft = torch.rand((n, 28, 28), generator=g)
    xy = torch.rand((n, 2), generator=g) * torch.tensor([w * 0.7, h * 0.7])
    boxes = torch.cat([xy, xy + torch.rand((n, 2), generator=g) * torch.tensor([w * 0.6, h * 0.6]) + 2], dim=1)
    boxes[0] = torch.tensor([-20.0, -10.0, w * 0.4, h * 0.5])
    boxes[1] = torch.tensor([w * 0.6, h * 0.5, w + 30.0, h + 15.0])
    boxes[2] = torch.tensor([0.0, 0.0, float(w), float(h)])
    boxes[3] = torch.tensor([w * 0.5, 3.0, w * 0.5 + 0.6, h - 3.0])
    soft[2] = 0.5 + 0.5 * soft[2]
    return ops.paste_masks(soft.to(dev), boxes.to(dev), h, w)


def test_pasted_masks(dev):
    for h, w, n, seed in ((97, 131, 9, 21), (257, 130, 5, 22)):
        masks = _pasted(dev, h, w, n, seed)
        host = masks.cpu().numpy()
        assert masks.dtype == torch.bool and all(0 < m.sum() for m in host[:3]) and host.sum() < host.size
        check_pack(masks)
        assert torch.equal(ops.mask_rle_decode(ops.mask_rle(masks)[0], h, w), masks)
        inter, a_dt, a_gt = ops.mask_intersections(masks, [wire.rle_counts(m) for m in host], h, w)
        flat = host.reshape(n, -1).astype(np.int64)
        assert np.array_equal(inter.numpy().astype(np.int64), flat @ flat.T) and a_dt.tolist() == a_gt.tolist() == flat.sum(1).tolist()


def test_evaluator_on_gpu_instances_equals_the_host_path(dev):
    ds, per_image = C.mixed_case()
    results = []
    for where in (dev, "cpu"):
        ev = COCOEvaluator(ds)
        ev.process([{"image_id": i} for i, _ in per_image], [{"instances": inst.to(where)} for _, inst in per_image])
        for p in ev._predictions:
            assert p["table"][0].shape == (len(p["instances"]), 5)
        results.append((ev.evaluate(), [p["table"] for p in ev._predictions]))
    (gpu, gpu_tables), (cpu, cpu_tables) = results
    for a, b in zip(gpu_tables, cpu_tables):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert C.same(gpu, cpu)
    assert set(gpu) == {"bbox", "segm"} and 0.0 < gpu["segm"]["AP"] < 100.0 and 0.0 < gpu["bbox"]["AP"] < 100.0
