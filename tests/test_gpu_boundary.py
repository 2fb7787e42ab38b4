"""-m gpu: the boundary kernel of Boundary AP (mask_boundary_kernel and mask_unpack_kernel of csrc/mask_iou.hip through
ops.mask_boundary_bits / ops.mask_boundary / ops.mask_boundary_intersections) against the literal definition in tests/boundary_ref.py, and
evaluation.COCOEvaluator with the task "boundary" on GPU Instances against the same Instances on the host.  Every result is an integer
(or a float formed from identical integers): every comparison is ==, no tolerance anywhere.

Shapes, each for a way the kernel can go wrong (a tile re-aligns rows of the linear bit stream to words, erodes along x by funnel shifts
over three words, along y by word ANDs over 2d+1 rows of a band with a halo, and ORs the result back shifted): 1x1 and 7x9 are one partial
word; 40x20 has several rows per word; 64x64 and 20x128 have word-aligned rows; 33x65 and 31x63 straddle words by one bit; 97x131 ends in
a partial word; 257x130 has more rows than a band (at most max(4d, 64) rows: 5 bands of 52 rows and a last of 49 up to d = 16, 129 and 128
rows at d = 40), so the halo between bands and a ragged last band are exercised; 97x131 is two bands up to d = 16.  d = 1, 2, 5, 16, 40 puts 2d+1 below, at (d = 16 with the doubling steps 1, 2, 4, 8, 1) and above 64, and
above W or H for the small shapes, where the boundary is the mask."""
import numpy as np
import pytest
import torch

from centermask2_amd import _lib, ops, wire
from centermask2_amd.evaluation import COCOEvaluator
from tests import boundary_ref as B
from tests import coco_cases as C
from tests.test_gpu_coco_eval import _pasted

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 9), (40, 20), (64, 64), (20, 128), (33, 65), (31, 63), (97, 131), (257, 130)]
DS = [1, 2, 5, 16, 40]


def words_of(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def sets(dev):
    """Per shape the pattern set on the host and on the device and, per d, its reference boundary: computed once, never modified."""
    out = {}
    for h, w in SHAPES:
        m = B.mask_set(h, w, seed=h * 1000 + w)
        out[(h, w)] = (m, torch.from_numpy(m).bool().to(dev), {d: B.boundary_ref(m, d) for d in DS})
    return out


def check_words(bwords, bareas, want, h, w):
    r = want.shape[0]
    assert bwords.dtype == torch.int64 and bareas.dtype == torch.int32 and bwords.is_cuda and bareas.is_cuda
    assert tuple(bwords.shape) == (r, (h * w + 63) // 64) and tuple(bareas.shape) == (r,)
    got = words_of(bwords)
    assert np.array_equal(got, B.packed(want)), (h, w)
    assert bareas.cpu().tolist() == want.reshape(r, -1).sum(1).tolist()
    if (h * w) % 64 and r:
        assert not (got[:, -1] >> np.uint64((h * w) % 64)).any()         # the unused high bits of the last word


@pytest.mark.parametrize("h,w", SHAPES)
def test_boundary_bits_against_the_reference_through_both_producers(sets, h, w):
    host, gpu, want = sets[(h, w)]
    packed, _ = ops.mask_pack_bits(gpu)
    decoded, _ = ops.mask_rle_decode([wire.rle_counts(m) for m in host], h, w, want_bitmasks=False)
    assert torch.equal(packed, decoded)
    for d in DS:
        for words in (packed, decoded):
            bwords, bareas = ops.mask_boundary_bits(words, h, w, d)
            check_words(bwords, bareas, want[d], h, w)
        if 2 * d + 1 > min(h, w):
            assert torch.equal(bwords, packed)                           # nothing survives the erosion: the boundary is the mask
    assert torch.equal(packed, decoded) and np.array_equal(words_of(packed), B.packed(host))        # the input is left alone


@pytest.mark.parametrize("h,w", [(7, 9), (33, 65), (97, 131)])
def test_mask_boundary_gives_the_bitmaps(sets, h, w):
    host, gpu, want = sets[(h, w)]
    for d in (1, 5, 16):
        got = ops.mask_boundary(gpu, d)
        assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == host.shape
        assert np.array_equal(got.cpu().numpy(), want[d]), (h, w, d)
    d = ops.boundary_dilation(h, w)
    assert np.array_equal(ops.mask_boundary(gpu).cpu().numpy(), B.boundary_ref(host, d))
    words, _ = ops.mask_pack_bits(gpu)
    assert torch.equal(ops.mask_unpack_bits(words, h, w), gpu)
    assert tuple(ops.mask_boundary(gpu[:0], 2).shape) == (0, h, w)


def test_pasted_masks(dev):
    for h, w, n, seed, d in ((97, 131, 9, 21, 3), (257, 130, 5, 22, 6)):
        masks = _pasted(dev, h, w, n, seed)
        host = masks.cpu().numpy()
        want = B.boundary_ref(host, d)
        assert 0 < want.sum() < host.sum()
        check_words(*ops.mask_boundary_bits(ops.mask_pack_bits(masks)[0], h, w, d), want, h, w)
        assert np.array_equal(ops.mask_boundary(masks, d).cpu().numpy(), want)


def _solid(n, h, w, seed):
    """n seeded masks that survive an erosion: unions of a rectangle and a disc, some cut by the image edge, a few pixels knocked out."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        y0, x0 = rng.randint(-h // 4, h // 2), rng.randint(-w // 4, w // 2)
        m = B.rect(h, w, y0, y0 + rng.randint(h // 4, h), x0, x0 + rng.randint(w // 4, w))
        m |= B.disc(h, w, rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.1, 0.4) * min(h, w))
        out.append(m & (rng.rand(h, w) < 0.999))
    return np.stack(out).astype(np.uint8) if n else np.zeros((0, h, w), dtype=np.uint8)


@pytest.mark.parametrize("r", [11, 17])
def test_odd_batches(dev, r):
    h, w, d = 97, 131, 5
    host = _solid(r, h, w, seed=r)
    want = B.boundary_ref(host, d)
    assert all(0 < b.sum() < m.sum() for b, m in zip(want[:3], host[:3]))
    check_words(*ops.mask_boundary_bits(ops.mask_pack_bits(torch.from_numpy(host).bool().to(dev))[0], h, w, d), want, h, w)


def test_back_to_back_calls_of_different_shapes_on_one_stream(dev, sets):
    """Nothing of an earlier call (the zeroed words the kernel ORs into, the areas) may show in a later one."""
    seq = [((257, 130), 16), ((1, 1), 1), ((33, 65), 5), ((257, 130), 2), ((40, 20), 40), ((97, 131), 16), ((257, 130), 16)]
    packed = {s: ops.mask_pack_bits(sets[s][1])[0] for s, _ in seq}
    results = [ops.mask_boundary_bits(packed[s], s[0], s[1], d) for s, d in seq]          # queued without a host read in between
    for (s, d), (bwords, bareas) in zip(seq, results):
        check_words(bwords, bareas, sets[s][2][d], *s)
    assert torch.equal(results[0][0], results[-1][0]) and torch.equal(results[0][1], results[-1][1])
    assert tuple(ops.mask_boundary_bits(packed[(33, 65)][:0], 33, 65, 3)[0].shape) == (0, 34)


@pytest.mark.parametrize("n,m", [(0, 3), (3, 0), (1, 1), (17, 33)])
def test_boundary_intersections_against_the_integer_matrix_product(dev, n, m):
    h, w, d = 97, 131, 4
    a, b = _solid(n, h, w, seed=100 * n + m), _solid(m, h, w, seed=100 * n + m + 1)
    counts = [wire.rle_counts(x) for x in b]
    gpu = torch.from_numpy(a).bool().to(dev)
    six = ops.mask_boundary_intersections(gpu, counts, h, w, d)
    assert len(six) == 6
    for t in six:
        assert t.dtype == torch.int32 and not t.is_cuda
    three = ops.mask_intersections(gpu, counts, h, w)
    assert all(torch.equal(x, y) for x, y in zip(six[:3], three))
    for k, (x, y) in enumerate(((a, b), (B.boundary_ref(a, d), B.boundary_ref(b, d)))):
        xn, yn = x.reshape(n, h * w).astype(np.int64), y.reshape(m, h * w).astype(np.int64)
        inter, a_dt, a_gt = six[3 * k:3 * k + 3]
        assert tuple(inter.shape) == (n, m) and np.array_equal(inter.numpy().astype(np.int64), xn @ yn.T), k
        assert a_dt.tolist() == xn.sum(1).tolist() and a_gt.tolist() == yn.sum(1).tolist(), k
    if n and m:
        assert six[3].sum() > 0 and (six[3].numpy() <= six[0].numpy()).all()


def test_input_handling(dev, sets):
    host, gpu, want = sets[(97, 131)]
    words, _ = ops.mask_pack_bits(gpu)
    part = words[1:]                                                     # a batch that does not start at the allocation
    check_words(*ops.mask_boundary_bits(part, 97, 131, 5), want[5][1:], 97, 131)
    for bad, h, w, d in ((words, 97, 130, 5), (words.to(torch.int32), 97, 131, 5), (words[0], 97, 131, 5), (words, 97, 131, 0),
                         (words.cpu(), 97, 131, 5)):
        with pytest.raises(_lib.CmkError):
            ops.mask_boundary_bits(bad, h, w, d)
    with pytest.raises(_lib.CmkError, match="97x131"):
        ops.mask_boundary_intersections(gpu[:, :7, :9].contiguous(), [[97 * 131]], 97, 131, 3)


def test_evaluator_on_gpu_instances_equals_the_host_path(dev):
    ds, per_image = C.mixed_case()
    results = []
    for where in (dev, "cpu"):
        ev = COCOEvaluator(ds, tasks=("bbox", "segm", "boundary"))
        ev.process([{"image_id": i} for i, _ in per_image], [{"instances": inst.to(where)} for _, inst in per_image])
        for p in ev._predictions:
            assert len(p["table"]) == 3 and p["table"][0].shape == (len(p["instances"]), 5) == p["boundary_table"][0].shape
        results.append((ev.evaluate(), [p["table"] + p["boundary_table"] for p in ev._predictions]))
    (gpu, gpu_tables), (cpu, cpu_tables) = results
    for a, b in zip(gpu_tables, cpu_tables):
        assert len(a) == len(b) == 6 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert C.same(gpu, cpu)
    assert set(gpu) == {"bbox", "segm", "boundary"} and set(gpu["boundary"]) == set(gpu["segm"])
    assert 0.0 <= gpu["boundary"]["AP"] <= gpu["segm"]["AP"]
    # without the task nothing of it appears
    ev = COCOEvaluator(ds)
    ev.process([{"image_id": i} for i, _ in per_image], [{"instances": inst.to(dev)} for _, inst in per_image])
    assert all("boundary_table" not in p for p in ev._predictions) and set(ev.evaluate()) == {"bbox", "segm"}
