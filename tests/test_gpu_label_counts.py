"""-m gpu: the overlap-count kernel of Cityscapes evaluation (csrc/eval/label_counts.hip through ops.mask_label_counts and the C entry
cmk_mask_label_counts) against np.bincount on the same bitmaps.  Every result is an integer: every comparison is ==.

Tiles of the kernel: a workgroup is one wave that owns 256 words (16384 pixels) of one mask, 4 words per lane; it leaves early when all
of them are zero, and reads the labels of up to 8 non-zero words at a time.  1x1 and 7x9 are a single partial word, 1x64 and 64x64
exactly 1 and 64 words, 33x130 is 68 words (two rounds of lanes, the second partial, a partial last word; 64 non-zero words are full
batches, 4 a partial one), 257x130 is 523 words: three workgroups per mask, the last of 11 words.  C = 4096 fills
the 16 KiB histogram (64 counters per lane), C = 37 is below one counter per lane, C = 1 and 2 are the degenerate tables."""
import ctypes

import numpy as np
import pytest
import torch

from centermask2_amd import _lib, ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 64), (7, 9), (64, 64), (33, 130), (257, 130)]
COLS = [1, 2, 37, 4096]
GUARD = 64
SENTINEL = 0x5a5a5a5a


def mask_set(h, w, seed):
    """Empty, full, the first pixel only, the last pixel only, and random at three densities."""
    z = np.zeros((h, w), dtype=bool)
    first, last = z.copy(), z.copy()
    first[0, 0] = True
    last[h - 1, w - 1] = True
    rng = np.random.RandomState(seed)
    return np.stack([z, ~z, first, last] + [rng.rand(h, w) < p for p in (0.02, 0.5, 0.98)])


def label_image(h, w, c, seed, kind):
    """kind "noise": every pixel its own column (up to 64 distinct columns under one word); "runs": blocks of rows and columns share one,
    as ground-truth regions do; "one": all pixels in the last column; "over": noise that reaches past C, with 65535 among the values."""
    rng = np.random.RandomState(seed)
    if kind == "noise":
        return rng.randint(0, c, size=(h, w)).astype(np.uint16)
    if kind == "runs":
        by, bx = max(1, h // 5), max(1, w // 7)
        blocks = rng.randint(0, c, size=(h // by + 1, w // bx + 1))
        return blocks[np.arange(h)[:, None] // by, np.arange(w)[None, :] // bx].astype(np.uint16)
    if kind == "one":
        return np.full((h, w), c - 1, dtype=np.uint16)
    out = rng.randint(0, c + 6, size=(h, w)).astype(np.uint16)
    out[rng.rand(h, w) < 0.1] = 65535
    out[h - 1, w - 1] = c                                               # the first value outside, under the last pixel
    return out


def expected(masks, cols, c):
    table = np.zeros((masks.shape[0], c), dtype=np.int64)
    for n, m in enumerate(masks):
        under = cols[m].astype(np.int64)
        table[n] = np.bincount(under[under < c], minlength=c)
    return table


def run_entry(masks_gpu, cols, c):
    """The C entry on a table that lies between two guard regions -> (table, guards intact)."""
    n, h, w = masks_gpu.shape
    words, _ = ops.mask_pack_bits(masks_gpu)
    cols_dev = torch.from_numpy(cols.view(np.int16)).to(masks_gpu.device)
    buf = torch.full((GUARD + n * c + GUARD,), SENTINEL, dtype=torch.int32, device=masks_gpu.device)
    table_ptr = buf.data_ptr() + 4 * GUARD
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.load().cmk_mask_label_counts(words.data_ptr(), n, cols_dev.data_ptr(), h, w, c, table_ptr, stream)
    assert rc == 0, _lib.load().cmk_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = (host[:GUARD] == SENTINEL).all() and (host[GUARD + n * c:] == SENTINEL).all()
    return host[GUARD:GUARD + n * c].reshape(n, c), bool(intact)


@pytest.mark.parametrize("h,w", SHAPES)
def test_counts_equal_bincount(dev, h, w):
    masks = mask_set(h, w, seed=h * 1000 + w)
    gpu = torch.from_numpy(masks).to(dev)
    for c in COLS:
        for kind in ("noise", "runs", "one", "over"):
            cols = label_image(h, w, c, seed=c + len(kind), kind=kind)
            want = expected(masks, cols, c)
            table, areas = ops.mask_label_counts(gpu, cols, c)
            assert table.dtype == torch.int32 and areas.dtype == torch.int32 and not table.is_cuda and tuple(table.shape) == (len(masks), c)
            assert np.array_equal(table.numpy(), want), (c, kind)
            assert areas.tolist() == masks.reshape(len(masks), -1).sum(1).tolist()
            if kind == "one":
                assert table[:, c - 1].tolist() == areas.tolist() and int(table.sum()) == int(areas.sum())
            if kind in ("over", "one"):                                 # nothing outside the table is written, whatever the labels hold
                got, intact = run_entry(gpu, cols, c)
                assert intact, (c, kind)
                assert np.array_equal(got, want), (c, kind)
            if kind == "over" and h * w > 1:
                assert (want.sum(1) < masks.reshape(len(masks), -1).sum(1))[1], "the full mask must lose the pixels whose column is outside"


@pytest.mark.parametrize("n", [0, 1, 17])
def test_mask_counts(dev, n):
    h, w, c = 33, 130, 37
    rng = np.random.RandomState(n)
    masks = rng.rand(n, h, w) < 0.3
    cols = label_image(h, w, c, seed=9, kind="runs")
    table, areas = ops.mask_label_counts(torch.from_numpy(masks).to(dev), cols, c)
    assert tuple(table.shape) == (n, c) and tuple(areas.shape) == (n,)
    assert np.array_equal(table.numpy(), expected(masks, cols, c)) and areas.tolist() == masks.sum(axis=(1, 2)).tolist()
    if n:
        got, intact = run_entry(torch.from_numpy(masks).to(dev), cols, c)
        assert intact and np.array_equal(got, expected(masks, cols, c))
        again, _ = run_entry(torch.from_numpy(masks).to(dev), cols, c)   # integers: the same bits every time
        assert np.array_equal(again, got)
    else:                                                               # N == 0: CMK_OK, and the table pointer is never written
        buf = torch.full((8,), SENTINEL, dtype=torch.int32, device=dev)
        cols_dev = torch.from_numpy(cols.view(np.int16)).to(dev)
        assert _lib.load().cmk_mask_label_counts(buf.data_ptr(), 0, cols_dev.data_ptr(), h, w, c, buf.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()


def test_the_wrapper_refuses_what_the_entry_would(dev):
    m = torch.zeros((1, 4, 4), dtype=torch.bool, device=dev)
    cols = np.zeros((4, 4), dtype=np.uint16)
    for bad_cols, c, word in [(cols, 0, "columns"), (cols, 4097, "columns"), (cols.astype(np.int32), 2, "uint16"), (cols[:3], 2, "uint16")]:
        with pytest.raises(_lib.CmkError, match=word):
            ops.mask_label_counts(m, bad_cols, c)
    with pytest.raises(_lib.CmkError, match="bool"):
        ops.mask_label_counts(m.to(torch.uint8), cols, 2)
