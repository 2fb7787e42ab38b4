"""-m gpu: the resize kernels (csrc/resize.hip) against Pillow's stored outputs (tests/golden/resize_pil.pt, made by
make_golden_resize.py; PIL is not needed here), byte for byte, and the fused resize + normalise + pad against ops.preprocess_images fed
the stored resized images: the same kernel expression, so the same bits."""
import pytest
import torch

from centermask2_amd import ops
from .helpers import golden

pytestmark = pytest.mark.gpu

MEAN, STD = (103.53, 116.28, 123.675), (1.0, 57.0, 2.0)
SHORT, MAX_SIZE = 80, 133


@pytest.fixture(scope="module")
def fixture():
    return golden("resize_pil")


@pytest.fixture(scope="module")
def batch3(dev, fixture):
    """The three shape-rule images as one mixed-size batch through the code under test, and the parent's device path for the same batch:
    preprocess_images on Pillow's resized images as CHW uint8.  Computed once, read by the tests below."""
    cases = fixture["rule_images"]
    got, sizes = ops.resize_preprocess_images([c["src"].to(dev) for c in cases], SHORT, MAX_SIZE, MEAN, STD)
    want, want_sizes = ops.preprocess_images([c["out"].permute(2, 0, 1).contiguous().to(dev) for c in cases], MEAN, STD)
    torch.cuda.synchronize()
    return dict(cases=cases, got=got, sizes=sizes, want=want, want_sizes=want_sizes)


@pytest.mark.parametrize("i", range(8))
def test_resize_bilinear_u8_equals_pillow_byte_for_byte(dev, fixture, i):
    c = fixture["ops"][i]
    h, w, new_h, new_w = c["size"]
    out = ops.resize_bilinear_u8(c["src"].to(dev), new_h, new_w)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (new_h, new_w, 3) and out.is_contiguous()
    got = out.cpu()
    assert torch.equal(got, c["out"]), "{}x{} -> {}x{}: {} bytes differ".format(h, w, new_h, new_w, int((got != c["out"]).sum()))


def test_resize_preprocess_batch_has_the_bits_of_preprocess_images(batch3):
    assert batch3["sizes"] == [(80, 107), (107, 80), (40, 133)] == batch3["want_sizes"]
    assert batch3["sizes"] == [tuple(c["size"][2:]) for c in batch3["cases"]]
    assert tuple(batch3["got"].shape) == (3, 3, 128, 160) == tuple(batch3["want"].shape) and batch3["got"].dtype == torch.float32
    assert torch.equal(batch3["got"], batch3["want"])


def test_resize_preprocess_batch_matches_cpu_normalisation_and_pads_with_zero(batch3):
    got = batch3["got"].cpu()
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    for i, c in enumerate(batch3["cases"]):
        new_h, new_w = c["size"][2:]
        ref = (c["out"].permute(2, 0, 1).float() - mean) / std
        assert torch.allclose(got[i, :, :new_h, :new_w], ref, rtol=0, atol=1e-5)
        assert (got[i, :, new_h:, :] == 0).all() and (got[i, :, :, new_w:] == 0).all()
        assert got[i, :, new_h:, :].numel() + got[i, :, :, new_w:].numel() > 0


def test_resize_preprocess_fixed_size_and_divisibility(dev, batch3):
    srcs = [c["src"].to(dev) for c in batch3["cases"]]
    out, sizes = ops.resize_preprocess_images(srcs, SHORT, MAX_SIZE, MEAN, STD, fixed_size=160)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, 3, 160, 160) and sizes == batch3["sizes"]
    assert torch.equal(out[:, :, :128, :], batch3["got"]) and (out[:, :, 128:, :] == 0).all()
    out1, _ = ops.resize_preprocess_images(srcs, SHORT, MAX_SIZE, MEAN, STD, size_divisibility=1)      # W = 133: no 16-byte alignment of the rows
    torch.cuda.synchronize()
    assert tuple(out1.shape) == (3, 3, 107, 133) and torch.equal(out1, batch3["got"][:, :, :107, :133])


def test_resize_preprocess_reverse_channels_equals_the_flipped_source(dev, batch3):
    srcs = [c["src"].to(dev) for c in batch3["cases"]]
    rev, sizes = ops.resize_preprocess_images(srcs, SHORT, MAX_SIZE, MEAN, STD, reverse_channels=True)
    flipped, _ = ops.resize_preprocess_images([s.flip(2).contiguous() for s in srcs], SHORT, MAX_SIZE, MEAN, STD)
    torch.cuda.synchronize()
    assert sizes == batch3["sizes"] and torch.equal(rev, flipped)
    assert not torch.equal(rev, batch3["got"])


def test_every_element_of_the_batch_is_written(dev, batch3, monkeypatch):
    """The batch tensor comes from torch.empty: hand the call one pre-filled with NaN and look for what is left."""
    real_empty = torch.empty
    filled = []

    def nan_empty(*a, **kw):
        t = real_empty(*a, **kw)
        if t.dtype == torch.float32:
            t.fill_(float("nan"))
            filled.append(t)
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)
    out, _ = ops.resize_preprocess_images([c["src"].to(dev) for c in batch3["cases"]], SHORT, MAX_SIZE, MEAN, STD)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(filled) == 1 and filled[0].data_ptr() == out.data_ptr()
    assert not torch.isnan(out).any() and torch.equal(out, batch3["got"])


def test_second_call_reuses_the_cached_tables_and_repeats_the_output(dev, batch3):
    srcs = [c["src"].to(dev) for c in batch3["cases"]]
    ops.resize_preprocess_images(srcs, SHORT, MAX_SIZE, MEAN, STD)
    tables = dict(ops._RESIZE_TABLES)
    for (h, w, new_h, new_w) in (c["size"] for c in batch3["cases"]):
        assert (dev.index, h, new_h) in tables and (dev.index, w, new_w) in tables
    again, sizes = ops.resize_preprocess_images(srcs, SHORT, MAX_SIZE, MEAN, STD)
    torch.cuda.synchronize()
    assert sizes == batch3["sizes"] and torch.equal(again, batch3["got"])
    assert set(ops._RESIZE_TABLES) == set(tables) and all(ops._RESIZE_TABLES[k][0] is tables[k][0] for k in tables)      # nothing uploaded


def test_wrong_inputs_on_the_device_are_refused(dev):
    from centermask2_amd._lib import CmkError
    for bad in (torch.zeros((8, 8, 3), dtype=torch.float32, device=dev), torch.zeros((8, 8, 4), dtype=torch.uint8, device=dev)):
        with pytest.raises(CmkError):
            ops.resize_preprocess_images([bad], SHORT, MAX_SIZE, MEAN, STD)
    with pytest.raises(CmkError):
        ops.resize_bilinear_u8(torch.zeros((8, 8, 3), dtype=torch.uint8, device=dev), 0, 4)
