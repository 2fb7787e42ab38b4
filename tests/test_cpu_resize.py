"""The resize front end without a GPU: detectron2's shape rule, Pillow's coefficient tables (through the numpy pass of tests/resize_ref.py)
against the stored Pillow outputs (tests/golden/make_golden_resize.py), the C ABI's argument checks, and the Predictor's host side."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import resize_ref
from .helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cmk_resize_ksize", "cmk_resize_h_u8", "cmk_resize_v_u8", "cmk_resize_v_preprocess")


@pytest.fixture(scope="module")
def fixture():
    return golden("resize_pil")


def test_shape_rule_matches_the_fixture_list(fixture):
    from centermask2_amd import ops
    want = [(48, 64, 80, 133, 80, 107), (64, 48, 80, 133, 107, 80), (30, 100, 80, 133, 40, 133), (427, 640, 800, 1333, 800, 1199),
            (480, 640, 800, 1333, 800, 1067), (4, 6, 3, 100, 3, 5)]
    assert [tuple(c) for c in fixture["shape_rule"]] == want
    for h, w, short, max_size, new_h, new_w in want:
        assert ops.resize_shortest_edge_shape(h, w, short, max_size) == (new_h, new_w), (h, w, short, max_size)
    for case, (h, w, short, max_size, new_h, new_w) in zip(fixture["rule_images"], want):
        assert tuple(case["size"]) == (h, w, new_h, new_w) and tuple(case["src"].shape) == (h, w, 3) and tuple(case["out"].shape) == (new_h, new_w, 3)
    assert len(fixture["rule_images"]) == 3


def test_fixture_holds_the_op_level_cases(fixture):
    assert [tuple(c["size"]) for c in fixture["ops"]] == [(37, 53, 61, 87), (97, 41, 33, 14), (230, 40, 31, 5), (40, 60, 90, 40), (50, 70, 50, 91),
                                                         (70, 50, 91, 50), (64, 64, 64, 64), (9, 300, 27, 900)]
    for c in fixture["ops"]:
        h, w, new_h, new_w = c["size"]
        assert c["src"].dtype == c["out"].dtype == torch.uint8 and tuple(c["src"].shape) == (h, w, 3) and tuple(c["out"].shape) == (new_h, new_w, 3)
    both_skipped = fixture["ops"][6]
    assert torch.equal(both_skipped["src"], both_skipped["out"])


def test_coefficient_tables_have_pillows_shape():
    from centermask2_amd import ops
    for in_size, out_size, ksize in ((53, 87, 3), (41, 14, 7), (230, 31, 17), (64, 64, 3), (640, 1067, 3), (1600, 1067, 5)):
        bounds, kk, ks = ops.resize_coeffs(in_size, out_size)
        assert ks == ksize and bounds.shape == (out_size, 2) and kk.shape == (out_size, ksize) and bounds.dtype == kk.dtype == np.int32
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= in_size).all()
        assert (kk >= 0).all() and (np.abs(kk.sum(axis=1, dtype=np.int64) - (1 << 22)) <= ksize).all()      # each weight rounded once
        assert 255 * ((1 << 22) + ksize) + (1 << 21) < 2 ** 31                                               # int32 accumulator
    with pytest.raises(ops._lib.CmkError):
        ops.resize_coeffs(0, 5)


def test_numpy_pass_on_the_tables_reproduces_every_fixture_image(fixture):
    for c in fixture["ops"] + fixture["rule_images"]:
        h, w, new_h, new_w = c["size"]
        got = resize_ref.resize_bilinear_u8(c["src"].numpy(), new_h, new_w)
        assert got.dtype == np.uint8 and np.array_equal(got, c["out"].numpy()), (tuple(c["size"]), int((got != c["out"].numpy()).sum()))


def test_numpy_pass_equals_pillow_on_a_coco_sized_pair():
    Image = pytest.importorskip("PIL.Image")
    src = np.random.default_rng(7).integers(0, 256, size=(480, 640, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(src).resize((1067, 800), Image.BILINEAR))
    assert np.array_equal(resize_ref.resize_bilinear_u8(src, 800, 1067), want)


def test_resize_entries_are_declared_and_refuse_bad_arguments_without_gpu():
    from centermask2_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "cmk.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
    assert all(hasattr(ops, n) for n in ("resize_shortest_edge_shape", "resize_bilinear_u8", "resize_preprocess_images"))
    lib = _lib.load()
    assert lib.cmk_version() == 5
    assert [lib.cmk_resize_ksize(i, o) for i, o in ((53, 87), (41, 14), (230, 31), (64, 64), (0, 4), (4, 0))] == [3, 7, 17, 3, 0, 0]
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    m3 = (ctypes.c_float * 3)(1.0, 2.0, 3.0)

    def hpass(src=p, h=4, w=8, new_w=16, bounds=p, kk=p, ksize=3, dst=p):
        return lib.cmk_resize_h_u8(src, h, w, new_w, bounds, kk, ksize, dst, None), lib.cmk_last_error()

    def vpass(src=p, h=4, new_h=8, new_w=16, bounds=p, kk=p, ksize=3, dst=p):
        return lib.cmk_resize_v_u8(src, h, new_h, new_w, bounds, kk, ksize, dst, None), lib.cmk_last_error()

    def vprep(src=p, h=4, new_h=8, new_w=16, bounds=p, kk=p, ksize=3, dst=p, H=8, W=16, mean=m3, std=m3):
        return lib.cmk_resize_v_preprocess(src, h, new_h, new_w, bounds, kk, ksize, dst, H, W, mean, std, 0, None), lib.cmk_last_error()

    for call, kws in ((hpass, (dict(src=None), dict(dst=None), dict(bounds=None), dict(kk=None))),
                      (vpass, (dict(src=None), dict(dst=None), dict(bounds=None), dict(kk=None))),
                      (vprep, (dict(src=None), dict(dst=None), dict(bounds=None), dict(kk=None), dict(mean=None), dict(std=None)))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == -1 and b"null pointer" in msg, (call.__name__, kw, msg)
    for call, kws in ((hpass, (dict(h=0), dict(w=0), dict(new_w=0))), (vpass, (dict(h=0), dict(new_h=0), dict(new_w=-1))),
                      (vprep, (dict(h=0), dict(new_h=0), dict(new_w=0)))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == -1 and b"empty image" in msg, (call.__name__, kw, msg)
    for kw in (dict(H=7), dict(W=15)):
        rc, msg = vprep(**kw)
        assert rc == -1 and b"padded size smaller" in msg, (kw, msg)
    for call, kws in ((hpass, (dict(ksize=5), dict(ksize=0), dict(w=41, new_w=14))),            # 41 -> 14 needs ksize 7
                      (vpass, (dict(ksize=5), dict(h=97, new_h=33), dict(h=8, ksize=0), dict(bounds=None, kk=None, ksize=0))),
                      (vprep, (dict(ksize=1), dict(h=97, new_h=33, H=33), dict(h=8, bounds=None, kk=None, ksize=3)))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == -1 and (b"ksize" in msg or b"null pointer" in msg), (call.__name__, kw, msg)
    rc, msg = hpass(dst=p + 2)
    assert rc == -1 and b"4-byte aligned" in msg, msg
    rc, msg = vprep(H=70000, new_h=70000, h=70000, bounds=None, kk=None, ksize=0)
    assert rc == -1 and b"65535" in msg, msg


def test_float_and_four_channel_images_are_refused():
    from centermask2_amd import ops
    from centermask2_amd._lib import CmkError
    mean, std = (103.53, 116.28, 123.675), (1.0, 1.0, 1.0)
    for bad in (torch.zeros((8, 8, 3), dtype=torch.float32), torch.zeros((8, 8, 4), dtype=torch.uint8), torch.zeros((3, 8, 8), dtype=torch.uint8),
                torch.zeros((8, 8), dtype=torch.uint8), np.zeros((8, 8, 3), dtype=np.uint8)):
        with pytest.raises(CmkError, match="uint8"):
            ops.resize_preprocess_images([bad], 16, 32, mean, std)
        with pytest.raises(CmkError, match="uint8"):
            ops.resize_bilinear_u8(bad, 16, 16)
    with pytest.raises(CmkError, match="no CPU fallback"):          # the right kind of image, but not on a GPU
        ops.resize_preprocess_images([torch.zeros((8, 8, 3), dtype=torch.uint8)], 16, 32, mean, std)
    with pytest.raises(CmkError):
        ops.resize_preprocess_images([], 16, 32, mean, std)


def _cpu_cfg(extra=()):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(extra))
    return cfg


def test_predictor_builds_on_cpu_and_refuses_what_it_cannot_resize():
    import centermask2_amd
    from centermask2_amd import Predictor, load_weights, predictor
    from centermask2_amd._lib import CmkError
    from centermask2_amd.modeling import GeneralizedRCNN
    assert Predictor is predictor.Predictor and load_weights is predictor.load_weights and "Predictor" in centermask2_amd.__all__
    pred = Predictor(_cpu_cfg(["INPUT.MIN_SIZE_TEST", 256, "INPUT.MAX_SIZE_TEST", 400]))
    assert isinstance(pred.model, GeneralizedRCNN) and not pred.model.training
    assert (pred.min_size, pred.max_size, pred.input_format) == (256, 400, "BGR")
    keep = pred.model.train()
    assert Predictor(_cpu_cfg(), model=keep).model is keep and not keep.training
    assert (Predictor(_cpu_cfg(), model=keep).min_size, Predictor(_cpu_cfg(), model=keep).max_size) == (800, 1333)
    for bad in (np.zeros((8, 8, 3), dtype=np.float32), torch.zeros((8, 8, 4), dtype=torch.uint8), [[1, 2, 3]]):
        with pytest.raises(CmkError):
            pred(bad)
    with pytest.raises(CmkError, match="no CPU fallback"):          # a well-formed image reaches the device check of the resize
        pred(np.zeros((8, 8, 3), dtype=np.uint8))


def test_load_weights_round_trips_both_checkpoint_forms(tmp_path):
    from centermask2_amd import Predictor, load_weights, synthetic as S
    sd = S.make_synthetic_state_dict("V-39-eSE", 3)
    plain, wrapped = str(tmp_path / "plain.pth"), str(tmp_path / "wrapped.pth")
    torch.save(sd, plain)
    torch.save({"model": sd, "iteration": 7}, wrapped)
    pred = Predictor(_cpu_cfg(["MODEL.WEIGHTS", wrapped]))          # cfg.MODEL.WEIGHTS goes through load_weights
    model = pred.model
    got = model.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with torch.no_grad():
        for v in model.parameters():
            v.zero_()
    assert load_weights(model, plain) is model
    got = model.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    small = torch.nn.Linear(2, 2)                                   # strict keys, and only the two checkpoint forms
    torch.save({"weight": torch.ones(2, 2)}, plain)
    with pytest.raises(RuntimeError, match="bias"):
        load_weights(small, plain)
    torch.save({"model": {"weight": torch.ones(2, 2), "bias": torch.ones(2), "extra": torch.ones(1)}}, plain)
    with pytest.raises(RuntimeError, match="extra"):
        load_weights(small, plain)
    torch.save([1, 2, 3], plain)
    with pytest.raises(RuntimeError, match="neither"):
        load_weights(small, plain)
