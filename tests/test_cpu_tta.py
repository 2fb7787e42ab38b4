"""Test-time augmentation without a GPU: the TEST.AUG defaults, the augmentation list, the properties of the numpy restatement
(tests/tta_ref.py) the kernels are held to, the C ABI's argument checks (include/cmk.h: cmk_resize_v_preprocess_hflip, cmk_tta_*), which run
before any launch, and the refusals and routing on the Python side."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from centermask2_amd import _lib, ops
from . import tta_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cmk_resize_v_preprocess_hflip", "cmk_tta_boxes_to_image", "cmk_tta_boxes_to_aug", "cmk_tta_reduce_masks")


def _cpu_cfg(extra=()):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(extra))
    return cfg


def test_aug_defaults_are_detectron2s():
    from centermask2_amd.config import get_cfg
    aug = get_cfg().TEST.AUG
    assert aug.ENABLED is False and aug.FLIP is True and aug.MAX_SIZE == 4000
    assert tuple(aug.MIN_SIZES) == (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
    assert _cpu_cfg().TEST.AUG.ENABLED is False                     # the shipped recipes leave it off


def test_augmentation_list_and_order():
    from centermask2_amd.modeling.test_time_augmentation import tta_augmentations
    want = [(400, 533, False), (400, 533, True), (1000, 1333, False), (1000, 1333, True)]
    assert tta_augmentations(480, 640, (400, 1200), 1333, True) == want == tta_ref.augmentations(480, 640, (400, 1200), 1333, True)
    assert tta_augmentations(480, 640, (400, 1200), 1333, False) == [want[0], want[2]]
    assert tta_augmentations(480, 640, (400, 400), 1333, False) == [want[0], want[0]]      # repeated shapes are not merged, as in d2


def test_restatement_round_trip_double_mirror_and_identity_reduce():
    rng = np.random.default_rng(5)
    h, w = 480, 640
    augs = tta_ref.augmentations(h, w, (400, 777, 1200), 1333, True)
    k = 64
    lo = rng.uniform(0, [w - 2, h - 2], size=(k, 2))
    box = np.concatenate([lo, lo + rng.uniform(1, [w, h], size=(k, 2))], axis=1)
    box = np.minimum(box, [w, h, w, h]).astype(np.float32)            # inside the image: the clip of to_image changes nothing
    in_aug = tta_ref.boxes_to_aug(box, k, augs, h, w)
    assert in_aug.dtype == np.float32 and in_aug.shape == (len(augs), k, 4)
    back = tta_ref.boxes_to_image(in_aug, np.zeros((len(augs), k)), np.zeros((len(augs), k), dtype=np.int64), in_aug[:, :, :2],
                                  [k] * len(augs), augs, h, w)
    assert back["box"].dtype == np.float32 and back["cls"].dtype == np.int32 and back["box"].shape == (len(augs) * k, 4)
    # four rounded operations on values up to the box's largest coordinate (in either frame, up to the ratio): 2 ulp of it
    for a, aug in enumerate(augs):
        got = back["box"][a * k:(a + 1) * k]
        ulp = np.spacing(box.max(axis=1).astype(np.float32))[:, None]
        assert (np.abs(got.astype(np.float64) - box) <= 2 * ulp).all(), aug
    # a double mirror is exact: nw - (nw - x) == x for coordinates on the fp32 grid of [0, nw] the detector emits (multiples of 2^-10 here)
    for nw in (533, 1333):
        x0 = (rng.integers(0, nw << 10, size=100) / 1024.0).astype(np.float32)
        x1 = (rng.integers(0, nw << 10, size=100) / 1024.0).astype(np.float32)
        a0, a1 = tta_ref._flip_x(nw, x0, x1)
        b0, b1 = tta_ref._flip_x(nw, a0, a1)
        assert np.array_equal(b0, x0) and np.array_equal(b1, x1)
    # A = 1, no flip: the reduce is the identity below the count and zero from it on
    m = rng.random((1, 7, 12, 12), dtype=np.float32)
    s = rng.random((1, 7), dtype=np.float32)
    rm, rs = tta_ref.reduce_masks(m, [0], s, 5)
    assert np.array_equal(rm[:5], m[0, :5]) and np.array_equal(rs[:5], s[0, :5]) and not rm[5:].any() and not rs[5:].any()
    rm, rs = tta_ref.reduce_masks(np.concatenate([m, m]), [0, 1], None, 7)
    assert rs is None and np.array_equal(rm, (m[0] + m[0][:, :, ::-1]) / np.float32(2))


def test_restatement_nms_is_classwise_greedy_and_stable():
    box = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [1, 0, 10, 10], [20, 20, 30, 30], [0, 0, 10, 10]], dtype=np.float32)
    score = np.array([0.5, 0.5, 0.9, 0.1, 0.4], dtype=np.float32)
    cls = np.array([1, 1, 1, 1, 2])
    assert tta_ref.nms(box, score, cls, 0.6, 100) == [2, 4, 3]       # 0 and 1 fall to 2 (IoU 0.9); class 2 is left alone
    assert tta_ref.nms(box, score, cls, 0.95, 100) == [2, 0, 4, 3]   # the tie 0/1 keeps the earlier candidate (IoU 1 > thr drops 1)
    assert tta_ref.nms(box, score, cls, 0.95, 2) == [2, 0]


def test_tta_entries_are_declared_and_wrapped():
    header = open(os.path.join(ROOT, "include", "cmk.h")).read()
    declared = set(re.findall(r"\b(cmk_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES)
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES, name
    assert all(hasattr(ops, n) for n in ("resize_preprocess_augmented", "tta_table", "tta_boxes_to_image", "tta_boxes_to_aug",
                                         "tta_reduce_masks"))
    import centermask2_amd
    from centermask2_amd.modeling import test_time_augmentation as T
    assert centermask2_amd.GeneralizedRCNNWithTTA is T.GeneralizedRCNNWithTTA and "GeneralizedRCNNWithTTA" in centermask2_amd.__all__
    t = ops.tta_table([(400, 533, False), (1000, 1333, True)], 480, 640, True, "cpu").numpy()
    assert t.dtype == np.float32 and np.array_equal(t, np.array([[533, 400, np.float32(640 / 533), np.float32(480 / 400), 0],
                                                                  [1333, 1000, np.float32(640 / 1333), np.float32(480 / 1000), 1]], dtype=np.float32))
    t = ops.tta_table([(400, 533, True)], 480, 640, False, "cpu").numpy()
    assert np.array_equal(t, np.array([[533, 400, np.float32(533 / 640), np.float32(400 / 480), 1]], dtype=np.float32))


def test_tta_c_abi_argument_validation_without_gpu():
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    m3 = (ctypes.c_float * 3)(1, 2, 3)

    def refused(rc, word=None):
        err = lib.cmk_last_error()
        return rc == -1 and err.strip() and (word is None or word in err)

    def hflip(src=p, h=4, new_h=8, new_w=6, bounds=p, kk=p, ksize=None, dst=p, H=8, W=8, mean=m3, std=m3):
        ksize = lib.cmk_resize_ksize(h, new_h) if ksize is None else ksize
        return lib.cmk_resize_v_preprocess_hflip(src, h, new_h, new_w, bounds, kk, ksize, dst, H, W, mean, std, 0, None)

    for name in ("src", "dst", "mean", "std", "bounds", "kk"):
        assert refused(hflip(**{name: None}), b"null"), name
    assert refused(hflip(h=0)) and refused(hflip(new_h=0)) and refused(hflip(new_w=0), b"empty")
    assert refused(hflip(H=7), b"smaller") and refused(hflip(W=5), b"smaller")
    assert refused(hflip(new_h=65536, H=65536), b"65535")
    assert refused(hflip(ksize=2), b"ksize") and refused(hflip(h=8, bounds=None, kk=None, ksize=3), b"ksize")        # the copy path: no tables, ksize 0

    def to_image(box=p, score=p, cls=p, loc=p, counts=p, table=p, A=2, K=3, w=64, h=48, cbox=p, cscore=p, ccls=p, cloc=p, ccount=p):
        return lib.cmk_tta_boxes_to_image(box, score, cls, loc, counts, table, A, K, w, h, cbox, cscore, ccls, cloc, ccount, None)

    for name in ("box", "score", "cls", "loc", "counts", "table", "cbox", "cscore", "ccls", "cloc", "ccount"):
        assert refused(to_image(**{name: None}), b"null"), name
    for bad in (dict(A=0), dict(A=-1), dict(A=4097), dict(K=0), dict(K=-5), dict(K=65536)):
        assert refused(to_image(**bad), b"need 1 <="), bad
    for bad in (dict(w=0), dict(h=0), dict(w=-3), dict(w=65536), dict(h=65536)):
        assert refused(to_image(**bad), b"image size"), bad
    assert refused(to_image(box=p + 4), b"aligned") and refused(to_image(cbox=p + 8), b"aligned")

    def to_aug(box=p, count=p, table=p, A=2, K=3, out=p, counts=p):
        return lib.cmk_tta_boxes_to_aug(box, count, table, A, K, out, counts, None)

    for name in ("box", "count", "table", "out", "counts"):
        assert refused(to_aug(**{name: None}), b"null"), name
    for bad in (dict(A=0), dict(A=4097), dict(K=0), dict(K=-1), dict(K=65536)):
        assert refused(to_aug(**bad), b"need 1 <="), bad
    assert refused(to_aug(box=p + 4), b"aligned") and refused(to_aug(out=p + 4), b"aligned")

    def reduce(masks=p, flips=p, ms=p, count=p, A=2, K=3, S=4, out=p, out_ms=p):
        return lib.cmk_tta_reduce_masks(masks, flips, ms, count, A, K, S, out, out_ms, None)

    for name in ("masks", "flips", "count", "out", "ms", "out_ms"):          # the two score pointers only go together
        assert refused(reduce(**{name: None}), b"null"), name
    for bad in (dict(A=0), dict(A=-2), dict(A=4097), dict(K=0), dict(K=-1), dict(K=65536)):
        assert refused(reduce(**bad), b"need 1 <="), bad
    for bad in (dict(S=0), dict(S=-28), dict(S=1025)):
        assert refused(reduce(**bad), b"S <= 1024"), bad


def test_ops_wrappers_refuse_host_tensors():
    with pytest.raises(_lib.CmkError, match="no CPU fallback"):
        ops.resize_preprocess_augmented(torch.zeros((8, 8, 3), dtype=torch.uint8), [(16, 16)], True, [0, 0, 0], [1, 1, 1])
    with pytest.raises(_lib.CmkError):
        ops.tta_reduce_masks(torch.zeros((2, 3, 4, 4)), torch.zeros(2, dtype=torch.int32), None, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.CmkError, match="shape"):
        ops.tta_boxes_to_aug(torch.zeros((3, 5)), torch.zeros(1, dtype=torch.int32), torch.zeros((2, 5)))


def test_tta_refusals_name_their_keys():
    from centermask2_amd import GeneralizedRCNNWithTTA, Predictor
    from centermask2_amd.modeling import build_model
    model = build_model(_cpu_cfg())
    with pytest.raises(NotImplementedError, match="MODEL.KEYPOINT_ON"):
        GeneralizedRCNNWithTTA(_cpu_cfg(["MODEL.KEYPOINT_ON", True]), model)
    with pytest.raises(NotImplementedError, match="TEST.DETECTIONS_PER_IMAGE"):
        GeneralizedRCNNWithTTA(_cpu_cfg(["TEST.DETECTIONS_PER_IMAGE", 2000]), model)
    with pytest.raises(NotImplementedError, match="TEST.DETECTIONS_PER_IMAGE"):
        Predictor(_cpu_cfg(["TEST.AUG.ENABLED", True, "TEST.DETECTIONS_PER_IMAGE", 2000]), model=model)
    tta = GeneralizedRCNNWithTTA(_cpu_cfg(["TEST.AUG.MIN_SIZES", (192, 256), "TEST.AUG.MAX_SIZE", 400]), model)
    assert (tta.min_sizes, tta.max_size, tta.flip, tta.topk) == ((192, 256), 400, True, 100)
    assert tta.nms_thresh == _cpu_cfg().MODEL.FCOS.NMS_TH           # FCOS's threshold: the merged boxes are FCOS's
    with pytest.raises(_lib.CmkError):
        tta([{"image": torch.zeros((8, 8, 3), dtype=torch.uint8)}])                          # HWC, not the mapper's CHW
    with pytest.raises(_lib.CmkError, match="no CPU fallback"):
        tta([{"image": torch.zeros((3, 8, 8), dtype=torch.uint8)}])


def test_predictor_builds_the_tta_object_only_when_enabled(monkeypatch):
    from centermask2_amd import Predictor
    from centermask2_amd.modeling import build_model, test_time_augmentation as T
    model = build_model(_cpu_cfg())
    built = []
    real = T.GeneralizedRCNNWithTTA.__init__

    def spy(self, cfg, model):
        built.append(cfg)
        real(self, cfg, model)

    monkeypatch.setattr(T.GeneralizedRCNNWithTTA, "__init__", spy)
    off = Predictor(_cpu_cfg(), model=model)
    assert off.tta is None and not built
    on = Predictor(_cpu_cfg(["TEST.AUG.ENABLED", True]), model=model)
    assert isinstance(on.tta, T.GeneralizedRCNNWithTTA) and len(built) == 1 and on.tta.model is on.model
    assert len(on.tta.min_sizes) == 9 and on.tta.max_size == 4000
