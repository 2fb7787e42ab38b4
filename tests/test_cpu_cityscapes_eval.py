"""No GPU: cityscapes_eval.py (the restatement of the Cityscapes instance-level scoring rule) and evaluation.CityscapesInstanceEvaluator
on CPU Instances: hand-worked known answers, a two-image case against the brute-force restatement on whole bitmaps
(tests/cityscapes_ref.py), the ignore rules exactly at ignore / pixelCount == t, duplicate matches, the refusals, the PNG reader, and
the argument checks of the C entry cmk_mask_label_counts, which run before any launch."""
import ctypes
import math
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import centermask2_amd
from centermask2_amd import _lib, cityscapes_eval as ce, ops
from centermask2_amd.evaluation import CityscapesInstanceEvaluator
from centermask2_amd.structures import Instances
from tests import cityscapes_ref as R
from tests.golden import make_golden_cityscapes as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAR = ce.THING_CLASSES.index("car")
H, W = 40, 60


def rect(y0, x0, y1, x1):
    m = np.zeros((H, W), dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


def scene(**regions):
    """Road everywhere, then v=(y0, x0, y1, x1) rectangles given as v26001=(..)."""
    g = np.full((H, W), 7, dtype=np.int32)
    for k, (y0, x0, y1, x1) in regions.items():
        g[y0:y1, x0:x1] = int(k[1:])
    return g


def car_ap(gt, preds, ti=0):
    """The car AP at overlap index ti of one image; preds: (confidence, mask) cars.  Through the evaluator's own path."""
    ev = CityscapesInstanceEvaluator(ground_truth={"a_0_0": gt})
    inst = Instances((H, W), pred_masks=torch.from_numpy(np.stack([m for _, m in preds])),
                     pred_classes=torch.full((len(preds),), CAR, dtype=torch.int64),
                     scores=torch.tensor([c for c, _ in preds], dtype=torch.float64))
    ev.process([{"file_name": "x/a_0_0_leftImg8bit.png"}], [{"instances": inst}])
    ap = ce.score(ev._predictions)["ap"]
    want = R.evaluate([(gt, [("car", c, m) for c, m in preds])])
    assert ev.evaluate()["segm"]["AP-car"] == pytest.approx(want["AP-car"] * 100, abs=1e-10)
    return ap[CAR, ti]


GT400 = scene(v26001=(0, 0, 20, 20))


def test_the_five_known_answers():
    exact = rect(0, 0, 20, 20)
    assert car_ap(GT400, [(0.9, exact)]) == 1.0
    assert car_ap(GT400, [(0.9, rect(20, 30, 40, 50))]) == 0.0
    # IoU exactly 0.5: a prediction of 200 px wholly inside the 400-px car, 200 / (400 + 200 - 200)
    inside = rect(0, 0, 10, 20)
    assert car_ap(GT400, [(0.9, exact), (0.8, inside)]) == 1.0
    assert car_ap(GT400, [(0.9, exact), (0.95, inside)]) == 0.25
    assert car_ap(GT400, [(0.9, exact), (0.95, inside)], ti=1) == 0.25
    void = scene(v26001=(0, 0, 20, 20), v0=(20, 30, 40, 50))
    ev = CityscapesInstanceEvaluator(ground_truth={"a_0_0": void})
    inst = Instances((H, W), pred_masks=torch.from_numpy(rect(20, 30, 40, 50)[None]), pred_classes=torch.tensor([CAR]), scores=torch.tensor([0.9]))
    ev.process([{"file_name": "a_0_0_leftImg8bit.png"}], [{"instances": inst}])
    (p,) = ev._predictions[0]["preds"]
    assert p["pixelCount"] == 400 and p["void"] == 400 and p["inter"] == {}
    trues, scores, hard, have_gt, have_pred = ce._entries(ev._predictions, 26, 0.5)
    assert len(trues) == 0 and hard == 1 and have_gt and have_pred
    assert ce.score(ev._predictions)["ap"][CAR, 0] == 0.0


def test_two_images_three_classes_against_the_brute_force_restatement():
    gt, preds = R.two_image_case()
    for with_ms in (True, False):
        ev = CityscapesInstanceEvaluator(ground_truth=gt)
        inputs = [{"file_name": "leftImg8bit/val/aachen/{}_leftImg8bit.png".format(n)} for n in R.NAMES]
        ev.process(inputs, [{"instances": R.instances_of(preds[n], with_mask_scores=with_ms)} for n in R.NAMES])
        got = ev.evaluate()["segm"]
        want = R.evaluate(R.bitmap_images(gt, preds, with_ms))
        assert set(got) == set(want)
        for k, v in want.items():
            if math.isnan(v):
                assert math.isnan(got[k]), k
            else:
                assert abs(got[k] - 100 * v) <= 1e-12 * 100, (k, got[k], v)
        assert 0 < want["AP"] < 1 and not math.isnan(want["AP-car"]) and not math.isnan(want["AP-person"]) and not math.isnan(want["AP-bicycle"])
        assert math.isnan(want["AP-truck"])
    # ranked by mask_scores when present: the two rankings differ on this case
    assert R.evaluate(R.bitmap_images(gt, preds, True))["AP"] != R.evaluate(R.bitmap_images(gt, preds, False))["AP"]
    # process order does not matter, and an image without "instances" is an empty prediction
    ev = CityscapesInstanceEvaluator(ground_truth=gt)
    ev.process(inputs[::-1], [{"instances": R.instances_of(preds[R.NAMES[1]])}, {}])
    want = R.evaluate([(gt[R.NAMES[0]], []), R.bitmap_images(gt, preds)[1]])
    assert ev.evaluate()["segm"]["AP"] == pytest.approx(100 * want["AP"], abs=1e-10)


def test_columns_and_the_host_table():
    gt, preds = R.two_image_case()
    g = gt[R.NAMES[0]]
    cols, regions = ce.columns(g)
    assert cols.dtype == np.uint16 and regions == [(26, 26, 80), (24001, 24, 120), (26001, 26, 144), (26002, 26, 144), (26003, 26, 25)]
    assert np.array_equal(cols == 0, g == 1) and np.array_equal(cols == 1, (g == 7) | (g == 29001))
    for k, (v, _, _) in enumerate(regions):
        assert np.array_equal(cols == 2 + k, g == v)
    masks = np.stack([m for *_, m in preds[R.NAMES[0]]])
    table, areas = ce.label_counts_host(masks, cols, 7)
    assert table.dtype == np.int32 and areas.dtype == np.int32 and table.shape == (len(masks), 7)
    assert np.array_equal(table.sum(1), areas) and areas.tolist() == masks.reshape(len(masks), -1).sum(1).tolist()
    short, _ = ce.label_counts_host(masks, cols, 4)                     # columns >= num_cols are counted nowhere
    assert np.array_equal(short, table[:, :4])
    big = np.full((2, 3), 70000, dtype=np.int64)                        # values above 2^16 - 1 and the sort path of columns()
    big[0, 0] = 26000 * 1000 + 5
    c2, r2 = ce.columns(big)
    assert c2.tolist() == [[1, 1, 1], [1, 1, 1]] and r2 == []
    with pytest.raises(ValueError, match="negative"):
        ce.columns(np.array([[-1, 7]]))


def fp_or_ignored(gt, mask):
    """A confident prediction beside an exact match: 0.25 when it counts as a false positive at t = 0.5, 1.0 when it is ignored."""
    ap = car_ap(gt, [(0.9, rect(0, 0, 20, 20)), (0.95, mask)])
    assert ap in (0.25, 1.0)
    return "fp" if ap == 0.25 else "ignored"


def test_void_group_and_small_regions_ignore_exactly_at_the_threshold():
    void = scene(v26001=(0, 0, 20, 20), v3=(30, 0, 40, 60))
    assert fp_or_ignored(void, rect(20, 30, 40, 40)) == "fp"                           # 100 of 200 on void: 0.5 <= 0.5
    m = rect(20, 30, 40, 40); m[29, 30] = False; m[19, 30] = True                      # still 200 px
    assert fp_or_ignored(void, m) == "fp"
    m = rect(20, 30, 40, 40); m[20, 30] = False; m[30, 45] = True                      # 101 of 200 on void
    assert fp_or_ignored(void, m) == "ignored"
    assert car_ap(void, [(0.9, rect(0, 0, 20, 20)), (0.95, m)], ti=1) == 0.25         # 0.505 <= 0.55: a false positive again
    not_void = scene(v26001=(0, 0, 20, 20), v29001=(30, 0, 40, 60))                    # 29xxx is not void
    assert fp_or_ignored(not_void, m) == "fp"
    group = scene(v26001=(0, 0, 20, 20), v26=(25, 30, 40, 40))                         # a 150-px group region
    assert fp_or_ignored(group, rect(20, 30, 35, 40) | rect(20, 40, 25, 50)) == "fp"   # 100 of 200 on the group
    assert fp_or_ignored(group, rect(20, 30, 35, 40) | rect(20, 40, 25, 50) | rect(35, 30, 36, 32)) == "ignored"   # 102 of 202
    small = scene(v26001=(0, 0, 20, 20), v26002=(30, 30, 38, 40))                      # 80 px: below the minimum region size
    m = rect(30, 30, 36, 40) | rect(36, 30, 37, 31) | rect(24, 30, 30, 40) | rect(23, 30, 24, 31)   # 61 on it, 61 off
    assert m.sum() == 122 and (m & (small == 26002)).sum() == 61
    assert fp_or_ignored(small, m) == "fp"
    m2 = m.copy(); m2[23, 30] = False; m2[36, 31] = True                               # 62 on it, 60 off
    assert fp_or_ignored(small, m2) == "ignored"
    both = scene(v26001=(0, 0, 20, 20), v26=(30, 30, 35, 40))                          # a group of 50 px: counted twice
    assert fp_or_ignored(both, rect(20, 30, 35, 40) | rect(20, 40, 25, 50)) == "fp"    # 2 * 50 of 200
    assert fp_or_ignored(both, rect(20, 30, 35, 40) | rect(20, 40, 25, 50) & ~rect(20, 48, 21, 50)) == "ignored"   # 2 * 50 of 198


def test_duplicate_matches_keep_the_larger_confidence_on_the_ground_truth():
    exact = rect(0, 0, 20, 20)
    # the weaker match comes first: the region's entry must be (1, 0.9) and the extra one (0, 0.7); the other way round gives 0.25
    assert car_ap(GT400, [(0.7, exact), (0.9, exact)]) == 1.0
    assert car_ap(GT400, [(0.9, exact), (0.7, exact)]) == 1.0
    ev = CityscapesInstanceEvaluator(ground_truth={"a": GT400})
    inst = Instances((H, W), pred_masks=torch.from_numpy(np.stack([exact, exact, exact])), pred_classes=torch.full((3,), CAR),
                     scores=torch.tensor([0.5, 0.75, 0.25], dtype=torch.float64))
    ev.process([{"file_name": "a.png"}], [{"instances": inst}])
    trues, scores, hard, _, _ = ce._entries(ev._predictions, 26, 0.5)
    assert sorted(zip(scores.tolist(), trues.tolist())) == [(0.25, 0.0), (0.5, 0.0), (0.75, 1.0)] and hard == 0


def test_the_refusals(tmp_path):
    with pytest.raises(ValueError, match="not Cityscapes label names"):
        CityscapesInstanceEvaluator(ground_truth={"a": GT400}, thing_classes=["car", "lorry"])
    with pytest.raises(ValueError, match="gt_dir or ground_truth"):
        CityscapesInstanceEvaluator()
    with pytest.raises(ValueError, match="gtFine_instanceIds"):
        CityscapesInstanceEvaluator(gt_dir=str(tmp_path))
    ev = CityscapesInstanceEvaluator(ground_truth={"a_0_0": GT400, "b_0_0": GT400}, thing_classes=["car", "road"])
    one = lambda m, c=0: Instances(m.shape[1:], pred_masks=torch.from_numpy(m), pred_classes=torch.tensor([c]), scores=torch.tensor([0.5]))  # noqa: E731
    with pytest.raises(ValueError, match="no ground truth for 'c_0_0'"):
        ev.process([{"file_name": "c_0_0_leftImg8bit.png"}], [{}])
    with pytest.raises(ValueError, match="pred_masks of image 'a_0_0' are 20x60, the ground truth is 40x60"):
        ev.process([{"file_name": "a_0_0_leftImg8bit.png"}], [{"instances": one(np.ones((1, 20, 60), dtype=bool))}])
    with pytest.raises(ValueError, match="class 2"):
        ev.process([{"file_name": "a_0_0_leftImg8bit.png"}], [{"instances": one(rect(0, 0, 20, 20)[None], 2)}])
    ev.process([{"file_name": "a_0_0_leftImg8bit.png"}], [{"instances": one(rect(0, 0, 20, 20)[None], 1)}])       # "road": known, not evaluated
    assert ev._predictions[-1]["preds"] == []
    with pytest.raises(ValueError, match=r"1 ground truths were never processed, among them \['b_0_0'\]"):
        ev.evaluate()
    ev.process([{"file_name": "b_0_0_leftImg8bit.png"}], [{"instances": one(rect(0, 0, 20, 20)[None], 0)}])
    res = ev.evaluate()["segm"]
    assert res["AP-car"] == pytest.approx(50.0) and res["AP50"] == pytest.approx(50.0) and math.isnan(res["AP-person"])
    assert centermask2_amd.CityscapesInstanceEvaluator is CityscapesInstanceEvaluator and "CityscapesInstanceEvaluator" in centermask2_amd.__all__
    with pytest.raises(_lib.CmkError, match="no CPU fallback"):
        ops.mask_label_counts(torch.zeros((1, 4, 4), dtype=torch.bool), np.zeros((4, 4), dtype=np.uint16), 2)


# ---------------------------------------------------------------------------------------------------------------
# the PNG reader
# ---------------------------------------------------------------------------------------------------------------
def write_png(path, img, filters, colour=0, interlace=0, depth=None):
    """A minimal PNG encoder: greyscale 8/16 bit, row y filtered with filters[y % len(filters)]."""
    h, w = img.shape
    depth = depth or img.dtype.itemsize * 8
    bpp = max(1, depth // 8)                                            # a depth below 8 only ever reaches the header check
    rows = img.astype(">u{}".format(bpp)).view(np.uint8).reshape(h, w * bpp).astype(np.int64)
    raw = bytearray()
    for y in range(h):
        ft = filters[y % len(filters)]
        cur, up = rows[y], rows[y - 1] if y else np.zeros(w * bpp, dtype=np.int64)
        a = np.concatenate([np.zeros(bpp, dtype=np.int64), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, dtype=np.int64), up[:-bpp]])
        p = a + up - c
        pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        pred = [0 * cur, a, up, (a + up) >> 1, paeth][ft] if ft < 5 else 0 * cur
        raw += bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
    chunk = lambda k, b: struct.pack(">I", len(b)) + k + b + struct.pack(">I", zlib.crc32(k + b) & 0xffffffff)  # noqa: E731
    z = zlib.compress(bytes(raw))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace)) + chunk(b"tEXt", b"k\0v")
                + chunk(b"IDAT", z[:7]) + chunk(b"IDAT", z[7:]) + chunk(b"IEND", b""))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_read_label_png_undoes_all_five_filters(tmp_path, dtype):
    rng = np.random.RandomState(5)
    img = rng.randint(0, np.iinfo(dtype).max + 1, size=(23, 31)).astype(dtype)
    img[5:12, 3:20] = 26001 % (np.iinfo(dtype).max + 1)
    for filters in ([0], [1], [2], [3], [4], [4, 3, 2, 1, 0], [3, 4]):
        p = str(tmp_path / "f{}.png".format("".join(map(str, filters))))
        write_png(p, img, filters)
        got = ce.read_label_png(p)
        assert got.dtype == dtype and np.array_equal(got, img), filters
    one = np.array([[513]], dtype=np.uint16).astype(dtype)
    write_png(str(tmp_path / "one.png"), one, [4])
    assert np.array_equal(ce.read_label_png(str(tmp_path / "one.png")), one)


def test_read_label_png_refuses_by_name(tmp_path):
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    p = str(tmp_path / "x.png")
    write_png(p, img, [0], colour=2)
    with pytest.raises(ValueError, match="colour type 2"):
        ce.read_label_png(p)
    write_png(p, img, [0], interlace=1)
    with pytest.raises(ValueError, match="interlaced"):
        ce.read_label_png(p)
    write_png(p, img, [0], depth=4)
    with pytest.raises(ValueError, match="bit depth 4"):
        ce.read_label_png(p)
    write_png(p, img, [5])
    with pytest.raises(ValueError, match="filter type 5"):
        ce.read_label_png(p)
    write_png(p, img, [0])
    data = bytearray(open(p, "rb").read())
    with open(p, "wb") as f:
        f.write(data[:-20])
    with pytest.raises(ValueError, match="truncated|IEND"):
        ce.read_label_png(p)
    data[40] ^= 1
    with open(p, "wb") as f:
        f.write(data)
    with pytest.raises(ValueError, match="CRC"):
        ce.read_label_png(p)
    with open(p, "wb") as f:
        f.write(b"GIF89a")
    with pytest.raises(ValueError, match="not a PNG"):
        ce.read_label_png(p)


def test_read_label_png_reads_the_files_pillow_wrote(tmp_path):
    for k, name in enumerate(G.FILES):
        path = os.path.join(G.HERE, name)
        assert os.path.getsize(path) < 8192
        got = ce.read_label_png(path)
        assert got.dtype == np.uint16 and np.array_equal(got, G.label_image(k)), name
    # the evaluator globs <gt_dir>/<city>/*_gtFine_instanceIds.png and reads with the default loader, or with loader=
    city = tmp_path / "gtFine" / "val" / "aachen"
    city.mkdir(parents=True)
    write_png(str(city / "aachen_000000_000019_gtFine_instanceIds.png"), G.label_image(0), [4, 1])
    seen = []
    for loader in (None, lambda p: seen.append(p) or ce.read_label_png(p)):
        ev = CityscapesInstanceEvaluator(gt_dir=str(tmp_path / "gtFine" / "val"), loader=loader)
        m = torch.from_numpy((G.label_image(0) == 26001)[None])
        ev.process([{"file_name": "/data/leftImg8bit/val/aachen/aachen_000000_000019_leftImg8bit.png"}],
                   [{"instances": Instances((40, 56), pred_masks=m, pred_classes=torch.tensor([CAR]), scores=torch.tensor([0.5]))}])
        assert ev.evaluate()["segm"]["AP-car"] == pytest.approx(50.0)     # 26001 matched, 26002 missed
    assert len(seen) == 1 and seen[0].endswith("aachen_000000_000019_gtFine_instanceIds.png")


# ---------------------------------------------------------------------------------------------------------------
# the C entry
# ---------------------------------------------------------------------------------------------------------------
def test_the_c_entry_checks_its_arguments_before_any_launch(cmk_lib):
    assert cmk_lib.cmk_version() == 5
    header = open(os.path.join(ROOT, "include", "cmk.h")).read()
    assert "#define CMK_LABEL_MAX_COLS 4096\n" in header and ops.LABEL_MAX_COLS == 4096 and ce.MAX_DEVICE_COLS == 4096
    assert "int cmk_mask_label_counts(const uint64_t* words, int N, const uint16_t* cols, int H, int W, int C, int32_t* table, void* stream);" in header
    res, args = _lib.SIGNATURES["cmk_mask_label_counts"]
    assert res is ctypes.c_int and len(args) == 8 and hasattr(ops, "mask_label_counts")
    buf = (ctypes.c_uint64 * 8)()
    a = ctypes.addressof(buf)
    f = cmk_lib.cmk_mask_label_counts
    assert f(a, 0, a, 4, 4, 2, a, None) == 0                            # N == 0: CMK_OK, no launch
    for bad, word in [((None, 1, a, 4, 4, 2, a), b"null"), ((a, 1, None, 4, 4, 2, a), b"null"), ((a, 1, a, 4, 4, 2, None), b"null"),
                      ((None, 0, a, 4, 4, 2, a), b"null"),
                      ((a, 1, a, 0, 4, 2, a), b"at least 1"), ((a, 1, a, 4, 0, 2, a), b"at least 1"), ((a, 1, a, -3, 4, 2, a), b"at least 1"),
                      ((a, 1, a, 46341, 46341, 2, a), b"int32"), ((a, 1, a, 1, 2 ** 31 - 1, 2, a), b"int32"),
                      ((a, 65536, a, 4, 4, 2, a), b"65535"), ((a, -1, a, 4, 4, 2, a), b"65535"),
                      ((a, 1, a, 4, 4, 0, a), b"columns"), ((a, 1, a, 4, 4, 4097, a), b"columns"), ((a, 0, a, 4, 4, 4097, a), b"columns")]:
        assert f(*bad, None) == -1 and word in cmk_lib.cmk_last_error(), bad
