"""not gpu: the visualizer's host side — hand-derived known answers for the NumPy restatement (tests/visualize_ref.py) the GPU tests
compare the kernels with, the font and palette data, the C ABI's argument validation, and the PNG / PPM helpers."""
import ctypes
import struct
import zlib

import numpy as np
import pytest
import torch

from . import visualize_ref as R

GREY = 100
COL0 = (242, 61, 61)            # palette[0]: hue 0, saturation 0.75, value 0.95 -> (0.95, 0.2375, 0.2375) * 255 = (242.25, 60.56, 60.56)
EDGE0 = (145, 36, 36)           # (242*154) >> 8 = 37268 >> 8, (61*154) >> 8 = 9394 >> 8
TEXT0 = (251, 196, 196)         # 242 + ((13*179) >> 8) = 242 + 9, 61 + ((194*179) >> 8) = 61 + 135


def _grey(h=6, w=8):
    return np.full((h, w, 3), GREY, dtype=np.uint8)


def test_palette_entry_and_derived_colours():
    from centermask2_amd.visualize import PALETTE_RGB
    assert PALETTE_RGB[0] == COL0
    assert R.colours(0, "RGB") == (COL0, EDGE0, TEXT0)
    assert R.colours(64, "BGR") == (COL0[::-1], EDGE0[::-1], TEXT0[::-1])                     # k mod 64; BGR swaps once


def test_restatement_fill_and_outline_by_hand():
    """6x8 grey image, one instance with a NaN box (no frame, no label), mask rows 1..3 x columns 2..5, alpha 0.5 (A = 128)."""
    mask = np.zeros((1, 6, 8), dtype=bool)
    mask[0, 1:4, 2:6] = True
    boxes = np.array([[np.nan, 1, 6, 4]], dtype=np.float32)
    out = R.render(_grey(), boxes, [0.5], [7], masks=mask, alpha=0.5, line_width=1, font_scale=1, input_format="RGB")
    fill = ((GREY * 128 + 242 * 128 + 128) >> 8, (GREY * 128 + 61 * 128 + 128) >> 8, (GREY * 128 + 61 * 128 + 128) >> 8)
    assert fill == (171, 81, 81)
    inner = {(2, 3), (2, 4)}                                       # the only set pixels whose four neighbours are all set
    for y in range(6):
        for x in range(8):
            want = (GREY,) * 3 if not mask[0, y, x] else (fill if (y, x) in inner else EDGE0)
            assert tuple(out[y, x]) == want, (y, x)
    # alpha 0 leaves the fill at the image's colour, alpha 1 at the instance's; the outline stays
    out0 = R.render(_grey(), boxes, [0.5], [7], masks=mask, alpha=0.0, line_width=1, font_scale=1, input_format="RGB")
    out1 = R.render(_grey(), boxes, [0.5], [7], masks=mask, alpha=1.0, line_width=1, font_scale=1, input_format="RGB")
    assert tuple(out0[2, 3]) == (GREY,) * 3 and tuple(out1[2, 3]) == COL0 and tuple(out0[1, 2]) == EDGE0 == tuple(out1[1, 2])
    # a mask on the border: outside the image counts as unset
    full = np.ones((1, 6, 8), dtype=bool)
    outf = R.render(_grey(), boxes, [0.5], [7], masks=full, alpha=1.0, line_width=1, font_scale=1, input_format="RGB")
    for y in range(6):
        for x in range(8):
            assert tuple(outf[y, x]) == (EDGE0 if y in (0, 5) or x in (0, 7) else COL0), (y, x)


def test_restatement_frame_plate_and_glyph_by_hand():
    """6x8 grey image, box (1, 1, 6.5, 4.2) -> rect [1,6] x [1,4], line width 1.  The label "C7 50%" makes a 37 x 9 plate, larger than the
    image: its origin clamps to (0, 0) and it darkens every pixel after the frame is drawn; 'C' sits at x 1..5, y 1..7."""
    boxes = np.array([[1, 1, 6.5, 4.2]], dtype=np.float32)
    out = R.render(_grey(), boxes, [0.5], [7], line_width=1, font_scale=1, input_format="RGB")
    assert R.label_text("C7", np.float32(0.5)) == "C7 50%"
    plate_grey = (GREY * 51 + 128) >> 8
    plate_frame = tuple((c * 51 + 128) >> 8 for c in COL0)
    assert plate_grey == 20 and plate_frame == (48, 12, 12)
    c_rows = (0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E)            # 'C': .XXX. / X...X / X.... x3 / X...X / .XXX.
    seven = (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08)             # '7' at x 7..11: only its first column (x = 7) is in the image
    for y in range(6):
        for x in range(8):
            frame = 1 <= x <= 6 and 1 <= y <= 4 and (x in (1, 6) or y in (1, 4))
            want = plate_frame if frame else (plate_grey,) * 3
            if 1 <= y <= 5 and 1 <= x <= 5 and (c_rows[y - 1] >> (4 - (x - 1))) & 1:
                want = TEXT0
            if 1 <= y <= 5 and x == 7 and (seven[y - 1] >> 4) & 1:
                want = TEXT0
            assert tuple(out[y, x]) == want, (y, x)
    # line width 2 on a larger image: the frame is two pixels thick inside the rect, and the plate starts at the box's corner
    big = R.render(_grey(30, 60), np.array([[10, 12, 50, 25]], dtype=np.float32), [0.5], [7], line_width=2, font_scale=1, input_format="RGB")
    assert tuple(big[24, 30]) == COL0 and tuple(big[25, 30]) == COL0 and tuple(big[23, 30]) == (GREY,) * 3 and tuple(big[26, 30]) == (GREY,) * 3
    assert tuple(big[18, 49]) == COL0 and tuple(big[18, 50]) == COL0 and tuple(big[18, 48]) == (GREY,) * 3 and tuple(big[18, 51]) == (GREY,) * 3
    assert tuple(big[12, 10]) == plate_frame and tuple(big[20, 46]) == (plate_grey,) * 3     # plate [10, 46] x [12, 20]
    assert tuple(big[21, 30]) == (GREY,) * 3 and tuple(big[16, 47]) == (GREY,) * 3
    # font scale 2: every font pixel a 2x2 block; 'C' row 0 column 1 -> x 10 + (1+1)*2, y 12 + 1*2
    big2 = R.render(_grey(30, 60), np.array([[10, 12, 50, 25]], dtype=np.float32), [0.5], [7], line_width=1, font_scale=2, input_format="RGB")
    assert all(tuple(big2[y, x]) == TEXT0 for y in (14, 15) for x in (14, 15)) and tuple(big2[14, 13]) != TEXT0


def test_restatement_order_later_instance_on_top():
    boxes = np.array([[0, 0, 3, 3], [0, 0, 7, 5], [np.nan, 0, 1, 1]], dtype=np.float32)
    assert R.draw_order(boxes) == [2, 1, 0]                          # NaN area first, then the larger box
    assert R.draw_order(np.array([[0, 0, 2, 2], [1, 1, 3, 3]], dtype=np.float32)) == [0, 1]   # ties by index


def test_disc_and_segment_membership():
    assert R.on_disc(3, 4, 0, 0, 5) and not R.on_disc(4, 4, 0, 0, 5)
    # horizontal (0,0) -> (10,0), width 3: 4 * dy^2 <= 9 holds for |dy| <= 1; beyond the ends the distance to the end point counts
    assert R.on_segment(5, 1, 0, 0, 10, 0, 3) and not R.on_segment(5, 2, 0, 0, 10, 0, 3)
    assert R.on_segment(-1, 0, 0, 0, 10, 0, 3) and not R.on_segment(-2, 0, 0, 0, 10, 0, 3) and R.on_segment(11, 1, 0, 0, 10, 0, 3)
    assert not R.on_segment(11, 2, 0, 0, 10, 0, 3)
    # width 1: only the line's own pixels
    assert R.on_segment(5, 0, 0, 0, 10, 0, 1) and not R.on_segment(5, 1, 0, 0, 10, 0, 1)
    # diagonal (0,0) -> (8,8), width 2: cross = 8*(x - y), 4*64*(x-y)^2 <= 4*128 iff |x - y| <= 1
    assert R.on_segment(4, 4, 0, 0, 8, 8, 2) and R.on_segment(5, 4, 0, 0, 8, 8, 2) and not R.on_segment(6, 4, 0, 0, 8, 8, 2)
    # zero length: the end test alone, 4 * d^2 <= lw^2
    assert R.on_segment(3, 3, 3, 3, 3, 3, 1) and not R.on_segment(4, 3, 3, 3, 3, 3, 1)
    assert R.on_segment(4, 3, 3, 3, 3, 3, 2) and not R.on_segment(4, 4, 3, 3, 3, 3, 2)
    # the array form the renderer uses agrees with the scalar form, far coordinates (exact path) included
    for ax, ay, bx, by, lw in ((2, 3, 17, 9, 3), (12, 1, 12, 1, 2), (-30000, -20000, 32768, 32768, 2), (5, 25, 25, 5, 1)):
        img = np.zeros((30, 30, 3), dtype=np.uint8)
        R._paint_segment(img, ax, ay, bx, by, lw, (1, 1, 1))
        for y in range(30):
            for x in range(30):
                assert bool(img[y, x, 0]) == R.on_segment(x, y, ax, ay, bx, by, lw), (ax, ay, bx, by, x, y)


def test_keypoints_by_hand():
    """One instance, K = 2: a horizontal segment of the instance's colour with red discs of radius 2 over its ends (line width 1)."""
    kp = np.array([[[2, 3, 0.9], [9, 3, 0.9]]], dtype=np.float32)
    boxes = np.array([[np.nan, 0, 1, 1]], dtype=np.float32)
    out = R.render(_grey(7, 12), boxes, [0.5], [0], keypoints=kp, skeleton=[(0, 1)], line_width=1, font_scale=1, input_format="RGB")
    for y in range(7):
        for x in range(12):
            disc = min((x - 2) ** 2, (x - 9) ** 2) + (y - 3) ** 2 <= 4
            want = (255, 0, 0) if disc else (COL0 if y == 3 and 2 <= x <= 9 else (GREY,) * 3)
            assert tuple(out[y, x]) == want, (y, x)
    # a score at the threshold, a NaN score: not visible, and a segment needs both ends
    for bad in (0.05, np.nan):
        kp2 = kp.copy()
        kp2[0, 1, 2] = bad
        out2 = R.render(_grey(7, 12), boxes, [0.5], [0], keypoints=kp2, skeleton=[(0, 1)], line_width=1, font_scale=1, input_format="RGB")
        assert tuple(out2[3, 6]) == (GREY,) * 3 and tuple(out2[3, 9]) == (GREY,) * 3 and tuple(out2[3, 2]) == (255, 0, 0)
    assert tuple(R.render(_grey(7, 12), boxes, [0.5], [0], keypoints=kp, skeleton=[(0, 1)], line_width=1, font_scale=1)[3, 2]) == (0, 0, 255)


def test_percent_rounding():
    f = np.float32
    # 0.005 is no float32: the one below it, float32(0.005) = 0.00499999988..., gives floor(0.99999998...) = 0 by the formula, the one above
    # it, 0.00500000035..., gives floor(1.00000003...) = 1: the half-way case falls where the float32 does, nothing is rounded twice
    assert float(f(0.005)) < 0.005 and R.percent(f(0.005)) == 0 and R.percent(np.nextafter(f(0.005), f(1))) == 1
    assert R.percent(f(0.015)) == 1 and R.percent(f(0.0051)) == 1
    assert R.percent(f(0.994)) == 99 and R.percent(f(0.995)) == 100 and R.percent(f(1.0)) == 100 and R.percent(f("nan")) == 0
    assert R.percent(f(0.0)) == 0 and R.percent(f(-3.0)) == 0 and R.percent(f(7.0)) == 100 and R.percent(f("inf")) == 100
    assert R.percent(f(0.5)) == 50 and R.percent(f(0.004)) == 0


def test_label_text_and_glyphs():
    from centermask2_amd.visualize import FONT_CHARS, label_glyphs
    assert R.label_text("traffic light", np.float32(0.873)) == "TRAFFIC LIGHT 87%"
    assert R.label_text("x" * 40, np.float32(0.5)) == "X" * 32 and R.label_text("a" * 29, np.float32(1.0)) == "A" * 29 + " 10"
    q = FONT_CHARS.index("?")
    assert R.glyph_indices("A_B?") == [FONT_CHARS.index("A"), q, FONT_CHARS.index("B"), q]
    assert R.glyph_indices(R.label_text("hair drier", np.float32(0.5))) == label_glyphs("hair drier 50%")        # the package's own mapping
    assert label_glyphs("é~" + "z" * 40) == [q, q] + [FONT_CHARS.index("Z")] * 30


def test_font_and_palette_tables():
    from centermask2_amd.visualize import COCO_CLASSES, COCO_PERSON_SKELETON, FONT_5X7, FONT_CHARS, PALETTE_RGB, _palette
    assert FONT_CHARS == " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ%.-?" and len(FONT_5X7) == 41 == len(set(FONT_5X7))
    for ch, g in zip(FONT_CHARS, FONT_5X7):
        assert len(g) == 7 and all(0 <= row < 32 for row in g)
        assert (sum(g) == 0) == (ch == " "), ch
    assert len(PALETTE_RGB) == 64 == len(set(PALETTE_RGB)) and all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in PALETTE_RGB)
    assert _palette() == PALETTE_RGB
    assert len(COCO_CLASSES) == 80 == len(set(COCO_CLASSES)) and COCO_CLASSES[0] == "person" and COCO_CLASSES[79] == "toothbrush"
    assert len(COCO_PERSON_SKELETON) == 19 == len(set(COCO_PERSON_SKELETON)) and all(0 <= a < 17 and 0 <= b < 17 and a != b for a, b in COCO_PERSON_SKELETON)


def test_vis_abi_argument_validation_without_gpu():
    from centermask2_amd import _lib
    lib = _lib.load()
    assert lib.cmk_vis_record_ints() >= 26 and lib.cmk_vis_record_ints() % 4 == 0
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    q = p + 2048

    def compose(img_in=p, img_out=q, h=4, w=4, words=None, rec=p, n=1, font=p, lw=1, fs=1, a=128):
        rc = lib.cmk_vis_compose(img_in, img_out, h, w, words, rec, n, font, lw, fs, a, None)
        return rc, lib.cmk_last_error()

    for kw, msg in (({"img_in": None}, b"null"), ({"img_out": None}, b"null"), ({"rec": None}, b"null"), ({"font": None}, b"null"),
                    ({"h": 0}, b"at least 1"), ({"w": -3}, b"at least 1"), ({"h": 46341, "w": 46341}, b"int32"), ({"h": 1, "w": 2 ** 31 - 1}, b"int32"),
                    ({"n": -1}, b"65535"), ({"n": 65536}, b"65535"), ({"lw": 0}, b"line_width"), ({"lw": 17}, b"line_width"),
                    ({"fs": 0}, b"font_scale"), ({"fs": 17}, b"font_scale"), ({"a": -1}, b"alpha256"), ({"a": 257}, b"alpha256"),
                    ({"img_out": p}, b"overlaps"), ({"img_out": p + 47}, b"overlaps"), ({"rec": p + 4}, b"16-byte aligned")):
        rc, err = compose(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)

    def prepare(boxes=p, scores=p, classes=p, order=p, names=p, lens=p, num_names=1, pal=p, n=1, h=4, w=4, fs=1, rec=q):
        rc = lib.cmk_vis_prepare(boxes, scores, classes, order, names, lens, num_names, pal, n, h, w, fs, 0, rec, None)
        return rc, lib.cmk_last_error()

    for kw, msg in (({"boxes": None}, b"null"), ({"scores": None}, b"null"), ({"classes": None}, b"null"), ({"order": None}, b"null"),
                    ({"names": None}, b"null"), ({"lens": None}, b"null"), ({"pal": None}, b"null"), ({"rec": None}, b"null"),
                    ({"h": 0}, b"at least 1"), ({"h": 65536, "w": 65536}, b"int32"), ({"n": -1}, b"65535"), ({"n": 65536}, b"65535"),
                    ({"fs": 0}, b"font_scale"), ({"fs": 17}, b"font_scale"), ({"num_names": -1}, b"names")):
        rc, err = prepare(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    assert prepare(n=0, boxes=None, rec=None)[0] == 0              # nothing to prepare: no launch
    assert prepare(names=None, lens=None, num_names=0, n=0)[0] == 0

    def keypoints(img=p, h=4, w=4, kps=p, rec=p, n=1, k=17, skel=p, s=19, lw=1, win=q):
        rc = lib.cmk_vis_keypoints(img, h, w, kps, rec, n, k, skel, s, 0.05, lw, 255, win, None)
        return rc, lib.cmk_last_error()

    for kw, msg in (({"img": None}, b"null"), ({"kps": None}, b"null"), ({"rec": None}, b"null"), ({"skel": None}, b"null"), ({"win": None}, b"null"),
                    ({"w": 0}, b"at least 1"), ({"h": 2 ** 16, "w": 2 ** 15}, b"int32"), ({"n": -1}, b"65535"), ({"n": 65536}, b"65535"),
                    ({"lw": 0}, b"line_width"), ({"lw": 17}, b"line_width"), ({"k": 0}, b"keypoints"), ({"k": 1025}, b"keypoints"),
                    ({"s": -1}, b"segments"), ({"s": 4097}, b"segments")):
        rc, err = keypoints(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    assert keypoints(n=0, img=None)[0] == 0


def test_cpu_inputs_are_refused():
    from centermask2_amd import Visualizer, draw_instance_predictions
    from centermask2_amd._lib import CmkError
    from centermask2_amd.structures import Boxes, Instances
    inst = Instances((6, 8), pred_boxes=Boxes(torch.tensor([[1.0, 1.0, 5.0, 4.0]])), scores=torch.tensor([0.9]), pred_classes=torch.tensor([3]))
    image = torch.full((6, 8, 3), 100, dtype=torch.uint8)
    with pytest.raises(CmkError, match=r"cpu.*\(1, 4\)"):
        Visualizer().draw(image, inst)
    with pytest.raises(CmkError, match=r"\(1, 4\)"):
        draw_instance_predictions(image.numpy(), inst, alpha=0.3)
    with pytest.raises(CmkError, match="pred_boxes"):
        Visualizer().draw(image, Instances((6, 8)))
    for kw in ({"color_by": "mask"}, {"input_format": "GRAY"}, {"alpha": 1.5}, {"alpha": float("nan")}, {"line_width": 0}, {"font_scale": 17},
               {"line_width": 1.5}):
        with pytest.raises(CmkError):
            Visualizer(**kw)


def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        out.append((tag, body))
        pos += 12 + length
    assert pos == len(data)
    return out


def test_write_png_by_hand_and_ppm_round_trip(tmp_path):
    from centermask2_amd._lib import CmkError
    from centermask2_amd.visualize import read_ppm, write_png, write_ppm
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8)       # BGR
    path = str(tmp_path / "a.png")
    write_png(path, torch.from_numpy(img))
    chunks = _chunks(open(path, "rb").read())
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", 7, 5, 8, 2, 0, 0, 0) and chunks[2][1] == b""
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(5, 1 + 21)
    assert (raw[:, 0] == 0).all() and np.array_equal(raw[:, 1:].reshape(5, 7, 3), img[:, :, ::-1])   # filter 0, RGB on disk
    write_png(path, img, input_format="RGB")
    raw = np.frombuffer(zlib.decompress(_chunks(open(path, "rb").read())[1][1]), dtype=np.uint8).reshape(5, 22)
    assert np.array_equal(raw[:, 1:].reshape(5, 7, 3), img)
    with pytest.raises(CmkError):
        write_png(path, img.astype(np.float32))
    ppm = str(tmp_path / "a.ppm")
    write_ppm(ppm, img)
    assert open(ppm, "rb").read() == b"P6\n7 5\n255\n" + img[:, :, ::-1].tobytes()
    assert np.array_equal(read_ppm(ppm), img) and np.array_equal(read_ppm(ppm, output_format="RGB"), img[:, :, ::-1])
    with open(ppm, "wb") as f:
        f.write(b"P6 # a comment\n7 5 # another\n255\n" + img.tobytes())
    assert np.array_equal(read_ppm(ppm, output_format="RGB"), img)
    with open(ppm, "wb") as f:
        f.write(b"P6\n7 5\n255\n" + img.tobytes()[:-1])
    with pytest.raises(CmkError, match="pixel bytes"):
        read_ppm(ppm)
    with open(ppm, "wb") as f:
        f.write(b"P5\n7 5\n255\n" + img.tobytes())
    with pytest.raises(CmkError, match="P6"):
        read_ppm(ppm)


def test_write_png_round_trip_through_pil(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from centermask2_amd.visualize import write_png
    img = np.random.RandomState(4).randint(0, 256, size=(9, 4, 3)).astype(np.uint8)
    path = str(tmp_path / "b.png")
    write_png(path, img)
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img[:, :, ::-1])
