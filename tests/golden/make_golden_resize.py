"""Golden vectors for the resize front end (csrc/resize.hip, ops.resize_bilinear_u8 / resize_preprocess_images): Pillow's own
Image.resize(BILINEAR) — what detectron2's ResizeShortestEdge + ResizeTransform.apply_image run on a uint8 image — on small seeded
random images.

    python tests/golden/make_golden_resize.py      # needs Pillow; writes tests/golden/resize_pil.pt

Per case the file holds the source, Pillow's output and the sizes; data only, the tests that read it do not import PIL.  Before
writing, the numpy restatement of tests/resize_ref.py (on the tables of ops.resize_coeffs) must equal Pillow byte for byte on every
case and on a list of further size pairs, and ops.resize_shortest_edge_shape must give the listed shapes (detectron2's
ResizeShortestEdge.get_output_shape, worked by hand from its published rule).
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from centermask2_amd import ops  # noqa: E402
from tests import resize_ref  # noqa: E402

OP_CASES = [  # (h, w, new_h, new_w)
    (37, 53, 61, 87),      # up on both axes
    (97, 41, 33, 14),      # down on both axes, ksize 7
    (230, 40, 31, 5),      # down about 7.4x, ksize 17
    (40, 60, 90, 40),      # up vertically, down horizontally
    (50, 70, 50, 91),      # vertical pass skipped
    (70, 50, 91, 50),      # horizontal pass skipped
    (64, 64, 64, 64),      # both passes skipped
    (9, 300, 27, 900),     # rows wider than one workgroup
]
RULE_CASES = [  # (h, w, short, max_size, new_h, new_w); the first RULE_IMAGES carry images
    (48, 64, 80, 133, 80, 107),
    (64, 48, 80, 133, 107, 80),
    (30, 100, 80, 133, 40, 133),       # the max_size branch
    (427, 640, 800, 1333, 800, 1199),
    (480, 640, 800, 1333, 800, 1067),
    (4, 6, 3, 100, 3, 5),              # the + 0.5 rounding
]
RULE_IMAGES = 3
EXTRA_PAIRS = [(480, 640, 800, 1067), (1200, 1600, 800, 1067), (427, 640, 800, 1199), (3000, 500, 1333, 222), (128, 160, 256, 320),
               (1, 1, 5, 7), (5, 7, 1, 1), (2, 1000, 3, 17), (333, 77, 334, 76)]      # checked against Pillow, not stored


def pil_resize(src: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    return np.asarray(Image.fromarray(src).resize((new_w, new_h), Image.BILINEAR))


def make_case(rng, h, w, new_h, new_w):
    src = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    out = pil_resize(src, new_h, new_w)
    assert out.shape == (new_h, new_w, 3) and out.dtype == np.uint8
    mine = resize_ref.resize_bilinear_u8(src, new_h, new_w)
    assert np.array_equal(mine, out), ("the numpy restatement differs from Pillow", (h, w, new_h, new_w), int((mine != out).sum()))
    return dict(src=torch.from_numpy(src.copy()), out=torch.from_numpy(out.copy()), size=(h, w, new_h, new_w))


def main():
    rng = np.random.default_rng(20240611)
    data = dict(ops=[make_case(rng, *c) for c in OP_CASES], shape_rule=[tuple(c) for c in RULE_CASES], rule_images=[])
    for h, w, short, max_size, new_h, new_w in RULE_CASES:
        assert ops.resize_shortest_edge_shape(h, w, short, max_size) == (new_h, new_w), (h, w, short, max_size)
    for h, w, short, max_size, new_h, new_w in RULE_CASES[:RULE_IMAGES]:
        data["rule_images"].append(make_case(rng, h, w, new_h, new_w))
    for c in EXTRA_PAIRS:
        make_case(rng, *c)
    path = os.path.join(HERE, "resize_pil.pt")
    torch.save(data, path)
    print("wrote {} ({} bytes), Pillow {}".format(path, os.path.getsize(path), Image.__version__))


if __name__ == "__main__":
    main()
