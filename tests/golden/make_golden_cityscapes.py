"""Writes tests/golden/cityscapes/label16_{a,b}.png: two small 16-bit greyscale label images saved ONCE by Pillow, which
tests/test_cpu_cityscapes_eval.py reads back with cityscapes_eval.read_label_png and compares with label_image(k) below.  The tests need
the files and this module's label_image only, never Pillow.

    python -m tests.golden.make_golden_cityscapes"""
import os

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cityscapes")
FILES = ("label16_a.png", "label16_b.png")


def label_image(k):
    """k = 0: a 40x56 scene in *_gtFine_instanceIds values (flat regions, the shape Cityscapes files have).  k = 1: 37x53 of noise over the
    whole 16-bit range, both bytes of a sample busy and an odd row length."""
    if k == 0:
        g = np.full((40, 56), 7, dtype=np.uint16)
        g[30:, :] = 1
        g[4:16, 3:17] = 26001
        g[6:20, 22:30] = 26002
        g[10:28, 36:44] = 24000
        g[12:22, 46:55] = 33001
        g[0:3, :] = 23
        g[20:26, 5:20] = 26
        return g
    return np.random.RandomState(20260).randint(0, 65536, size=(37, 53)).astype(np.uint16)


def main():
    from PIL import Image
    os.makedirs(HERE, exist_ok=True)
    for k, name in enumerate(FILES):
        Image.fromarray(label_image(k)).save(os.path.join(HERE, name))
        back = np.asarray(Image.open(os.path.join(HERE, name)))
        assert np.array_equal(back, label_image(k)), name
        print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main()
