"""numpy restatement of Pillow's 8-bit separable resampling pass (Resample.c ImagingResampleHorizontal_8bpc / Vertical_8bpc) on the
tables of ops.resize_coeffs: what the HIP kernels of csrc/resize.hip must reproduce byte for byte.  tests/golden/make_golden_resize.py
checks it against Pillow itself before it writes the fixture; the GPU tests use it where no fixture image is stored."""
import numpy as np

from centermask2_amd import ops


def resample_pass(img: np.ndarray, out_size: int, axis: int) -> np.ndarray:
    """One pass over `axis` (0 = vertical, 1 = horizontal) of an (h, w, c) uint8 image; skipped when the length does not change."""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    bounds, kk, ksize = ops.resize_coeffs(in_size, out_size)
    lo, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    t = np.arange(ksize, dtype=np.int64)[None, :]
    assert (kk[t >= n[:, None]] == 0).all() and (lo >= 0).all() and (lo + n <= in_size).all() and (n <= ksize).all()
    idx = np.minimum(lo[:, None] + t, in_size - 1)                         # (out, ksize); taps past n carry weight 0
    src = np.moveaxis(img, axis, 0).astype(np.int64)                       # (in, other, c)
    acc = (1 << (ops.RESIZE_BITS - 1)) + (src[idx] * kk.astype(np.int64)[:, :, None, None]).sum(axis=1)
    assert int(acc.max()) < 2 ** 31 and int(acc.min()) >= 0              # the kernels accumulate in int32
    out = np.clip(acc >> ops.RESIZE_BITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_bilinear_u8(img: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """PIL.Image.fromarray(img).resize((new_w, new_h), BILINEAR): horizontal pass, rounded to uint8, then the vertical pass."""
    return resample_pass(resample_pass(img, new_w, 1), new_h, 0)
