"""The tests' float64 restatement of the keypoint head (keypoint_head.py:219-224: conv_fcn* + ReLU, score_lowres as torch's own
conv_transpose2d) in front of tests/keypoint_ref.py, and the comparison rule the keypoint tests of the head and of the model share.

The rule, per valid (RoI, keypoint).  e is the observed max abs error of the kernel path's 28 x 28 logits against the float64 ones
(itself asserted <= 1e-3, the project's bar for logits).  The bilinear x2 is a convex combination and cannot enlarge an error; the bicubic
resize to the box can, by at most the square of its largest absolute row sum, 1.375^2 = 1.8906.  With m the maximum of the float64 resized
map, eps = 2 * 1.8906 * e + 1e-4 * max(1, |m|)  (the error may lift one pixel and lower another; the second term is the decode kernel's own
fp32 bar from tests/test_gpu_keypoint.py):
  * where m lies more than eps above every other pixel ("exact case") the kernel's pixel is that maximum and x, y are within 1e-3 px;
  * elsewhere the kernel's pixel has a float64 value >= m - eps;
  * the score, 1 / sum(exp(map56 - max)), is within 3 * 1.9 * e + 1e-5 relative (the same bound on the exponents).
detectron2's heatmaps_to_keypoints is not available offline: the expected keypoints come from keypoint_ref applied to float64 logits, so
they are unpinned against a real detectron2, like the decode kernel's own test."""
import torch
import torch.nn.functional as F

from . import keypoint_ref as KR

BICUBIC_GAIN = 1.8906


def head_state(sd, prefix="roi_heads.keypoint_head."):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def logits28(head_sd, pooled: torch.Tensor) -> torch.Tensor:
    """(M, C, S, S) pooled features -> (M, K, 2S, 2S) float64 score_lowres output."""
    x = pooled.double()
    i = 1
    while "conv_fcn{}.weight".format(i) in head_sd:
        x = F.relu(F.conv2d(x, head_sd["conv_fcn{}.weight".format(i)].double(), head_sd["conv_fcn{}.bias".format(i)].double(), padding=1))
        i += 1
    return F.conv_transpose2d(x, head_sd["score_lowres.weight"].double(), head_sd["score_lowres.bias"].double(), stride=2, padding=1)


def layers(head_sd, pooled: torch.Tensor) -> torch.Tensor:
    """The reference's `layers`: logits28 then the bilinear x2, float64, (M, K, 4S, 4S)."""
    return KR.heatmaps(logits28(head_sd, pooled))


def pack(logits: torch.Tensor) -> torch.Tensor:
    """(M, K, 2S, 2S) -> the packed (M, S, S, 4K) form, channel (2py+px)K + k: the inverse of keypoint_ref.depth_to_space."""
    m, k, s2, _ = logits.shape
    s = s2 // 2
    return logits.reshape(m, k, s, 2, s, 2).permute(0, 2, 4, 3, 5, 1).reshape(m, s, s, 4 * k)


def check_keypoints(got: torch.Tensor, ref_logits28: torch.Tensor, boxes: torch.Tensor, e: float, what=""):
    """got (M, K, 3) from the kernel path, ref_logits28 (M, K, 2S, 2S) float64, boxes (M, 4), e as in the module docstring.
    Asserts the rule; returns (pairs in the exact case, all pairs)."""
    exact = total = 0
    for r in range(got.shape[0]):
        ref = KR.decode_one(ref_logits28[r], boxes[r])
        for k, d in enumerate(ref):
            x, y, score = (float(v) for v in got[r, k])
            row, col = KR.pixel_of(x, y, boxes[r])
            eps = 2 * BICUBIC_GAIN * e + 1e-4 * max(1.0, abs(d["value"]))
            assert 0 <= row < d["map"].shape[0] and 0 <= col < d["map"].shape[1], (what, r, k, row, col)
            if d["gap"] > eps:
                assert (row, col) == (d["row"], d["col"]), (what, r, k, (row, col), (d["row"], d["col"]), d["gap"], eps)
                assert abs(x - d["xys"][0]) <= 1e-3 and abs(y - d["xys"][1]) <= 1e-3, (what, r, k, x, y, d["xys"])
                exact += 1
            else:
                assert float(d["map"][row, col]) >= d["value"] - eps, (what, r, k)
            total += 1
            assert abs(score - d["xys"][2]) <= (3 * e * 1.9 + 1e-5) * d["xys"][2], (what, r, k, score, d["xys"][2], e)
    return exact, total


def exact_share(ref_logits28: torch.Tensor, boxes: torch.Tensor, e: float):
    """The share of (RoI, keypoint) pairs in the exact case for a given e, from the float64 restatement alone."""
    exact = total = 0
    for r in range(ref_logits28.shape[0]):
        for d in KR.decode_one(ref_logits28[r], boxes[r]):
            exact += d["gap"] > 2 * BICUBIC_GAIN * e + 1e-4 * max(1.0, abs(d["value"]))
            total += 1
    return exact, total
