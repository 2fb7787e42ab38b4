import os

import torch

GOLDEN_ROOT = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(GOLDEN_ROOT, "golden")


def golden(name):
    return torch.load(os.path.join(GOLDEN, name + ".pt"), weights_only=True)


def golden_f64():
    """The reference's outputs computed in float64 (tests/golden/make_golden_f64.py), float64 tensors nested like the fp32 fixtures
    they correct: {fixture name: {key: tensor | {index: tensor} | {key: ...}}}.  reference_f64.npz holds, per output, int8 steps from the
    fp32 fixture's value and the step, STEP * max(1, max|output|): a decoded value is within half a step (5e-8 of that scale) of the
    float64 output."""
    import numpy as np
    z = np.load(os.path.join(GOLDEN, "reference_f64.npz"))
    fixtures, out = {}, {}
    for key in z.files:
        if key.startswith("step."):
            continue
        path = key.split(".")
        if path[0] not in fixtures:
            fixtures[path[0]] = golden(path[0])
        base, node = fixtures[path[0]], out
        for p in path[:-1]:
            node = node.setdefault(int(p) if p.isdigit() else p, {})
        for p in path[1:]:
            base = base[int(p)] if isinstance(base, list) else base[p]
        last = path[-1]
        node[int(last) if last.isdigit() else last] = base.double() + torch.from_numpy(z[key]).double() * float(z["step." + key])
    return out


OBSERVED = {}      # what -> largest absolute error seen this session (printed by conftest at the end of a run: the margin on record)


def _record(what, err):
    if what:
        OBSERVED[what] = max(OBSERVED.get(what, 0.0), float(err))


def close(got, ref, tol, what=""):
    """Quantities with a natural scale (pixels, features of a single random op): max abs err <= tol * max(1, max|ref|)."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs().max().item()
    bound = tol * max(1.0, ref.abs().max().item())
    _record(what + " (rel)", err / max(1.0, ref.abs().max().item()))
    assert err <= bound, "{}: max abs err {:.3e} > {:.3e}".format(what, err, bound)
    return err


def close_abs(got, ref, tol, what=""):
    """north_star's bar for logits / regression / centerness / mask logits / scores: max ABSOLUTE error <= tol, whatever the
    magnitude of the reference (no max|ref| factor)."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs().max().item()
    _record(what + " (abs)", err)
    assert err <= tol, "{}: max abs err {:.3e} > {:.3e} (absolute)".format(what, err, tol)
    return err


def build_gpu_model(conv_body="V-39-eSE", seed=0):
    from centermask2_amd.config import get_cfg, config_path
    from centermask2_amd.modeling import build_model
    from centermask2_amd import synthetic as S
    cfg = get_cfg()
    name = "centermask_V_99_eSE_FPN_ms_3x.yaml" if conv_body == "V-99-eSE" else "centermask_V_39_eSE_FPN_ms_3x.yaml"
    cfg.merge_from_file(config_path(name))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "MODEL.VOVNET.CONV_BODY", conv_body])
    cfg.freeze()
    sd = S.make_synthetic_state_dict(conv_body, seed)
    model = build_model(cfg).eval()
    model.load_state_dict(sd)
    return model, sd


def raw_conv(x, pc, y, variant=None, relu=False, relu_upto=None, res=None, res_upsample=False, in_relu=False, in_affine=None, gn=None,
             launch=True):
    """One conv launch through the C ABI on descriptors filled as the wrappers of ops.py fill them, with the tile variant (wm, sc, wn[, splitk[,
    tail ways]]; None = the library's default) written into them as the tuner does.  x, pc, y (and in_affine): one problem, or lists of them
    for the _multi entry.  gn = (workspace, groups) of the fused GroupNorm records.  Returns (rc, descs, keep): the library's return code after
    a synchronize (None with launch=False: fill only, for tests that ask about the descriptor or change it first — cmk_conv_pool_rows and
    pool_ws — and then relaunch), the descriptors, and what they borrow pointers of (keep["ws"]: the split-K or tail workspace, or None)."""
    from centermask2_amd import _lib, ops
    xs, pcs, ys, affs = (x, pc, y, in_affine) if isinstance(x, (list, tuple)) else ([x], [pc], [y], [in_affine])
    descs = (_lib.ConvDesc * len(xs))()
    for i, d in enumerate(descs):
        ops._fill_desc(d, xs[i], pcs[i], ys[i], relu, relu_upto, res, res_upsample, in_relu, affs[i] if affs is not None else None)
        if gn is not None:
            d.gn_ws, d.gn_groups = gn[0].data_ptr(), gn[1]
    keep = {"ws": ops._set_variant(descs, len(xs), variant) if variant is not None else None, "tensors": (xs, pcs, ys, res, affs, gn)}
    return (relaunch(descs) if launch else None), descs, keep


def relaunch(descs):
    """Launch filled conv descriptors (cmk_conv2d_nhwc for one, else the _multi entry) on the current stream and wait; returns the library's code."""
    import ctypes
    from centermask2_amd import _lib, ops
    lib, n = _lib.load(), len(descs)
    rc = lib.cmk_conv2d_nhwc(ctypes.byref(descs[0]), ops._stream()) if n == 1 else lib.cmk_conv2d_nhwc_multi(descs, n, ops._stream())
    torch.cuda.synchronize()
    return rc


def load_shipped_variant_table():
    """The measured conv variant table bench.py uses (Winograd where it wins), so parity is checked on the same kernels."""
    from centermask2_amd import ops
    path = os.path.join(os.path.dirname(GOLDEN_ROOT), "centermask2_amd", "tuned", "mi355x_V-39-eSE_b8_800x1280.json")
    return ops.load_tuned(path) if os.path.exists(path) else 0


def match_detections(a_scores, a_classes, a_locations, b_scores, b_classes, b_locations, tol=1e-4):
    """perm with b[perm[i]] == a[i] as detections — identified by (class, location), which is unique after per-class NMS — or an
    AssertionError.  The two lists must hold the SAME detections; their descending-score ORDER may differ only where the scores
    are within `tol`: descending-score order is defined up to the numeric noise of the scores, and on the deep V-99 body the CPU
    oracle itself orders two detections 9e-6 apart differently on different hosts (conv reduction order depends on the CPU's
    vector width and thread count).  Everything else — which detections, their labels, their locations — is exact."""
    a_scores, b_scores = a_scores.detach().float().cpu(), b_scores.detach().float().cpu()
    a_classes, b_classes = a_classes.detach().cpu(), b_classes.detach().cpu()
    a_locations, b_locations = a_locations.detach().float().cpu(), b_locations.detach().float().cpu()
    assert a_scores.shape == b_scores.shape, (a_scores.shape, b_scores.shape)
    key = lambda c, l, k: (int(c[k]), float(l[k, 0]), float(l[k, 1]))
    where = {key(b_classes, b_locations, k): k for k in range(b_scores.shape[0])}
    assert len(where) == b_scores.shape[0], "(class, location) must identify a detection"
    perm = []
    for i in range(a_scores.shape[0]):
        k = where.get(key(a_classes, a_locations, i))
        assert k is not None, "detection {} (class {}, location {}) has no counterpart".format(i, int(a_classes[i]), a_locations[i].tolist())
        assert abs(float(b_scores[k]) - float(b_scores[i])) <= tol, \
            "detection {} sits at rank {} in the other list and the scores there differ by more than {}: a real order change".format(i, k, tol)
        perm.append(k)
    assert sorted(perm) == list(range(len(perm)))
    return torch.tensor(perm, dtype=torch.int64)
