"""Deformable VoVNet stages without a GPU: the C ABI's argument checks, the module tree against the reference's state-dict listing
(tests/golden/vovnet_dcn.pt, written by tests/golden/make_golden_dcn.py), construction-time refusals, and a hand-derived
known-answer case for the tests' float64 restatement (tests/deform_ref.py)."""
import ctypes

import pytest
import torch

from tests.deform_ref import deform_conv3x3_ref
from tests.helpers import golden


def _cfg(body, flags, modulated=False, dg=1):
    from centermask2_amd.config import config_path, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.VOVNET.CONV_BODY", body, "MODEL.VOVNET.STAGE_WITH_DCN", tuple(flags),
                         "MODEL.VOVNET.WITH_MODULATED_DCN", modulated, "MODEL.VOVNET.DEFORMABLE_GROUPS", dg])
    cfg.freeze()
    return cfg


def _backbone_shapes(cfg):
    import centermask2_amd.modeling  # noqa: F401  registers the builders
    from centermask2_amd.registry import BACKBONE_REGISTRY
    from centermask2_amd.structures import ShapeSpec
    bb = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, ShapeSpec(channels=3))
    return {"backbone." + k: tuple(v.shape) for k, v in bb.state_dict().items()}


def test_deform_abi_argument_validation_without_gpu():
    """Each bad argument is refused before any launch, with its message."""
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(x=p, x_cs=64, x_co=0, off=p, off_cs=18, y=p + 4096, y_cs=64, y_co=0, cin=64, cout=64, dg=1, modulated=0):
        rc = lib.cmk_deform_conv3x3_nhwc(x, x_cs, x_co, off, off_cs, p, p, p, y, y_cs, y_co, 1, 4, 4, cin, cout, dg, modulated, 1, None)
        return rc, lib.cmk_last_error()

    rc, msg = call(x=None)
    assert rc == -1 and b"null" in msg
    rc, msg = call(off=None)
    assert rc == -1 and b"null" in msg
    rc, msg = call(x_cs=66)
    assert rc == -1 and b"aligned" in msg
    rc, msg = call(x_co=2)
    assert rc == -1 and b"aligned" in msg
    rc, msg = call(x=p + 4)
    assert rc == -1 and b"aligned" in msg
    rc, msg = call(cin=48, x_cs=48, dg=5)
    assert rc == -1 and b"do not divide Cin" in msg
    rc, msg = call(cin=48, x_cs=48, dg=3, off_cs=81)
    assert rc == -1 and b"not supported" in msg
    rc, msg = call(cin=80, x_cs=80, dg=4, off_cs=72)
    assert rc == -1 and b"not a multiple of 8" in msg
    rc, msg = call(cin=24, x_cs=24)
    assert rc == -1 and b"multiple of 16" in msg
    rc, msg = call(off_cs=17)
    assert rc == -1 and b"offset tensor has 17 channels, needs 18" in msg
    rc, msg = call(off_cs=53, dg=2, modulated=1)
    assert rc == -1 and b"needs 54" in msg
    rc, msg = call(y=p, y_cs=128, y_co=32)         # output slice overlapping the input slice of the same buffer
    assert rc == -1 and b"overlap" in msg
    rc, msg = call(y_co=8)
    assert rc == -1 and b"does not hold Cout" in msg


@pytest.mark.parametrize("case", ["v39_v1_dg1", "v39_mod_dg2", "v19slim_mod_dg2"])
def test_dcn_state_dict_matches_reference_listing(case):
    """Keys and shapes of the package's backbone equal those the reference's own VoVNet/FPN built for the same config."""
    g = golden("vovnet_dcn")[case]
    ref = {k: tuple(s) for k, s in zip(g["keys"], g["shapes"])}
    flags = tuple(bool(f) for f in g["stage_with_dcn"].tolist())
    ours = _backbone_shapes(_cfg(g["body"], flags, bool(g["modulated"]), int(g["dg"])))
    assert ours == ref, sorted(set(ours.items()) ^ set(ref.items()))[:8]
    assert any("/conv_offset." in k for k in ours)
    from centermask2_amd import synthetic as S
    shapes = S.model_param_shapes(g["body"], stage_with_dcn=flags, with_modulated_dcn=bool(g["modulated"]), deformable_groups=int(g["dg"]))
    assert {k: tuple(v) for k, v in shapes.items() if k.startswith("backbone.")} == ref


def test_dw_body_ignores_dcn_flags():
    """vovnet.py:292-298: the depth-wise bodies build dw_conv3x3 layers whatever the DCN flags say."""
    plain = _backbone_shapes(_cfg("V-19-slim-dw-eSE", (False,) * 4))
    flagged = _backbone_shapes(_cfg("V-19-slim-dw-eSE", (True,) * 4, True, 4))
    assert flagged == plain
    g = golden("vovnet_dcn")["v19slimdw_flags"]
    assert {k: tuple(s) for k, s in zip(g["keys"], g["shapes"])} == plain


@pytest.mark.parametrize("body,dg", [("V-39-eSE", 3), ("V-39-eSE", 8), ("V-19-slim-eSE", 4)])
def test_unsupported_deformable_groups_raise_at_construction(body, dg):
    """dg 3 / 8, and dg 4 on V-19-slim (stage 3: 80 channels, 20 per group) are refused when the model is built, not at run time."""
    with pytest.raises(NotImplementedError, match="DEFORMABLE_GROUPS"):
        _backbone_shapes(_cfg(body, (False, True, True, True), True, dg))


def test_fcos_deformable_tower_still_refused():
    import centermask2_amd.modeling  # noqa: F401
    from centermask2_amd.config import config_path, get_cfg
    from centermask2_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.FCOS.USE_DEFORMABLE", True])
    cfg.freeze()
    with pytest.raises(NotImplementedError, match="USE_DEFORMABLE"):
        build_model(cfg)


def test_restatement_known_answer():
    """Hand-derived values on a 2x2 map [[1, 2], [3, 4]] through the centre tap only (weight 1)."""
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0]]).view(1, 1, 2, 2).repeat(1, 8, 1, 1) / 8      # 8 channels summing to the map
    weight = torch.zeros(1, 8, 3, 3)
    weight[:, :, 1, 1] = 1.0
    off = torch.zeros(1, 27, 2, 2)
    off[0, 8, 0, 0], off[0, 9, 0, 0] = 0.5, 0.25          # (0.5, 0.25): .375*1 + .125*2 + .375*3 + .125*4 = 2.25
    off[0, 8, 0, 1], off[0, 9, 0, 1] = 0.0, -2.0          # (0, -1): on the boundary -> 0
    off[0, 8, 1, 0], off[0, 9, 1, 0] = 0.5, 0.0           # (1.5, 0): corner row 2 lies outside -> .5*3 = 1.5
    off[0, 8, 1, 1], off[0, 9, 1, 1] = -1.0, -1.0         # (0, 0): integer offset -> 1
    y = deform_conv3x3_ref(x, off, weight, 1, False)
    assert torch.allclose(y.view(-1), torch.tensor([2.25, 0.0, 1.5, 1.0], dtype=torch.float64), atol=1e-12)
    off[0, 18 + 4] = torch.tensor([[0.0, 100.0], [-100.0, 2.0]])        # centre-tap mask logits: .5, 1, 0, sigmoid(2)
    y = deform_conv3x3_ref(x, off, weight, 1, True)
    s2 = 1.0 / (1.0 + torch.exp(torch.tensor(-2.0, dtype=torch.float64)))
    assert torch.allclose(y.view(-1), torch.stack([torch.tensor(1.125, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64),
                                                   torch.tensor(0.0, dtype=torch.float64), s2]), atol=1e-12)
    off2 = torch.zeros(1, 36, 2, 2)                       # dg 2: group 1 (channels 4..7) shifted by +1 column at the centre tap
    off2[0, 18 + 9] = 1.0
    y = deform_conv3x3_ref(x, off2, weight, 2, False)
    # group 0 samples x itself (half the map), group 1 the right neighbour or 0 past the edge
    assert torch.allclose(y.view(-1), torch.tensor([0.5 + 1.0, 1.0 + 0.0, 1.5 + 2.0, 2.0 + 0.0], dtype=torch.float64), atol=1e-12)
