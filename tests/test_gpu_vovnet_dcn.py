"""-m gpu: VoVNet with deformable stages (MODEL.VOVNET.STAGE_WITH_DCN) against the reference's own VoVNet/FPN
(tests/golden/vovnet_dcn.pt, tests/golden/make_golden_dcn.py), and a full model with DCN in stages 3-5 end to end."""
import pytest
import torch

from centermask2_amd import synthetic as S
from tests.helpers import close_abs, golden

pytestmark = pytest.mark.gpu

CASES = ["v39_v1_dg1", "v39_mod_dg2", "v19slim_mod_dg2", "v19slimdw_flags"]


def _build(body, flags, modulated, dg, plain=False):
    """plain: offset convs zeroed and mask logits at +40 (mask 1), i.e. the same network with undeformed 3x3 convs."""
    from centermask2_amd.config import config_path, get_cfg
    from centermask2_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "MODEL.VOVNET.CONV_BODY", body, "MODEL.VOVNET.STAGE_WITH_DCN", tuple(flags),
                         "MODEL.VOVNET.WITH_MODULATED_DCN", modulated, "MODEL.VOVNET.DEFORMABLE_GROUPS", dg])
    cfg.freeze()
    sd = S.make_synthetic_state_dict(body, 0, stage_with_dcn=tuple(flags), with_modulated_dcn=modulated, deformable_groups=dg)
    if plain:
        for k, v in sd.items():
            if "/conv_offset." in k:
                z = torch.zeros_like(v)
                if modulated and k.endswith(".bias"):
                    z[18 * dg:] = 40.0
                sd[k] = z
    model = build_model(cfg).eval()
    model.load_state_dict(sd)
    return model


def _outputs(m, x, x32, dev):
    bu = m.backbone.bottom_up(x.to(dev))
    p = m.backbone(x32.to(dev))
    torch.cuda.synchronize()
    got = {k: bu[k].cpu() for k in ("stage3", "stage4", "stage5")}
    got.update({k: p[k].cpu() for k in ("p3", "p4", "p5", "p6", "p7")})
    return got


@pytest.mark.parametrize("case", CASES[:3])
def test_dcn_backbone_matches_reference(dev, case):
    G = golden("vovnet_dcn")
    g = G[case]
    flags = tuple(bool(f) for f in g["stage_with_dcn"].tolist())
    args = (g["body"], flags, bool(g["modulated"]), int(g["dg"]))
    got = _outputs(_build(*args), G["x"], G["x32"], dev)
    plain = _outputs(_build(*args, plain=True), G["x"], G["x32"], dev)
    for k, ref in g["out"].items():
        assert tuple(got[k].shape) == tuple(ref.shape), (k, tuple(got[k].shape), tuple(ref.shape))
        close_abs(got[k], ref, 1e-3, "dcn {} {}".format(case, k))
        # the deformation is not trivial: the same network with zero offsets and unit mask is far from the reference's output
        assert (plain[k] - ref).abs().max().item() > 0.05, (case, k)


def test_dw_body_with_dcn_flags_matches_plain_reference(dev):
    """The depth-wise body ignores the DCN flags (vovnet.py:292-298): it reproduces the reference's plain dw body (vovnet_bodies.pt)."""
    g = golden("vovnet_dcn")["v19slimdw_flags"]
    ref = golden("vovnet_bodies")["V-19-slim-dw-eSE"]
    got = _outputs(_build(g["body"], (True,) * 4, bool(g["modulated"]), int(g["dg"])), ref["x"], ref["x32"], dev)
    for k in ("stage3", "stage4", "stage5", "p3", "p4", "p5", "p6", "p7"):
        close_abs(got[k], ref[k], 1e-3, "dcn flags on dw body " + k)


def test_full_model_with_dcn_runs_end_to_end(dev):
    from centermask2_amd.structures import FakeImageList
    m = _build("V-39-eSE", (False, True, True, True), True, 2)
    x = S.make_synthetic_images(2, 256, 320, seed0=4321).to(dev)
    res = m.inference(FakeImageList(x, [(256, 320), (256, 320)]), do_preprocess=False, do_postprocess=False)
    torch.cuda.synchronize()
    assert len(res) == 2 and sum(len(r) for r in res) > 0
    for r in res:
        for t in (r.pred_boxes.tensor, r.scores, r.pred_masks, r.mask_scores):
            assert torch.isfinite(t).all()
