"""Golden vectors for the MobileNetV2 backbone (mobilenet.py) and the CenterMask-Lite model built on it, from the REFERENCE's own modules.

    python tests/golden/make_golden_mnv2.py      # needs the reference tree; writes state_dict_keys_Mv2.txt, mnv2_backbone.pt, e2e_mnv2_lite.pt

The three builders of mobilenet.py:147-215 run on the synthetic weights of centermask2_amd/synthetic.py ("MobileNetV2"); FPN, the top blocks
and the d2 layers enter through tests/golden/d2_stub.py as for the VoVNet fixtures ("parity unpinned" against a real detectron2; the
MobileNetV2 body, the builders, FCOS and CenterROIHeads are the reference's).  The Lite recipe is the package's yaml (the reference tree
has none), merged into the reference's own config.  Written:
  * state_dict_keys_Mv2.txt: '# <builder>' then that builder's state-dict keys, in order;
  * mnv2_backbone.pt: res2..res5 of the bare body on a 2x3x64x96 batch and an odd 1x3x75x109 image; the p-levels of the FPN builders on
    the 64x96 batch (FCOS TOP_LEVELS 2 and 1 over res3..res5; LastLevelMaxPool over res2..res5, which exercises the 24-channel lateral);
    the inputs are regenerated from the stored seeds; `clamp_shares` (sites, 2): the share of values above 6 and below 0 entering each of the 34 ReLU6 sites, per input;
  * e2e_mnv2_lite.pt: two images through backbone -> FCOS -> CenterROIHeads at the Lite widths, in the form of e2e_800x1280.pt.
Data only.  Asserted before writing: every site's upper-clamp share in [0.001, 0.5] (both clamps of every fused kernel launch are
exercised), 5..POST_NMS_TOPK_TEST detections per e2e image, every fixture under 2 MB.
"""
import os
import sys
from collections import OrderedDict

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the d2 stand-ins and imports the reference package)

S = G.S
from detectron2.modeling.backbone.build import BACKBONE_REGISTRY  # noqa: E402  (stub registry, filled by the reference)
from centermask2_amd.structures import ShapeSpec  # noqa: E402

LITE = dict(fpn_ch=128, mask_dim=128, num_tower_convs=2, mask_num_conv=2, maskiou_num_conv=2)
E2E_HW, E2E_SEED0 = (608, 1024), 1234
SMALL_SEED0, ODD_SEED0 = 91, 77
ALL = ["res2", "res3", "res4", "res5"]


def ref_cfg(*pairs):
    cfg = G.ref_get_cfg()
    cfg.merge_from_file(G.config_path("centermask_lite_Mv2_FPN_ms_4x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(pairs))
    cfg.freeze()
    return cfg


def build_backbone(name, *pairs):
    cfg = ref_cfg("MODEL.BACKBONE.NAME", name, *pairs)
    return cfg, BACKBONE_REGISTRY.get(name)(cfg, ShapeSpec(channels=3)).eval()


def load_backbone(backbone, fpn_in, top_levels, bare=False):
    shapes = S.model_param_shapes(S.MOBILENETV2, fpn_in=fpn_in, top_levels=top_levels, **LITE)
    sd = S.make_synthetic_state_dict(S.MOBILENETV2, 0, shapes=shapes)
    prefix = "backbone.bottom_up." if bare else "backbone."
    sub = OrderedDict((k[len(prefix):], v) for k, v in sd.items() if k.startswith(prefix))
    missing, unexpected = backbone.load_state_dict(sub, strict=True)
    assert not missing and not unexpected
    return sd


class ClampShares(object):
    """Share of the values entering each nn.ReLU6 (in module order) that its upper / lower clamp changes."""

    def __init__(self, body):
        self.sites = [m for m in body.modules() if isinstance(m, nn.ReLU6)]
        self.rows = []
        self.handles = [m.register_forward_pre_hook(self._hook) for m in self.sites]

    def _hook(self, module, inputs):
        x = inputs[0]
        self.rows.append([float((x > 6).float().mean()), float((x < 0).float().mean())])

    def take(self):
        rows, self.rows = torch.tensor(self.rows), []
        assert rows.shape == (len(self.sites), 2)
        return rows

    def remove(self):
        for h in self.handles:
            h.remove()


def main():
    out, keys = {}, OrderedDict()
    x_small = S.make_synthetic_images(2, 64, 96, seed0=SMALL_SEED0)
    x_odd = S.make_synthetic_images(1, 75, 109, seed0=ODD_SEED0)
    with torch.no_grad():
        # ---- the bare body ------------------------------------------------------------------------------------------
        _, body = build_backbone("build_mnv2_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL)
        load_backbone(body, ALL, 0, bare=True)
        keys["build_mnv2_backbone"] = list(body.state_dict().keys())
        shp = body.output_shape()
        assert [shp[k].channels for k in ALL] == [24, 32, 96, 320] and [shp[k].stride for k in ALL] == [4, 8, 16, 32]
        bb = dict(image_seed0=torch.tensor(SMALL_SEED0), image_seed0_odd=torch.tensor(ODD_SEED0))     # S.make_synthetic_images(2, 64, 96) / (1, 75, 109)
        for tag, x in (("", x_small), ("_odd", x_odd)):
            ref = body(x)
            ref64 = body.double()(x.double())
            body.float()
            for k in ALL:
                bb[k + tag] = ref[k].clone()
                print("body" + tag, k, tuple(ref[k].shape), "absmax %.3f" % float(ref[k].abs().max()),
                      "fp32 vs fp64 %.2e" % float((ref[k].double() - ref64[k]).abs().max()))
        probe = ClampShares(body)
        assert len(probe.sites) == 34
        for tag, x in (("", x_small), ("_odd", x_odd)):
            body(x)
            shares = probe.take()
            bb["clamp_shares" + tag] = shares
            print("clamp shares" + tag, "upper %.4f..%.4f" % (float(shares[:, 0].min()), float(shares[:, 0].max())),
                  "lower %.3f..%.3f" % (float(shares[:, 1].min()), float(shares[:, 1].max())))
            assert float(shares[:, 0].min()) >= 0.001 and float(shares[:, 0].max()) <= 0.5, shares[:, 0]
        probe.remove()

        # ---- the three FPN builders on the 64x96 batch ---------------------------------------------------------------------
        cases = (("fcos_top2", "build_fcos_mobilenetv2_fpn_backbone", ALL[1:], 2, ["p3", "p4", "p5", "p6", "p7"]),
                 ("fcos_top1", "build_fcos_mobilenetv2_fpn_backbone", ALL[1:], 1, ["p3", "p4", "p5", "p6"]),
                 ("maxpool", "build_mobilenetv2_fpn_backbone", ALL, 0, ["p2", "p3", "p4", "p5", "p6"]))
        for tag, name, fpn_in, top, levels in cases:
            _, backbone = build_backbone(name, "MODEL.RESNETS.OUT_FEATURES", fpn_in, "MODEL.FPN.IN_FEATURES", fpn_in, "MODEL.FCOS.TOP_LEVELS", top)
            load_backbone(backbone, fpn_in, top)
            if tag != "fcos_top1":
                keys[name] = list(backbone.state_dict().keys())
            ref = backbone(x_small)
            assert list(ref.keys()) == levels and backbone.size_divisibility == 32, (list(ref.keys()), backbone.size_divisibility)
            if tag == "maxpool":
                assert torch.equal(ref["p6"], ref["p5"][:, :, ::2, ::2])
            bb[tag] = {k: v.clone() for k, v in ref.items()}
            for k in bb[tag]:        # a level the first builder already produced, bit for bit, shares its storage (stored once)
                if tag != "fcos_top2" and k in bb["fcos_top2"] and torch.equal(bb[tag][k], bb["fcos_top2"][k]):
                    bb[tag][k] = bb["fcos_top2"][k]
            for k, v in ref.items():
                print(tag, k, tuple(v.shape), "absmax %.3f" % float(v.abs().max()))
        out["mnv2_backbone"] = bb

        # ---- end to end at the Lite widths ---------------------------------------------------------------------------------
        from centermask.modeling.fcos.fcos import FCOS
        from centermask.modeling.centermask.center_heads import CenterROIHeads
        cfg, backbone = build_backbone("build_fcos_mobilenetv2_fpn_backbone")
        fcos, roi_heads = FCOS(cfg, backbone.output_shape()).eval(), CenterROIHeads(cfg, backbone.output_shape()).eval()
        sd = S.make_synthetic_state_dict(S.MOBILENETV2, 0, shapes=S.model_param_shapes(S.MOBILENETV2, **LITE))
        G.load_synthetic(backbone, fcos, roi_heads, sd)
        h, w = E2E_HW
        x = S.make_synthetic_images(2, h, w, seed0=E2E_SEED0)
        sizes = [(h, w), (h, w)]
        images = G.FakeImageList(x, sizes)
        feats = backbone(x)
        props, _ = G.quiet(fcos, images, feats, None)
        results, _ = G.quiet(roi_heads, images, feats, props, None)
        e2e = dict(image_seed0=torch.tensor(E2E_SEED0), weight_seed=torch.tensor(0), image_hw=torch.tensor(E2E_HW))
        names = ("p3", "p4", "p5", "p6", "p7")
        for k in names:
            e2e[k] = G.probe(feats[k])
        rl, rr, rc, _ = fcos.fcos_head([feats[k] for k in names])
        for l in range(5):
            e2e["logits{}".format(l)] = G.probe(rl[l])
            e2e["reg{}".format(l)] = G.probe(rr[l])
            e2e["ctr{}".format(l)] = G.probe(rc[l])
        topk = cfg.MODEL.FCOS.POST_NMS_TOPK_TEST
        for i in range(2):
            r = G.inst_to_dict(results[i])
            n = r["scores"].shape[0]
            cands = int(sum(int((torch.sigmoid(t[i]) > cfg.MODEL.FCOS.INFERENCE_TH_TEST).sum()) for t in rl))
            print("e2e img", i, "cands", cands, "dets", n, "score range", float(r["scores"][-1]) if n else None, float(r["scores"][0]) if n else None)
            assert 5 <= n <= topk, "image {}: {} detections, need 5..{}".format(i, n, topk)
            e2e["img{}".format(i)] = dict(**{k: v.clone() for k, v in r.items()}, num_candidates=torch.tensor(cands))
        out["e2e_mnv2_lite"] = e2e

    with open(os.path.join(HERE, "state_dict_keys_Mv2.txt"), "w") as f:
        for name, ks in keys.items():
            f.write("# {}\n".format(name) + "\n".join(ks) + "\n")
    for name, blob in out.items():
        path = os.path.join(HERE, name + ".pt")
        torch.save(blob, path)
        size = os.path.getsize(path)
        print("wrote", path, size // 1024, "KiB")
        assert size < 2 * 1000 * 1000, "{} is {} bytes: fixtures stay under 2 MB".format(name, size)


if __name__ == "__main__":
    main()
