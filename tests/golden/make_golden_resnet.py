"""Golden vectors for the ResNet backbones and the R-50 CenterMask model, from the REFERENCE's own builder, FCOS and CenterROIHeads.

    python tests/golden/make_golden_resnet.py      # needs the reference tree; writes state_dict_keys_R50.txt, resnet_backbone*.pt, e2e_r50.pt

The reference's build_fcos_resnet_fpn_backbone (modeling/backbone/fpn.py:56-87) looks `build_resnet_backbone` up in its module at call
time; detectron2 is absent, so that name is set to the plain-torch stand-in of tests/golden/d2_resnet_stub.py (written from d2's public
behaviour, like the FPN of d2_stub.py: "parity unpinned" against a real detectron2).  The builder, its top blocks, FCOS and
CenterROIHeads are the reference's.  The weights are centermask2_amd/synthetic.py's ("R-50", "R-101"); the recipe is the package's
centermask_R_50_FPN_ms_3x.yaml (the reference tree has none), merged into the reference's own config.  Written:
  * state_dict_keys_R50.txt: '# <builder>' then that builder's state-dict keys, in order, for the three builders at depth 50 and
    ('# build_resnet_backbone depth 101') the bare body at depth 101;
  * resnet_backbone.pt: res2..res5 of the bare R-50 on a 1x3x64x96 image, and the image seeds;
    resnet_backbone_s3x3.pt: the same image with STRIDE_IN_1X1 False;
    resnet_backbone_odd.pt (res2, res3) and resnet_backbone_fpn.pt (res4_odd, res5_odd): an odd 1x3x75x109 image;
    resnet_backbone_fpn.pt also: the p-levels of the FCOS builder (TOP_LEVELS 2) over res3..res5 and of build_resnet_fpn_backbone over
    res2..res5 on the 64x96 image.  One file would be 3.3 MB; the full tensors are kept and spread over four files;
  * e2e_r50.pt: two images through backbone -> FCOS -> CenterROIHeads in the form of e2e_mnv2_lite.pt, at the smallest size (multiples
    of 128 per side, up to 608x1024) at which every image yields 5..POST_NMS_TOPK_TEST detections; `image_hw` records it.
Data only.  Asserted before writing: 5..POST_NMS_TOPK_TEST detections per e2e image, every fixture under 1 MiB (so under 2 MB).
"""
import os
import sys
from collections import OrderedDict

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the d2 stand-ins and imports the reference package)
import d2_resnet_stub  # noqa: E402

import centermask.modeling.backbone.fpn as ref_fpn  # noqa: E402  (the reference module)
ref_fpn.build_resnet_backbone = d2_resnet_stub.build_resnet_backbone

S = G.S
from detectron2.modeling.backbone.build import BACKBONE_REGISTRY  # noqa: E402  (stub registry, filled by the reference)
from centermask2_amd.structures import ShapeSpec  # noqa: E402

SMALL_SEED0, ODD_SEED0, E2E_SEED0 = 91, 77, 1234
ALL = ["res2", "res3", "res4", "res5"]
MAX_BYTES = 1 << 20
BUILDERS = {"build_resnet_backbone": d2_resnet_stub.build_resnet_backbone, "build_resnet_fpn_backbone": d2_resnet_stub.build_resnet_fpn_backbone}


def ref_cfg(*pairs):
    cfg = G.ref_get_cfg()
    cfg.merge_from_file(G.config_path("centermask_R_50_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(pairs))
    cfg.freeze()
    return cfg


def build_backbone(name, *pairs):
    cfg = ref_cfg("MODEL.BACKBONE.NAME", name, *pairs)
    build = BUILDERS[name] if name in BUILDERS else BACKBONE_REGISTRY.get(name)      # d2's own builders: the stand-ins; the FCOS one: the reference's
    return cfg, build(cfg, ShapeSpec(channels=3)).eval()


def load_backbone(backbone, fpn_in, top_levels, bare=False, body="R-50"):
    sd = S.make_synthetic_state_dict(body, 0, shapes=S.model_param_shapes(body, fpn_in=fpn_in, top_levels=top_levels))
    prefix = "backbone.bottom_up." if bare else "backbone."
    sub = OrderedDict((k[len(prefix):], v) for k, v in sd.items() if k.startswith(prefix))
    missing, unexpected = backbone.load_state_dict(sub, strict=True)
    assert not missing and not unexpected
    return sd


def run_body(body, x, tag, store, names):
    ref = body(x)
    ref64 = body.double()(x.double())
    body.float()
    assert list(ref.keys()) == ALL
    for k in names:
        store[k + tag] = ref[k].clone()
    for k in ALL:
        print("body" + tag, k, tuple(ref[k].shape), "absmax %.3f" % float(ref[k].abs().max()), "mean %.3f" % float(ref[k].mean()),
              "zeros %.2f" % float((ref[k] == 0).float().mean()), "fp32 vs fp64 %.2e" % float((ref[k].double() - ref64[k]).abs().max()))


def e2e(hw):
    from centermask.modeling.fcos.fcos import FCOS
    from centermask.modeling.centermask.center_heads import CenterROIHeads
    cfg, backbone = build_backbone("build_fcos_resnet_fpn_backbone")
    fcos, roi_heads = FCOS(cfg, backbone.output_shape()).eval(), CenterROIHeads(cfg, backbone.output_shape()).eval()
    G.load_synthetic(backbone, fcos, roi_heads, S.make_synthetic_state_dict("R-50", 0))
    h, w = hw
    x = S.make_synthetic_images(2, h, w, seed0=E2E_SEED0)
    images = G.FakeImageList(x, [(h, w), (h, w)])
    feats = backbone(x)
    props, _ = G.quiet(fcos, images, feats, None)
    results, _ = G.quiet(roi_heads, images, feats, props, None)
    blob = dict(image_seed0=torch.tensor(E2E_SEED0), weight_seed=torch.tensor(0), image_hw=torch.tensor(hw))
    names = ("p3", "p4", "p5", "p6", "p7")
    for k in names:
        blob[k] = G.probe(feats[k])
    rl, rr, rc, _ = fcos.fcos_head([feats[k] for k in names])
    for l in range(5):
        blob["logits{}".format(l)] = G.probe(rl[l])
        blob["reg{}".format(l)] = G.probe(rr[l])
        blob["ctr{}".format(l)] = G.probe(rc[l])
    topk = cfg.MODEL.FCOS.POST_NMS_TOPK_TEST
    counts = []
    for i in range(2):
        r = G.inst_to_dict(results[i])
        n = r["scores"].shape[0]
        cands = int(sum(int((torch.sigmoid(t[i]) > cfg.MODEL.FCOS.INFERENCE_TH_TEST).sum()) for t in rl))
        print("e2e", hw, "img", i, "cands", cands, "dets", n, "score range", float(r["scores"][-1]) if n else None, float(r["scores"][0]) if n else None)
        counts.append(n)
        blob["img{}".format(i)] = dict(**{k: v.clone() for k, v in r.items()}, num_candidates=torch.tensor(cands))
    return blob, all(5 <= n <= topk for n in counts), topk


def main():
    out, keys = {}, OrderedDict()
    x_small = S.make_synthetic_images(1, 64, 96, seed0=SMALL_SEED0)
    x_odd = S.make_synthetic_images(1, 75, 109, seed0=ODD_SEED0)
    with torch.no_grad():
        # ---- the bare body ------------------------------------------------------------------------------------------
        _, body = build_backbone("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL)
        load_backbone(body, ALL, 0, bare=True)
        keys["build_resnet_backbone"] = list(body.state_dict().keys())
        shp = body.output_shape()
        assert [shp[k].channels for k in ALL] == [256, 512, 1024, 2048] and [shp[k].stride for k in ALL] == [4, 8, 16, 32]
        bb = dict(image_seed0=torch.tensor(SMALL_SEED0), image_seed0_odd=torch.tensor(ODD_SEED0))   # S.make_synthetic_images(1, 64, 96) / (1, 75, 109)
        odd, fpn = {}, {}
        run_body(body, x_small, "", bb, ALL)
        run_body(body, x_odd, "_odd", odd, ALL[:2])
        run_body(body, x_odd, "_odd", fpn, ALL[2:])
        _, body3 = build_backbone("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.RESNETS.STRIDE_IN_1X1", False)
        load_backbone(body3, ALL, 0, bare=True)
        s3 = {}
        run_body(body3, x_small, "", s3, ALL)
        assert not torch.equal(s3["res3"], bb["res3"])
        _, body101 = build_backbone("build_resnet_backbone", "MODEL.RESNETS.OUT_FEATURES", ALL, "MODEL.RESNETS.DEPTH", 101)
        load_backbone(body101, ALL, 0, bare=True, body="R-101")
        keys["build_resnet_backbone depth 101"] = list(body101.state_dict().keys())
        run_body(body101, x_small, " R-101", {}, [])

        # ---- the two FPN builders on the 64x96 image ---------------------------------------------------------------------
        cases = (("fcos_top2", "build_fcos_resnet_fpn_backbone", ALL[1:], 2, ["p3", "p4", "p5", "p6", "p7"]),
                 ("maxpool", "build_resnet_fpn_backbone", ALL, 0, ["p2", "p3", "p4", "p5", "p6"]))
        for tag, name, fpn_in, top, levels in cases:
            _, backbone = build_backbone(name, "MODEL.RESNETS.OUT_FEATURES", fpn_in, "MODEL.FPN.IN_FEATURES", fpn_in, "MODEL.FCOS.TOP_LEVELS", top)
            load_backbone(backbone, fpn_in, top)
            keys[name] = list(backbone.state_dict().keys())
            ref = backbone(x_small)
            assert list(ref.keys()) == levels and backbone.size_divisibility == 32, (list(ref.keys()), backbone.size_divisibility)
            if tag == "maxpool":
                assert torch.equal(ref["p6"], ref["p5"][:, :, ::2, ::2])
            fpn[tag] = {k: v.clone() for k, v in ref.items()}
            for k, v in ref.items():
                print(tag, k, tuple(v.shape), "absmax %.3f" % float(v.abs().max()))
        out.update(resnet_backbone=bb, resnet_backbone_s3x3=s3, resnet_backbone_odd=odd, resnet_backbone_fpn=fpn)

        # ---- end to end: the smallest size that yields detections on both images --------------------------------------------------
        sizes = sorted(((h, w) for h in range(128, 609, 128) for w in range(128, 1025, 128) if h <= w), key=lambda s: (s[0] * s[1], s))
        sizes.append((608, 1024))
        for hw in sizes:
            blob, ok, topk = e2e(hw)
            if ok:
                break
        assert ok, "no size up to 608x1024 yields 5..{} detections on each image".format(topk)
        out["e2e_r50"] = blob

    with open(os.path.join(HERE, "state_dict_keys_R50.txt"), "w") as f:
        for name, ks in keys.items():
            f.write("# {}\n".format(name) + "\n".join(ks) + "\n")
    for name, blob in out.items():
        path = os.path.join(HERE, name + ".pt")
        tmp = path + ".tmp"
        torch.save(blob, tmp)
        size = os.path.getsize(tmp)
        assert size < MAX_BYTES, "{} is {} bytes: fixtures stay under 1 MiB".format(name, size)
        os.replace(tmp, path)
        print("wrote", path, size // 1024, "KiB")


if __name__ == "__main__":
    main()
