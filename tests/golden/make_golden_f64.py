"""Float64 golden vectors for the oracle tests of the convolutional parts, produced by the REFERENCE's own modules.

    python tests/golden/make_golden_f64.py        # needs /root/reference; writes tests/golden/reference_f64.npz

The fp32 fixtures (make_golden.py, make_golden_bodies.py) hold what the reference computed in float32 on the host that made them.  An
fp32 convolution sums in an order that depends on the CPU's vector width and thread count, so on another host the oracle lands
~1e-6 (relative) away from them by rounding alone.  Here the reference's modules run in float64 on the same seeded weights and on the
inputs those fixtures store.  Each output is stored as its correction to the fp32 fixture of the same case, an int8 count of steps of
STEP * max(1, max|output|) (that scale is the one tests/helpers.py:close applies its bar to), so a decoded value lies within half a
step — a twentieth of the tests' 1e-6 bar — of the float64 output; tests/helpers.py:golden_f64 decodes them.  The tests run the
oracle in float64 against them, which no host's summation order moves.  The ROI heads run on the pooled features roi_crafted.pt
stores (the reference's own), so that their float64 inputs are exact; the pooler itself keeps its fp32 fixture.  Data only — no
reference source.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the d2 stand-ins and imports the reference package)

S, O = G.S, G.O
BODIES = ("V-19-slim-dw-eSE", "V-19-dw-eSE", "V-19-slim-eSE", "V-19-eSE", "V-57-eSE")
STEP = 1e-7


def load(name):
    return torch.load(os.path.join(HERE, name + ".pt"), weights_only=True)


def f64(sd):
    return {k: v.double() for k, v in sd.items()}


def reference(body, sd):
    _, backbone, fcos, roi_heads = G.build_reference(body)
    G.load_synthetic(backbone, fcos, roi_heads, sd)
    return backbone.double(), fcos.double(), roi_heads.double()


def agree(got, ref, what):
    """The oracle and the reference, both in float64: they differ by float64 rounding only."""
    return G.close(got.double(), ref.double(), 1e-9, what)


def encode(out):
    """{fixture name: nested dict / list of float64 outputs} -> npz arrays: "<name>.<key>..." (int8 steps from the fp32 fixture's
    value at the same place) and "step.<name>.<key>..." (the step)."""
    arrays = {}

    def walk(path, ref, base):
        if isinstance(ref, dict):
            for k in ref:
                walk(path + [k], ref[k], base[k])
        elif isinstance(ref, list):
            for i, r in enumerate(ref):
                walk(path + [str(i)], r, base[i])
        else:
            step = STEP * max(1.0, float(ref.abs().max()))
            q = ((ref - base.double()) / step).round()
            assert float(q.abs().max()) <= 127, (path, float(q.abs().max()))
            assert float((base.double() + q * step - ref).abs().max()) <= 0.5 * step * (1 + 1e-9), path
            key = ".".join(path)
            arrays[key] = q.to(torch.int8).numpy()
            arrays["step." + key] = np.float64(step)

    for name, ref in out.items():
        walk([name], ref, load(name))
    return arrays


def main():
    out = {}
    sd = S.make_synthetic_state_dict("V-39-eSE", seed=0)
    sd64 = f64(sd)
    backbone, fcos, roi_heads = reference("V-39-eSE", sd)
    with torch.no_grad():
        x = load("vovnet_odd")["x"].double()
        ref, orc = backbone.bottom_up(x), O.vovnet_forward(sd64, x)
        out["vovnet_odd"] = dict(ref)
        for k in ref:
            print("vovnet odd", k, agree(orc[k], ref[k], "vovnet " + k))

        bb = load("backbone_small")
        x = bb["x"].double()
        ref, orc = backbone(x), O.backbone_forward(sd64, x)
        out["backbone_small"] = dict(ref)
        for k in ref:
            print("backbone+fpn", k, agree(orc[k], ref[k], "fpn " + k))

        # FCOS head with the shifted class bias of fcos_small.pt, on the fp32 fixture's features (exact in float64)
        shift = float(load("fcos_small")["cls_bias_shift"])
        feats = [bb[k].double() for k in ("p3", "p4", "p5", "p6", "p7")]
        key = "proposal_generator.fcos_head.cls_logits.bias"
        sd_shift = dict(sd64)
        sd_shift[key] = sd64[key] + shift
        fcos.fcos_head.cls_logits.bias.data += shift
        rl, rr, rc, _ = fcos.fcos_head(feats)
        fcos.fcos_head.cls_logits.bias.data -= shift
        ol, orr, oc = O.fcos_head_forward(sd_shift, feats)
        for l in range(5):
            agree(ol[l], rl[l], "logits")
            agree(orr[l], rr[l], "reg")
            agree(oc[l], rc[l], "ctr")
        out["fcos_small"] = dict(logits=list(rl), reg=list(rr), ctr=list(rc))
        print("fcos head: logits / reg / ctr agree")

        # ROI heads (SAM mask head -> mask selection -> MaskIoU) on the reference's pooled features of the crafted boxes
        g = load("roi_crafted")
        roi_feat = g["roi_feat"].double()
        insts = []
        for i in range(2):
            r = g["img{}".format(i)]
            it = G.Instances((64, 96))
            it.pred_boxes = G.Boxes(r["boxes"].clone())
            it.pred_classes = r["classes"]
            it.scores = r["scores"].double()
            it.locations = r["boxes"][:, :2].clone()
            insts.append(it)
        roi_heads.mask_pooler.forward = lambda features, instances: roi_feat
        rres = G.quiet(roi_heads.forward_with_given_boxes, {k: bb[k].double() for k in ("p3", "p4", "p5")}, insts)
        rlogits = roi_heads.mask_head(roi_feat)
        rmiou = roi_heads.maskiou_head(roi_feat, torch.cat([r_.pred_masks for r_ in rres]))
        classes = torch.cat([g["img{}".format(i)]["classes"] for i in range(2)])
        scores = torch.cat([g["img{}".format(i)]["scores"] for i in range(2)]).double()
        ologits = O.sam_mask_head_forward(sd64, roi_feat)
        omasks = O.mask_rcnn_inference(ologits, classes)
        omiou = O.maskiou_head_forward(sd64, roi_feat, omasks)
        agree(ologits, rlogits, "mask_logits")
        agree(omasks, torch.cat([r_.pred_masks for r_ in rres]), "pred_masks")
        agree(omiou, rmiou, "maskiou")
        agree(O.mask_iou_inference(scores, classes, omiou), torch.cat([r_.mask_scores for r_ in rres]), "mask_scores")
        out["roi_crafted"] = dict(mask_logits=rlogits, maskiou=rmiou,
                                  **{"img{}".format(i): dict(pred_masks=rres[i].pred_masks, mask_scores=rres[i].mask_scores) for i in range(2)})
        print("roi heads: mask logits / masks / maskiou / mask scores agree")

        bodies = load("vovnet_bodies")
        out["vovnet_bodies"] = {}
        for body in BODIES:
            sdb = S.make_synthetic_state_dict(body, seed=0)
            backbone_b, _, _ = reference(body, sdb)
            case = bodies[body]
            ref_bu, orc_bu = backbone_b.bottom_up(case["x"].double()), O.vovnet_forward(f64(sdb), case["x"].double(), conv_body=body)
            ref, orc = backbone_b(case["x32"].double()), O.backbone_forward(f64(sdb), case["x32"].double(), conv_body=body)
            for k in ref_bu:
                agree(orc_bu[k], ref_bu[k], body + " " + k)
            for k in ref:
                agree(orc[k], ref[k], body + " " + k)
            out["vovnet_bodies"][body] = dict(**ref_bu, **ref)
            print(body, "agrees")

    path = os.path.join(HERE, "reference_f64.npz")
    np.savez_compressed(path, **encode(out))
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
