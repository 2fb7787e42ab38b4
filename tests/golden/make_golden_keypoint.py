"""Golden vectors for the keypoint branch of CenterROIHeads (MODEL.KEYPOINT_ON): the REFERENCE's own ROIPooler and
KRCNNConvDeconvUpsampleHead.layers, built by its CenterROIHeads._init_keypoint_head (center_heads.py:358-382), on small seeded pyramids.

    python tests/golden/make_golden_keypoint.py      # needs /root/reference; writes tests/golden/roi_keypoint.pt

Two set-ups, both with the "ratio" level rule: IN_FEATURES p3-p5 (what the shipped CenterMask backbones produce) and the default p2-p5.
CONV_DIMS is reduced to (32, 16) on 16-channel pyramids — a production state dict is 66 MB — NUM_KEYPOINTS stays 17.  Per set-up the
file holds the features, boxes and image sizes, the head's state dict, the pooled features (fp32, as the reference computes them) and,
from those pooled features with the head in float64, the score_lowres maps of the first LOWRES_ROIS RoIs (the file stays under 1 MiB)
and the `layers` output of RoI 0 for the keypoints PROBE_KP (both rounded to fp32 for storage: 6e-8 relative).  ConvTranspose2d and interpolate enter through
tests/golden/d2_stub.py as torch's own; detectron2's heatmaps_to_keypoints is absent, so no decoded keypoints are stored.  Data only.
"""
import os
import sys
from collections import OrderedDict

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the d2 stand-ins and imports the reference package)

from centermask.modeling.centermask.center_heads import CenterROIHeads  # noqa: E402
from centermask2_amd.structures import Boxes, Instances, ShapeSpec  # noqa: E402

C, CONV_DIMS, PROBE_KP, LOWRES_ROIS = 16, (32, 16), (0, 16), 4
SETUPS = {
    # name: (IN_FEATURES, padded (H, W), image sizes, boxes per image) — box areas chosen so that the ratio rule
    # ceil(5 - log2(image area / box area)) lands on every level of the set-up and is clamped at both ends
    "p3_p5": (["p3", "p4", "p5"], (128, 160), [(128, 160), (96, 112)],
              [[[8.0, 6.0, 150.5, 120.25], [20.5, 30.0, 110.0, 100.0], [40.0, 40.0, 75.5, 90.0], [100.0, 10.0, 112.0, 19.5]],
               [[0.0, 0.0, 112.0, 96.0], [30.25, 20.0, 90.0, 70.5], [5.0, 50.0, 25.0, 64.0]]]),
    "p2_p5": (["p2", "p3", "p4", "p5"], (96, 128), [(96, 128), (64, 96)],
              [[[4.0, 2.0, 120.0, 90.0], [10.0, 10.0, 80.5, 60.0], [50.0, 30.0, 90.0, 70.25], [60.0, 5.0, 84.0, 31.0], [3.0, 70.0, 9.5, 80.0]],
               [[20.0, 8.0, 70.0, 52.5], [1.5, 2.5, 33.0, 40.0]]]),
}


def run(name, in_features, pad, sizes, boxes):
    cfg = G.ref_get_cfg()
    cfg.merge_from_file("/root/reference/centermask2/configs/centermask/zy_model_config.yaml")
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.KEYPOINT_ON", True, "MODEL.ROI_KEYPOINT_HEAD.IN_FEATURES", in_features,
                         "MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", CONV_DIMS, "MODEL.ROI_HEADS.IN_FEATURES", ["p3", "p4", "p5"]])
    cfg.freeze()
    assert cfg.MODEL.ROI_KEYPOINT_HEAD.ASSIGN_CRITERION == "ratio" and cfg.MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS == 17
    shapes = {"p{}".format(l): ShapeSpec(channels=C if "p{}".format(l) in in_features else 256, stride=2 ** l) for l in range(2, 8)}
    heads = CenterROIHeads(cfg, shapes).eval()
    pooler, head = heads.keypoint_pooler, heads.keypoint_head
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in name))
    sd = OrderedDict()
    for k, v in head.state_dict().items():
        if v.dim() == 4:      # Kaiming trunk; score_lowres sums Cin * 4 taps per output pixel: logits of order 1
            std = (2.0 / (v.shape[1] * 9)) ** 0.5 if "conv_fcn" in k else 3.0 * (1.0 / (4 * v.shape[0])) ** 0.5
        else:
            std = 0.1
        sd[k] = torch.randn(v.shape, generator=g) * std
    head.load_state_dict(sd, strict=True)
    feats = [torch.randn((len(sizes), C, pad[0] // 2 ** int(f[1]), pad[1] // 2 ** int(f[1])), generator=g) for f in in_features]
    insts = [Instances(tuple(hw), pred_boxes=Boxes(torch.tensor(b, dtype=torch.float32)), pred_classes=torch.zeros(len(b), dtype=torch.int64))
             for hw, b in zip(sizes, boxes)]      # pooler.py:72 reads pred_classes' device
    with torch.no_grad():
        pooled = G.quiet(pooler, feats, insts)
        assert pooled.dtype == torch.float32
        head64 = head.double()
        x = pooled.double()
        for layer in head64.blocks:
            x = torch.relu(layer(x))
        lowres = head64.score_lowres(x)
        logits = head64.layers(pooled.double())
    levels = G.assign_boxes_to_levels_by_ratio(insts, pooler.min_level, pooler.max_level)
    assert sorted(set(levels.tolist())) == list(range(len(in_features))), levels.tolist()
    k = head.score_lowres.out_channels
    assert lowres.shape == (pooled.shape[0], k, 28, 28) and logits.shape == (pooled.shape[0], k, 56, 56)
    print(name, "RoIs", pooled.shape[0], "levels", levels.tolist(), "lowres std %.3f" % float(lowres.std()), "absmax %.3f" % float(lowres.abs().max()))
    out = dict(in_features=list(in_features), image_sizes=torch.tensor(sizes), boxes=[torch.tensor(b, dtype=torch.float32) for b in boxes],
               levels=levels.clone(), state_dict=OrderedDict((kk, v.clone()) for kk, v in sd.items()), pooled=pooled.clone(),
               score_lowres=lowres[:LOWRES_ROIS].float(), layers_roi0=logits[0, list(PROBE_KP)].float(), probe_kp=torch.tensor(PROBE_KP),
               conv_dims=torch.tensor(CONV_DIMS))
    for f, t in zip(in_features, feats):
        out[f] = t
    return out


def main():
    out = {name: run(name, *spec) for name, spec in SETUPS.items()}
    path = os.path.join(HERE, "roi_keypoint.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
