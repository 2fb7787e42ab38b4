"""See what the model detects in one image: Predictor, then Visualizer, then a PNG (the reference's visualizer.py:21-38, without
detectron2's matplotlib renderer and without an imaging library).

    python tools/demo.py CONFIG IMAGE OUT.png [--weights FILE] [--min-size N --max-size N] [--score-threshold T]
                         [--json OUT.json [--segmentation rle|polygon]]

CONFIG is a yaml of centermask2_amd/configs (a bare file name is looked up there); IMAGE is a binary P6 `.ppm` or a `.npy` holding an
(h,w,3) uint8 array in the config's INPUT.FORMAT channel order (a .ppm is RGB on disk and is converted).  Without --weights and without
MODEL.WEIGHTS a VoVNet config gets the seeded synthetic weights, which detect arbitrary things: good for trying the tools, nothing else.
--json also writes the detections as COCO results (wire.instances_to_coco_json, image_id 0), their masks as compressed RLE or as the
polygons of their outer boundaries, traced on the device (holes are not represented in polygons)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("image")
    ap.add_argument("out")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--score-threshold", type=float, default=None, help="draw only detections at or above this score")
    ap.add_argument("--min-size", type=int, default=None, help="INPUT.MIN_SIZE_TEST")
    ap.add_argument("--max-size", type=int, default=None, help="INPUT.MAX_SIZE_TEST")
    ap.add_argument("--json", default=None, help="also write the detections as COCO results to this file")
    ap.add_argument("--segmentation", choices=("rle", "polygon"), default="rle", help="form of the masks in --json")
    a = ap.parse_args()

    import numpy as np
    import torch
    from centermask2_amd import Predictor, Visualizer, synthetic as S
    from centermask2_amd.config import config_path, get_cfg
    from centermask2_amd.modeling import build_model
    from centermask2_amd.visualize import COCO_CLASSES, read_ppm, write_png

    if not torch.cuda.is_available():
        raise SystemExit("demo needs the MI355X: there is no CPU path")
    cfg = get_cfg()
    cfg.merge_from_file(a.config if os.path.exists(a.config) else config_path(a.config))
    opts = ["MODEL.DEVICE", "cuda"]
    for key, v in (("MODEL.WEIGHTS", a.weights), ("INPUT.MIN_SIZE_TEST", a.min_size), ("INPUT.MAX_SIZE_TEST", a.max_size)):
        if v is not None:
            opts += [key, v]
    cfg.merge_from_list(opts)
    cfg.freeze()
    model = build_model(cfg)
    if not cfg.MODEL.WEIGHTS:
        if "vovnet" not in cfg.MODEL.BACKBONE.NAME:
            raise SystemExit("demo: give --weights; the synthetic stand-in is wired for the VoVNet configs only")
        model.load_state_dict(S.make_synthetic_state_dict(cfg.MODEL.VOVNET.CONV_BODY, 0))
        print("no weights given: seeded synthetic weights")
    fmt = cfg.INPUT.FORMAT
    image = read_ppm(a.image, output_format=fmt) if a.image.lower().endswith(".ppm") else np.load(a.image)
    inst = Predictor(cfg, model=model)(image)["instances"]
    if a.score_threshold is not None:
        inst = inst[inst.scores >= a.score_threshold]
    names = COCO_CLASSES if int(cfg.MODEL.FCOS.NUM_CLASSES) == len(COCO_CLASSES) else None
    out = Visualizer(class_names=names, input_format=fmt).draw(image, inst)
    write_png(a.out, out, input_format=fmt)
    print("{} detections drawn into {}".format(len(inst), a.out))
    if a.json:
        import json
        from centermask2_amd import wire
        with open(a.json, "w") as f:
            json.dump(wire.instances_to_coco_json(inst, 0, segmentation=a.segmentation), f)
        print("{} COCO results ({}) written to {}".format(len(inst), a.segmentation, a.json))


if __name__ == "__main__":
    main()
