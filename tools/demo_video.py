"""Run the model over a clip and draw every frame with colours that follow the objects: Predictor, then VideoVisualizer, then PNGs (the
reference's demo.py --video-input, without detectron2's host-side VideoVisualizer and without a video or imaging library).

    python tools/demo_video.py CONFIG FRAMES_DIR OUT_DIR [--weights FILE] [--match box|mask] [--ttl N] [--max-tracks N]
                               [--min-size N --max-size N] [--score-threshold T]

FRAMES_DIR holds the frames as binary P6 `.ppm` or as `.npy` files of (h,w,3) uint8 arrays in the config's INPUT.FORMAT channel order (a
.ppm is RGB on disk and is converted); they are taken in name order.  OUT_DIR gets one PNG per frame under the frame's name, and the
track ids of every frame are printed.  Without --weights and without MODEL.WEIGHTS a VoVNet config gets the seeded synthetic weights,
which detect arbitrary things: good for trying the tools, nothing else."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_files(frames_dir):
    """The .ppm / .npy files of a directory, in name order."""
    names = sorted(f for f in os.listdir(frames_dir) if f.lower().endswith((".ppm", ".npy")))
    if not names:
        raise SystemExit("demo_video: no .ppm or .npy frames in {}".format(frames_dir))
    return [os.path.join(frames_dir, f) for f in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("frames_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--match", default="box", choices=("box", "mask"), help="IoU of the boxes (detectron2's default) or of the masks")
    ap.add_argument("--ttl", type=int, default=8, help="frames a track outlives its last match")
    ap.add_argument("--max-tracks", type=int, default=256)
    ap.add_argument("--score-threshold", type=float, default=None, help="track and draw only detections at or above this score")
    ap.add_argument("--min-size", type=int, default=None, help="INPUT.MIN_SIZE_TEST")
    ap.add_argument("--max-size", type=int, default=None, help="INPUT.MAX_SIZE_TEST")
    a = ap.parse_args()
    files = frame_files(a.frames_dir)

    import numpy as np
    import torch
    from centermask2_amd import Predictor, VideoVisualizer, synthetic as S
    from centermask2_amd.config import config_path, get_cfg
    from centermask2_amd.modeling import build_model
    from centermask2_amd.visualize import COCO_CLASSES, read_ppm, write_png

    if not torch.cuda.is_available():
        raise SystemExit("demo_video needs the MI355X: there is no CPU path")
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
            raise SystemExit("demo_video: give --weights; the synthetic stand-in is wired for the VoVNet configs only")
        model.load_state_dict(S.make_synthetic_state_dict(cfg.MODEL.VOVNET.CONV_BODY, 0))
        print("no weights given: seeded synthetic weights")
    fmt = cfg.INPUT.FORMAT
    pred = Predictor(cfg, model=model)
    names = COCO_CLASSES if int(cfg.MODEL.FCOS.NUM_CLASSES) == len(COCO_CLASSES) else None
    vis = VideoVisualizer(class_names=names, input_format=fmt, match=a.match, ttl=a.ttl, max_tracks=a.max_tracks)
    os.makedirs(a.out_dir, exist_ok=True)
    size = None
    for path in files:
        image = read_ppm(path, output_format=fmt) if path.lower().endswith(".ppm") else np.load(path)
        if size is not None and tuple(image.shape[:2]) != size:
            vis.reset()                                              # a clip of another size starts over
        size = tuple(image.shape[:2])
        inst = pred(image)["instances"]
        if a.score_threshold is not None:
            inst = inst[inst.scores >= a.score_threshold]
        out = vis.draw(image, inst)
        dst = os.path.join(a.out_dir, os.path.splitext(os.path.basename(path))[0] + ".png")
        write_png(dst, out, input_format=fmt)                        # the download of the picture; the ids come down for the printout
        print("{}: {} detections, track ids {}".format(dst, len(inst), inst.track_ids.cpu().tolist()))
    print("{} frames, {} tracks numbered, {} dropped for lack of room".format(len(files), vis.tracker.next_id, vis.tracker.dropped))


if __name__ == "__main__":
    main()
