"""-m gpu: Visualizer.draw (csrc/visualize.hip) against the tests' NumPy restatement of the rendering rules (tests/visualize_ref.py), byte
for byte: every comparison is torch.equal on uint8, no tolerance and no pixel left out.  Shapes: (37,70) has a tail word and rows that
straddle words, (16,64) rows that are words, (5,3) is smaller than one word and than any plate, (40,129) has rows of two words and a bit."""
import itertools

import numpy as np
import pytest
import torch

from centermask2_amd import Visualizer, draw_instance_predictions
from centermask2_amd._lib import CmkError
from centermask2_amd.structures import Boxes, Instances
from centermask2_amd.visualize import COCO_CLASSES, COCO_PERSON_SKELETON
from . import visualize_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(37, 70), (16, 64), (5, 3), (40, 129)]
NAN = float("nan")


def scene(h, w, n, seed):
    """(image, boxes, scores, classes, masks) as NumPy arrays.  n = 7 — masks: two blobs that overlap, an empty one, a full one, a cross
    that touches all four borders, a single pixel in a corner, seeded noise; boxes: inside, past the left and top, past the right and
    bottom, entirely outside, zero area, one NaN, and a small one in the bottom right corner whose plate has to be clamped at both edges.
    n = 1 keeps the first of each."""
    rng = np.random.RandomState(seed)
    image = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    masks = np.zeros((7, h, w), dtype=bool)
    masks[0] = ((xs - 0.40 * w) / (0.30 * w + 1)) ** 2 + ((ys - 0.45 * h) / (0.35 * h + 1)) ** 2 <= 1
    masks[1] = ((xs - 0.60 * w) / (0.25 * w + 1)) ** 2 + ((ys - 0.55 * h) / (0.30 * h + 1)) ** 2 <= 1
    masks[3] = True
    masks[4] = (xs == w // 2) | (ys == h // 2)
    masks[5, h - 1, w - 1] = True
    masks[6] = rng.rand(h, w) < 0.5
    boxes = np.array([[0.2 * w, 0.15 * h, 0.8 * w + 0.5, 0.9 * h - 0.25],
                      [-0.3 * w - 2, -4.5, 0.5 * w, 0.6 * h],
                      [0.45 * w, 0.5 * h, 1.4 * w + 3, h + 7.75],
                      [w + 5, h + 3, 2 * w + 9, 2 * h + 9],
                      [0.5 * w, 0.5 * h, 0.5 * w, 0.5 * h],
                      [0.1 * w, NAN, 0.7 * w, 0.8 * h],
                      [w - 3.5, h - 2.5, w - 0.5, h - 0.5]], dtype=np.float32)
    scores = np.array([0.9, 0.005, 0.995, NAN, 1.0, 0.5, 0.07], dtype=np.float32)
    classes = np.array([0, 79, 9, 80, 67, -2, 17], dtype=np.int64)            # 80 and -2 have no name: "C80", "C-2"
    return image, boxes[:n], scores[:n], classes[:n], masks[:n]


def instances_on(dev, h, w, boxes, scores, classes, masks=None, keypoints=None):
    inst = Instances((h, w), pred_boxes=Boxes(torch.from_numpy(boxes).to(dev)), scores=torch.from_numpy(scores).to(dev),
                     pred_classes=torch.from_numpy(classes).to(dev))
    if masks is not None:
        inst.pred_masks = torch.from_numpy(masks).to(dev)
    if keypoints is not None:
        inst.pred_keypoints = torch.from_numpy(keypoints).to(dev)
    return inst


def check(dev, image, boxes, scores, classes, masks=None, keypoints=None, skeleton=None, **kw):
    """One draw against the restatement; also: the input image is untouched and the output is a new tensor."""
    h, w = image.shape[:2]
    img = torch.from_numpy(image).to(dev)
    inst = instances_on(dev, h, w, boxes, scores, classes, masks, keypoints)
    vis_kw = dict(kw)
    if skeleton is not None:
        vis_kw["skeleton"] = skeleton
    got = Visualizer(**vis_kw).draw(img, inst)
    want = R.render(image, boxes, scores, classes, masks=masks, keypoints=keypoints, skeleton=skeleton or (), **kw)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and got.device == img.device and got.data_ptr() != img.data_ptr()
    assert torch.equal(img.cpu(), torch.from_numpy(image)), "draw changed its input image"
    if not torch.equal(got.cpu(), torch.from_numpy(want)):
        bad = (got.cpu() != torch.from_numpy(want)).any(dim=2).nonzero()
        raise AssertionError("{} pixels differ, the first at (y, x) = {}: got {}, want {}; {}".format(
            len(bad), bad[0].tolist(), got.cpu()[tuple(bad[0])].tolist(), want[tuple(bad[0].tolist())].tolist(), kw))
    return got, want


@pytest.mark.parametrize("n", [0, 1, 7])
@pytest.mark.parametrize("h,w", SHAPES)
def test_draw_matches_restatement(dev, h, w, n):
    image, boxes, scores, classes, masks = scene(h, w, n, seed=100 * h + n)
    drawn = False
    for lw, fs, alpha, color_by, fmt in itertools.product((1, 3), (1, 2), (0.0, 0.5, 1.0), ("instance", "class"), ("BGR", "RGB")):
        names = COCO_CLASSES if color_by == "class" else None
        got, want = check(dev, image, boxes, scores, classes, masks=masks, class_names=names, alpha=alpha, line_width=lw, font_scale=fs,
                          color_by=color_by, input_format=fmt)
        drawn = drawn or bool((want != image).any())
    assert drawn == (n > 0), "a picture with instances must differ from its image, one without must not"


def test_box_only_instances_and_clamped_plate(dev):
    """No pred_masks at all; names with characters outside the font and longer than a label; the last box sits in the bottom right
    corner, so its plate is clamped at the right and at the bottom edge."""
    h, w = 37, 70
    image, boxes, scores, classes, _ = scene(h, w, 7, seed=5)
    classes = np.array([0, 1, 2, 3, 1, 0, 2], dtype=np.int64)
    names = ["a_b.c-d", "x" * 40, "Stop Sign"]                       # class 3 falls back to "C3"
    for lw, fs in ((1, 1), (3, 2)):
        got, want = check(dev, image, boxes, scores, classes, class_names=names, line_width=lw, font_scale=fs, input_format="RGB")
        assert (want[h - 1, w - 1] != image[h - 1, w - 1]).any(), "the clamped plate reaches the last pixel"
    # the defaults: line width and font scale from the image size, alpha 0.5, BGR, colour by instance, "C<id>" names
    img = torch.from_numpy(image).to(dev)
    got = draw_instance_predictions(img, instances_on(dev, h, w, boxes, scores, classes))
    assert torch.equal(got.cpu(), torch.from_numpy(R.render(image, boxes, scores, classes)))
    # a NumPy image is uploaded
    got2 = Visualizer().draw(image, instances_on(dev, h, w, boxes, scores, classes))
    assert got2.is_cuda and torch.equal(got2, got)


def keypoint_scene(h, w, n, k, seed):
    rng = np.random.RandomState(seed)
    kp = np.zeros((n, k, 3), dtype=np.float32)
    kp[:, :, 0] = rng.uniform(-12, w + 12, size=(n, k))              # some points outside the image
    kp[:, :, 1] = rng.uniform(-12, h + 12, size=(n, k))
    thr = np.float32(0.05)
    choices = np.array([0.9, 0.3, thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0)), 0.0, NAN, 0.9, 0.8], dtype=np.float32)
    kp[:, :, 2] = choices[rng.randint(0, len(choices), size=(n, k))]
    return kp


@pytest.mark.parametrize("lw", [1, 3])
def test_keypoints_coco_skeleton(dev, lw):
    """K = 17 with the COCO skeleton on (40,129), three instances with masks and boxes below the keypoints.  Instances 0 and 1 carry two
    long visible segments that cross (5-6 of one, 5-6 of the other): the later instance in draw order owns the crossing."""
    h, w, n = 40, 129, 3
    image, boxes, scores, classes, masks = scene(h, w, n, seed=9)
    kp = keypoint_scene(h, w, n, 17, seed=10)
    kp[0, 5], kp[0, 6] = (3.2, 2.7, 0.9), (120.9, 37.1, 0.9)
    kp[1, 5], kp[1, 6] = (4.0, 36.5, 0.9), (125.5, 1.5, 0.9)
    kp[2, 7, :2] = kp[2, 5, :2]                                        # coincident end points of segment (5, 7)
    kp[2, 5, 2] = kp[2, 7, 2] = 0.9
    kp[2, 0, 0] = NAN                                                  # a NaN coordinate is not drawn
    skel = [tuple(p) for p in COCO_PERSON_SKELETON]
    for fmt in ("BGR", "RGB"):
        got, want = check(dev, image, boxes, scores, classes, masks=masks, keypoints=kp, skeleton=skel, line_width=lw, font_scale=1, input_format=fmt)
    # where the two diagonals cross, the instance drawn earlier never shows (want is the RGB picture here, colours by instance)
    order = R.draw_order(boxes)
    below = 0 if order.index(0) < order.index(1) else 1
    cross = [(y, x) for y in range(h) for x in range(w) if R.on_segment(x, y, 3, 2, 120, 37, lw) and R.on_segment(x, y, 4, 36, 125, 1, lw)]
    assert all(tuple(want[y, x]) != R.colours(below, "RGB")[0] for y, x in cross) and (cross or lw == 1)
    # the default skeleton for 17 keypoints is COCO's
    inst = instances_on(dev, h, w, boxes, scores, classes, masks, kp)
    got_default = Visualizer(line_width=lw, font_scale=1, input_format="RGB").draw(torch.from_numpy(image).to(dev), inst)
    assert torch.equal(got_default, got)


@pytest.mark.parametrize("lw", [1, 3])
def test_keypoints_custom_skeleton(dev, lw):
    """K = 3 on (37,70): a triangle plus a segment from a point to itself; box-only instances; a threshold other than the default."""
    h, w, n = 37, 70, 7
    image, boxes, scores, classes, _ = scene(h, w, n, seed=11)
    kp = keypoint_scene(h, w, n, 3, seed=12)
    skel = [(0, 1), (1, 2), (2, 0), (1, 1)]
    check(dev, image, boxes, scores, classes, keypoints=kp, skeleton=skel, line_width=lw, font_scale=1)
    check(dev, image, boxes, scores, classes, keypoints=kp, skeleton=skel, line_width=lw, font_scale=1, keypoint_threshold=0.5, color_by="class")
    # without a skeleton K = 3 draws discs only
    inst = instances_on(dev, h, w, boxes, scores, classes, None, kp)
    got = Visualizer(line_width=lw, font_scale=1).draw(torch.from_numpy(image).to(dev), inst)
    assert torch.equal(got.cpu(), torch.from_numpy(R.render(image, boxes, scores, classes, keypoints=kp, skeleton=(), line_width=lw, font_scale=1)))


def test_draw_batch_equals_loop_and_refusals(dev):
    vis = Visualizer(class_names=COCO_CLASSES, line_width=1, font_scale=1)
    images, insts = [], []
    for (h, w), n in zip(SHAPES, (7, 1, 7, 0)):
        image, boxes, scores, classes, masks = scene(h, w, n, seed=h)
        images.append(torch.from_numpy(image).to(dev))
        insts.append(instances_on(dev, h, w, boxes, scores, classes, masks))
    batch = vis.draw_batch(images, insts)
    assert len(batch) == 4 and all(torch.equal(b, vis.draw(im, it)) for b, im, it in zip(batch, images, insts))
    with pytest.raises(CmkError, match="4 images"):
        vis.draw_batch(images, insts[:2])
    with pytest.raises(CmkError, match="37x70.*16x64"):                # Instances of another size
        vis.draw(images[1], insts[0])
    with pytest.raises(CmkError, match=r"float32.*\(37, 70, 3\)"):
        vis.draw(images[0].float(), insts[0])
    with pytest.raises(CmkError, match=r"\(37, 70\)"):
        vis.draw(images[0][:, :, 0], insts[0])
    big = 65536
    many = Instances((37, 70), pred_boxes=Boxes(torch.zeros((big, 4), device=dev)), scores=torch.zeros(big, device=dev),
                     pred_classes=torch.zeros(big, dtype=torch.int64, device=dev))
    with pytest.raises(CmkError, match=r"\(65536, 4\)"):
        vis.draw(images[0], many)
    bad_masks = instances_on(dev, 37, 70, *scene(37, 70, 7, seed=1)[1:4], masks=scene(16, 64, 7, seed=1)[4])
    with pytest.raises(CmkError, match=r"\(7, 16, 64\)"):
        vis.draw(images[0], bad_masks)


def test_draw_is_capturable_and_bakes_nothing_on_the_host(dev):
    """One capture of draw at (37,70) with 7 instances on a single stream; the replay equals the eager picture, and after the input
    tensors' contents change in place it equals the eager picture of the new contents."""
    h, w, n = 37, 70, 7
    image, boxes, scores, classes, masks = scene(h, w, n, seed=21)
    kp = keypoint_scene(h, w, n, 17, seed=22)
    vis = Visualizer(class_names=COCO_CLASSES, line_width=1, font_scale=1, color_by="class")
    img = torch.from_numpy(image).to(dev)
    inst = instances_on(dev, h, w, boxes, scores, classes, masks, kp)
    eager = vis.draw(img, inst).clone()                                # also uploads the tables of this device
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vis.draw(img, inst)                                            # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = vis.draw(img, inst)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # new contents, same tensors: another image, the instances reversed (so the draw order, labels and colours all change)
    image2 = scene(h, w, n, seed=23)[0]
    kp2 = keypoint_scene(h, w, n, 17, seed=24)
    img.copy_(torch.from_numpy(image2))
    inst.pred_boxes.tensor.copy_(torch.from_numpy(boxes[::-1].copy()))
    inst.scores.copy_(torch.from_numpy(scores[::-1].copy()))
    inst.pred_classes.copy_(torch.from_numpy(classes[::-1].copy()))
    inst.pred_masks.copy_(torch.from_numpy(masks[::-1].copy()))
    inst.pred_keypoints.copy_(torch.from_numpy(kp2))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager2 = vis.draw(img, inst)
    want2 = R.render(image2, boxes[::-1], scores[::-1], classes[::-1], masks=masks[::-1], keypoints=kp2, skeleton=COCO_PERSON_SKELETON,
                     class_names=COCO_CLASSES, line_width=1, font_scale=1, color_by="class")
    assert torch.equal(eager2.cpu(), torch.from_numpy(want2)) and not torch.equal(eager2, eager)
    assert torch.equal(replayed, eager2), "{} pixels of the replay differ from the eager picture of the new contents".format(
        int((replayed != eager2).any(dim=2).sum()))


def test_predictor_to_picture_end_to_end(dev):
    """The synthetic model on one small synthetic image through Predictor, then Visualizer.draw: equal to the restatement run on the
    downloaded Instances, and not the input image."""
    from centermask2_amd import Predictor
    from centermask2_amd.config import config_path, get_cfg
    from .helpers import build_gpu_model
    from .test_gpu_predictor import MAX_SIZE, MIN_SIZE, raw_image
    model, _ = build_gpu_model()
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MIN_SIZE_TEST", MIN_SIZE, "INPUT.MAX_SIZE_TEST", MAX_SIZE])
    cfg.freeze()
    raw = raw_image(128, 160, 77)
    inst = Predictor(cfg, model=model)(raw)["instances"]
    assert len(inst) > 0 and bool(inst.pred_masks.any()), "the synthetic weights detect something at this size (test_gpu_predictor relies on it too)"
    vis = Visualizer(class_names=COCO_CLASSES)
    got = vis.draw(raw, inst)
    want = R.render_instances(raw, inst, class_names=COCO_CLASSES)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert not torch.equal(got.cpu(), raw), "a picture of detections differs from its image"
