"""-m gpu: Predictor (raw uint8 image in, Instances at the original resolution out) against the path that existed before it: the image
resized on the host (tests/resize_ref.py, the numpy restatement the CPU tests pin to Pillow) and fed to GeneralizedRCNN.inference as a CHW
float tensor with its original height and width.  Same resized bytes, same normalisation expression, same canvas: the same bits."""
import pytest
import torch

from centermask2_amd import Predictor, synthetic as S
from . import resize_ref
from .helpers import build_gpu_model, close, close_abs, match_detections

pytestmark = pytest.mark.gpu

MIN_SIZE, MAX_SIZE = 256, 400


def raw_image(h, w, seed):
    """A synthetic model input turned back into what a camera would hand over: (h, w, 3) uint8, BGR."""
    x = S.make_synthetic_images(1, h, w, seed0=seed)[0] + torch.tensor(S.PIXEL_MEAN).view(3, 1, 1)
    return x.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


@pytest.fixture(scope="module")
def predictor(dev):
    from centermask2_amd.config import config_path, get_cfg
    model, _ = build_gpu_model()
    cfg = get_cfg()
    cfg.merge_from_file(config_path("centermask_V_39_eSE_FPN_ms_3x.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MIN_SIZE_TEST", MIN_SIZE, "INPUT.MAX_SIZE_TEST", MAX_SIZE])
    cfg.freeze()
    return Predictor(cfg, model=model)


def test_predictor_equals_host_resize_plus_inference(dev, predictor):
    from centermask2_amd import ops
    raw = raw_image(128, 160, 77)
    new_h, new_w = ops.resize_shortest_edge_shape(128, 160, MIN_SIZE, MAX_SIZE)
    assert (new_h, new_w) == (256, 320)
    resized = torch.from_numpy(resize_ref.resize_bilinear_u8(raw.numpy(), new_h, new_w))
    with torch.no_grad():
        ref = predictor.model.inference([{"image": resized.permute(2, 0, 1).float().contiguous(), "height": 128, "width": 160}])[0]["instances"]
    torch.cuda.synchronize()
    assert len(ref) > 0, "the reference path alone must detect something"
    for image in (raw, raw.numpy(), raw.to(dev)):                   # torch tensor, numpy array, already on the device
        got = predictor(image)["instances"]
        torch.cuda.synchronize()
        assert tuple(got.image_size) == (128, 160) == tuple(ref.image_size) and len(got) == len(ref)
        assert torch.equal(got.pred_boxes.tensor, ref.pred_boxes.tensor) and torch.equal(got.scores, ref.scores)
        assert torch.equal(got.pred_classes, ref.pred_classes) and torch.equal(got.mask_scores, ref.mask_scores)
        assert got.pred_masks.dtype == torch.bool and tuple(got.pred_masks.shape) == (len(ref), 128, 160)
        assert torch.equal(got.pred_masks, ref.pred_masks) and bool(got.pred_masks.any())


def test_predict_batch_equals_single_calls(dev, predictor):
    """Two images that differ in height, width and scale.  Their sizes are chosen so that each alone and both together are padded to the
    same 256 x 320 canvas: the FCOS towers' GroupNorm takes its statistics over the padded map (as in detectron2), so a batch that pads an
    image further computes different activations for it, not differently rounded ones, and equality with a single call is not defined
    there.  On the shared canvas what may differ is rounding (a batch of 2 may run other conv kernels than a batch of 1): the same
    detections by class and location, scores within match_detections' 1e-4, boxes within 1e-4 of the largest coordinate
    (helpers.close), mask scores within the suite's 1e-3."""
    from centermask2_amd import ops
    raws = [raw_image(128, 160, 77), raw_image(124, 150, 78)]
    assert [ops.resize_shortest_edge_shape(r.shape[0], r.shape[1], MIN_SIZE, MAX_SIZE) for r in raws] == [(256, 320), (256, 310)]
    singles = [predictor(r)["instances"] for r in raws]
    both = predictor.predict_batch(raws)
    torch.cuda.synchronize()
    assert len(both) == 2
    for r, one, two in zip(raws, singles, (b["instances"] for b in both)):
        assert tuple(two.image_size) == tuple(r.shape[:2]) == tuple(one.image_size)
        assert len(one) == len(two) > 0
        p = match_detections(one.scores, one.pred_classes, one.locations, two.scores, two.pred_classes, two.locations, tol=1e-4).to(dev)
        assert torch.equal(two.pred_classes[p], one.pred_classes) and torch.equal(two.locations[p], one.locations)
        close(two.pred_boxes.tensor[p], one.pred_boxes.tensor, 1e-4, "predict_batch boxes (pixels)")
        close_abs(two.mask_scores[p], one.mask_scores, 1e-3, "predict_batch mask_scores")
        assert tuple(two.pred_masks.shape) == (len(one),) + tuple(r.shape[:2])
    # a batch whose canvas is larger than an image's own: sizes and resolutions still per image
    wide = raw_image(96, 176, 79)
    mixed = predictor.predict_batch([raws[0], wide])
    torch.cuda.synchronize()
    assert [tuple(m["instances"].image_size) for m in mixed] == [(128, 160), (96, 176)]
    assert all(tuple(m["instances"].pred_masks.shape[1:]) == tuple(m["instances"].image_size) for m in mixed)
