"""Raw image in, instances out: the counterpart of detectron2's DefaultPredictor on the HIP path.

    pred = Predictor(cfg)                       # build_model(cfg), cfg.MODEL.WEIGHTS if set, eval mode
    inst = pred(image_bgr_u8)["instances"]      # (h, w, 3) uint8 numpy array or torch tensor -> Instances at h x w

The reference's loader (deploy_utils.py:60-73) resizes on the CPU with ResizeShortestEdge(800, 1333) and uploads floats; here the raw
bytes are uploaded and the resize runs on the device, fused with the normalisation and the padding (ops.resize_preprocess_images), so no
imaging library is needed.  The output side is detectron2's detector_postprocess (postprocess.detector_postprocess_d2)."""
from typing import Dict, List, Sequence

import torch

from . import _lib, ops
from .postprocess import detector_postprocess_d2
from .structures import ImageList, Instances

__all__ = ["Predictor", "load_weights"]


def load_weights(model: torch.nn.Module, path: str) -> torch.nn.Module:
    """cfg.MODEL.WEIGHTS: a file torch.save wrote, holding a state dict or a {"model": state_dict} checkpoint; the keys must be exactly
    the model's (strict)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(ckpt, dict) and isinstance(ckpt.get("model"), dict):
        ckpt = ckpt["model"]
    if not isinstance(ckpt, dict) or not all(torch.is_tensor(v) for v in ckpt.values()):
        raise _lib.CmkError("load_weights: {} holds neither a state dict nor a {{'model': state_dict}} checkpoint".format(path))
    model.load_state_dict(ckpt, strict=True)
    return model


class Predictor:
    def __init__(self, cfg, model=None):
        if model is None:
            from .modeling import build_model
            model = build_model(cfg)
        if cfg.MODEL.WEIGHTS:
            load_weights(model, cfg.MODEL.WEIGHTS)
        self.cfg = cfg
        self.model = model.eval()
        self.min_size = int(cfg.INPUT.MIN_SIZE_TEST)
        self.max_size = int(cfg.INPUT.MAX_SIZE_TEST)
        self.input_format = cfg.INPUT.FORMAT
        if self.input_format not in ("BGR", "RGB"):
            raise _lib.CmkError("Predictor: INPUT.FORMAT must be BGR or RGB, got {!r}".format(self.input_format))
        self.tta = None                         # cfg.TEST.AUG: multi-scale + flip inference, merged on the device
        self.sliced = None                      # cfg.TEST.SLICE: overlapping tiles at the model's test size, merged on the device
        if cfg.TEST.SLICE.ENABLED:              # refuses TEST.AUG.ENABLED beside it
            from .modeling.sliced_inference import SlicedInference
            self.sliced = SlicedInference(cfg, self.model)
        if cfg.TEST.AUG.ENABLED:
            from .modeling.test_time_augmentation import GeneralizedRCNNWithTTA
            self.tta = GeneralizedRCNNWithTTA(cfg, self.model)

    def _upload(self, image) -> torch.Tensor:
        if not torch.is_tensor(image):
            import numpy as np
            if not isinstance(image, np.ndarray):
                raise _lib.CmkError("Predictor: need an (h,w,3) uint8 numpy array or torch tensor, got {}".format(type(image).__name__))
            image = torch.from_numpy(np.ascontiguousarray(image))
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            raise _lib.CmkError("Predictor: need an (h,w,3) uint8 image, got {} {}; float images take another resize in detectron2 "
                                "and are not supported".format(image.dtype, tuple(image.shape)))
        return image.to(self.model.device)

    @torch.no_grad()
    def predict_batch(self, images: Sequence) -> List[Dict[str, Instances]]:
        """One model call over raw BGR images that may differ in size; results at each image's own resolution."""
        raw = [self._upload(im) for im in images]
        if self.sliced is not None:
            return [{"instances": self.sliced.inference_one_image(im, int(im.shape[0]), int(im.shape[1]),
                                                                  reverse_channels=self.input_format == "RGB")} for im in raw]
        if self.tta is not None:
            return [{"instances": self.tta.inference_one_image(im, int(im.shape[0]), int(im.shape[1]),
                                                               reverse_channels=self.input_format == "RGB")} for im in raw]
        model = self.model
        batch, sizes = ops.resize_preprocess_images(raw, self.min_size, self.max_size, model.pixel_mean.flatten().tolist(),
                                                    model.pixel_std.flatten().tolist(), model.backbone.size_divisibility,
                                                    reverse_channels=self.input_format == "RGB")
        results = model.inference(ImageList(batch, sizes), do_preprocess=False, do_postprocess=False)
        return [{"instances": detector_postprocess_d2(r, int(im.shape[0]), int(im.shape[1]))} for r, im in zip(results, raw)]

    def __call__(self, image) -> Dict[str, Instances]:
        return self.predict_batch([image])[0]
