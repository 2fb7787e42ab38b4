"""Test-time augmentation, cfg.TEST.AUG: detectron2's GeneralizedRCNNWithTTA (modeling/test_time_augmentation.py, source absent:
restated from its published behaviour) for the CenterMask detector.

Per image (DESIGN §3 "Test-time augmentation"): the image at every TEST.AUG.MIN_SIZES scale, plain and (FLIP) mirrored, each scale one
batch of two; FCOS detections of every augmentation mapped back to the image frame and merged by one class-wise NMS; the mask head run
on the merged boxes mapped into every augmentation's frame; the soft masks (flipped back) and the mask scores averaged.  detectron2 runs
the backbone a second time per augmentation for the mask pass; here the feature maps of the first pass stay on the device and are reused.
Everything between the raw bytes and the pasted bitmasks is on the device; the host reads one candidate-overflow word and the merged count.
"""
from typing import Dict, List, Tuple

import torch

from .. import ops
from ..postprocess import detector_postprocess_d2
from ..structures import Boxes, Instances

__all__ = ["GeneralizedRCNNWithTTA", "tta_augmentations"]


def tta_augmentations(h: int, w: int, min_sizes, max_size: int, flip: bool) -> List[Tuple[int, int, bool]]:
    """d2's DatasetMapperTTA order: [(new_h, new_w, flipped)] per MIN_SIZES entry the plain resize, then (FLIP) its mirror.  Repeated
    shapes are kept, as in d2."""
    augs = []
    for s in min_sizes:
        nh, nw = ops.resize_shortest_edge_shape(h, w, int(s), int(max_size))
        augs.append((nh, nw, False))
        if flip:
            augs.append((nh, nw, True))
    return augs


class GeneralizedRCNNWithTTA:
    def __init__(self, cfg, model):
        if cfg.MODEL.KEYPOINT_ON:
            raise NotImplementedError("MODEL.KEYPOINT_ON with TEST.AUG: detectron2's GeneralizedRCNNWithTTA has no keypoint merge; "
                                      "turn one of them off")
        self.topk = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        if not 1 <= self.topk <= 1024:
            raise NotImplementedError("TEST.DETECTIONS_PER_IMAGE must be in [1, 1024] for TEST.AUG (the merge NMS keeps its list in LDS), "
                                      "got {}".format(self.topk))
        self.min_sizes = tuple(int(s) for s in cfg.TEST.AUG.MIN_SIZES)
        self.max_size = int(cfg.TEST.AUG.MAX_SIZE)
        self.flip = bool(cfg.TEST.AUG.FLIP)
        if not self.min_sizes or min(self.min_sizes) < 1:
            raise ValueError("TEST.AUG.MIN_SIZES must name at least one positive size, got {!r}".format(cfg.TEST.AUG.MIN_SIZES))
        for need, part in (("forward_padded", model.proposal_generator), ("forward_padded", model.roi_heads)):
            if not hasattr(part, need):
                raise NotImplementedError("TEST.AUG needs a detector with device-side {}(), {} has none".format(need, type(part).__name__))
        # the merged boxes are FCOS's, so is the threshold: ROI_HEADS.NMS_THRESH_TEST belongs to a box head CenterROIHeads does not have
        self.nms_thresh = float(cfg.MODEL.FCOS.NMS_TH)
        self.mask_on = bool(cfg.MODEL.MASK_ON)
        self.cfg = cfg
        self.model = model.eval()
        self._tables = {}

    def _geometry(self, h: int, w: int, dev):
        key = (h, w, str(dev))
        g = self._tables.get(key)
        if g is None:                           # uploaded once per image size
            augs = tta_augmentations(h, w, self.min_sizes, self.max_size, self.flip)
            g = self._tables[key] = (augs, ops.tta_table(augs, h, w, True, dev), ops.tta_table(augs, h, w, False, dev),
                                     torch.tensor([int(f) for _, _, f in augs], dtype=torch.int32).to(dev))
        return g

    def _mask_features(self, i: int, canvases, feats):
        """Feature maps of scale batch i for the mask pass: the ones the detection pass computed.  (detectron2 runs the backbone again
        here; tools/bench_tta.py overrides this to measure that schedule.)"""
        return feats[i]

    @torch.no_grad()
    def merged_instances(self, image: torch.Tensor, reverse_channels: bool = False) -> Instances:
        """Steps 1-6 for image, (h,w,3) uint8 on the model's device with its channels in the model's order unless reverse_channels: the
        merged detections in the image's own frame with the averaged SOFT masks (n,1,S,S) and mask scores, before the paste."""
        model = self.model
        h, w = int(image.shape[0]), int(image.shape[1])
        augs, to_image, to_aug, flips = self._geometry(h, w, image.device)
        per = 2 if self.flip else 1
        shapes = [(nh, nw) for nh, nw, _ in augs[::per]]
        canvases = ops.resize_preprocess_augmented(image, shapes, self.flip, model.pixel_mean.flatten().tolist(),
                                                   model.pixel_std.flatten().tolist(), model.backbone.size_divisibility,
                                                   reverse_channels=reverse_channels)
        fcos = model.proposal_generator
        feats, dets = [], []
        for canvas in canvases:                 # one backbone pass per scale batch; its feature maps are kept for the mask pass
            f = model.backbone(canvas)
            feats.append(f)
            dets.append(fcos.forward_padded(f)[0])
        if "cand_capacity" in dets[0]:          # the detector's overflow rule, one host read for all scales
            worst = torch.stack([d["cand_counts"].max() for d in dets]).cpu().tolist()
            dets = [fcos.resolve_overflow(d) if n > d["cand_capacity"] else d for d, n in zip(dets, worst)]
        det = {k: torch.cat([d[k] for d in dets]) for k in ("box", "score", "cls", "loc", "counts")}
        merged = ops.nms_topk(ops.tta_boxes_to_image(det, to_image, h, w), self.nms_thresh, self.topk)
        red_masks = red_scores = None
        if self.mask_on:
            boxes, counts = ops.tta_boxes_to_aug(merged["box"][0], merged["counts"], to_aug)
            shared = {k: merged[k].expand(per, *merged[k].shape[1:]).contiguous() for k in ("score", "cls", "loc")}
            masks, scores = [], []
            for i, hw in enumerate(shapes):
                sl = slice(i * per, (i + 1) * per)
                out = model.roi_heads.forward_padded(self._mask_features(i, canvases, feats), dict(shared, box=boxes[sl], counts=counts[sl]), [hw] * per)
                masks.append(out["pred_masks"])
                scores.append(out.get("mask_scores"))
            masks = torch.cat(masks)
            s = int(masks.shape[-1])
            red_masks, red_scores = ops.tta_reduce_masks(masks.reshape(len(augs), self.topk, s, s), flips,
                                                         torch.cat(scores) if scores[0] is not None else None, merged["counts"])
        n = int(merged["counts"][0])
        res = Instances((h, w))
        res.pred_boxes = Boxes(merged["box"][0, :n])
        res.scores = merged["score"][0, :n]
        res.pred_classes = merged["cls"][0, :n]
        res.locations = merged["loc"][0, :n]
        if red_masks is not None:
            res.pred_masks = red_masks[:n].unsqueeze(1)
        if red_scores is not None:
            res.mask_scores = red_scores[:n]
        return res

    def inference_one_image(self, image: torch.Tensor, height: int, width: int, reverse_channels: bool = False) -> Instances:
        """merged_instances, then detectron2's detector_postprocess to height x width."""
        return detector_postprocess_d2(self.merged_instances(image, reverse_channels), int(height), int(width))

    def __call__(self, batched_inputs) -> List[Dict[str, Instances]]:
        """d2's mapper format: [{"image": (3,h,w) uint8 in INPUT.FORMAT order, "height", "width"}]; height and width default to the
        image's own size."""
        out = []
        for x in batched_inputs:
            im = x["image"]
            if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[0] != 3:
                raise ops._lib.CmkError("GeneralizedRCNNWithTTA: need a (3,h,w) uint8 image tensor, got {}".format(
                    "{} {}".format(im.dtype, tuple(im.shape)) if torch.is_tensor(im) else type(im).__name__))
            hwc = im.to(self.model.device).permute(1, 2, 0).contiguous()
            out.append({"instances": self.inference_one_image(hwc, x.get("height", im.shape[1]), x.get("width", im.shape[2]))})
        return out
