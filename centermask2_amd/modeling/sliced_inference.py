"""Sliced inference, cfg.TEST.SLICE: a large image cut into overlapping tiles, every tile run at the model's own test size, the
detections merged in the image frame.  No detectron2 counterpart; the scheme is the published one of slicing-aided inference.

Per image (DESIGN §3 "Sliced inference"): the tiles of ops.slice_grid, all of one size, cropped on the device and resized by the ordinary
ResizeShortestEdge(INPUT.MIN_SIZE_TEST, MAX_SIZE_TEST) rule, BATCH tiles per model call; with FULL_IMAGE the whole image as one more pass
of batch 1 after the tiles.  Every pass is the whole model: backbone, FCOS, the RoI heads with soft masks and mask scores.  The padded
detections of all passes are mapped into the image frame (cmk_slice_boxes_to_image) and merged by one class-wise NMS on MATCH_METRIC at
MATCH_THRESH (cmk_nms_topk_metric), keeping TEST.DETECTIONS_PER_IMAGE.  A survivor keeps the soft mask and the mask score of its own
pass, gathered through the source slots the two kernels hand back; the mask head is not run again.  The host reads one
candidate-overflow word and the merged count.
"""
from typing import Dict, List

import torch

from .. import ops
from ..postprocess import detector_postprocess_d2
from ..structures import Boxes, Instances

__all__ = ["SlicedInference"]


class SlicedInference:
    def __init__(self, cfg, model):
        sl = cfg.TEST.SLICE
        if cfg.MODEL.KEYPOINT_ON:
            raise NotImplementedError("MODEL.KEYPOINT_ON with TEST.SLICE: sliced inference has no keypoint merge; turn one of them off")
        if cfg.TEST.AUG.ENABLED and sl.ENABLED:
            raise NotImplementedError("TEST.SLICE.ENABLED together with TEST.AUG.ENABLED: one of the two merges per image; turn one of them off")
        self.topk = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        if not 1 <= self.topk <= 1024:
            raise NotImplementedError("TEST.DETECTIONS_PER_IMAGE must be in [1, 1024] for TEST.SLICE (the merge NMS keeps its list in LDS), "
                                      "got {}".format(self.topk))
        tile = tuple(sl.TILE)
        if len(tile) != 2 or any(int(t) != t or int(t) < 1 for t in tile):
            raise ValueError("TEST.SLICE.TILE must be two positive integers (h, w), got {!r}".format(sl.TILE))
        self.tile = (int(tile[0]), int(tile[1]))
        self.overlap = float(sl.OVERLAP)
        if not 0.0 <= self.overlap < 1.0:
            raise ValueError("TEST.SLICE.OVERLAP must be in [0, 1), got {!r}".format(sl.OVERLAP))
        self.batch = int(sl.BATCH)
        if self.batch < 1:
            raise ValueError("TEST.SLICE.BATCH must be at least 1, got {!r}".format(sl.BATCH))
        if sl.MATCH_METRIC not in ("IOS", "IOU"):
            raise ValueError("TEST.SLICE.MATCH_METRIC must be \"IOS\" or \"IOU\", got {!r}".format(sl.MATCH_METRIC))
        self.metric = sl.MATCH_METRIC.lower()
        self.match_thresh = float(sl.MATCH_THRESH)
        self.full_image = bool(sl.FULL_IMAGE)
        self.min_size = int(cfg.INPUT.MIN_SIZE_TEST)
        self.max_size = int(cfg.INPUT.MAX_SIZE_TEST)
        for need, part in (("forward_padded", model.proposal_generator), ("forward_padded", model.roi_heads)):
            if not hasattr(part, need):
                raise NotImplementedError("TEST.SLICE needs a detector with device-side {}(), {} has none".format(need, type(part).__name__))
        self.mask_on = bool(cfg.MODEL.MASK_ON)
        self.cfg = cfg
        self.model = model.eval()
        self._tables = {}

    def passes(self, h: int, w: int):
        """[(y0, x0, th, tw, new_h, new_w)]: the tiles in row-major order, then (FULL_IMAGE) the whole image."""
        out = [(y0, x0, th, tw) + ops.resize_shortest_edge_shape(th, tw, self.min_size, self.max_size)
               for y0, x0, th, tw in ops.slice_grid(h, w, self.tile[0], self.tile[1], self.overlap)]
        if self.full_image:
            out.append((0, 0, h, w) + ops.resize_shortest_edge_shape(h, w, self.min_size, self.max_size))
        return out

    def _geometry(self, h: int, w: int, dev):
        key = (h, w, str(dev))
        g = self._tables.get(key)
        if g is None:                           # uploaded once per image size
            passes = self.passes(h, w)
            g = self._tables[key] = (passes, ops.slice_table(passes, dev))
        return g

    def _run(self, images, reverse_channels: bool) -> dict:
        """One model call over raw crops of one size: the padded outputs of GeneralizedRCNN.inference_padded."""
        model = self.model
        batch, sizes = ops.resize_preprocess_images(images, self.min_size, self.max_size, model.pixel_mean.flatten().tolist(),
                                                    model.pixel_std.flatten().tolist(), model.backbone.size_divisibility,
                                                    reverse_channels=reverse_channels)
        features = model.backbone(batch)
        det, _ = model.proposal_generator.forward_padded(features)
        out = model.roi_heads.forward_padded(features, det, sizes)
        out["_redo"] = lambda det2: model.roi_heads.forward_padded(features, det2, sizes)
        return out

    def merge(self, det: dict, table: torch.Tensor, h: int, w: int):
        """The padded (A,K,..) detections of all passes -> (the candidate set in the image frame, the merged padded detections)."""
        cand = ops.slice_boxes_to_image(det, table, h, w)
        return cand, ops.nms_topk(cand, self.match_thresh, self.topk, metric=self.metric)

    @torch.no_grad()
    def merged_instances(self, image: torch.Tensor, reverse_channels: bool = False) -> Instances:
        """image: (h,w,3) uint8 on the model's device with its channels in the model's order unless reverse_channels.  The merged
        detections in the image's own frame, each with the SOFT mask (n,1,S,S) and the mask score of the pass that found it, before
        the paste."""
        h, w = int(image.shape[0]), int(image.shape[1])
        passes, table = self._geometry(h, w, image.device)
        tiles = passes[:-1] if self.full_image else passes
        crops = [image[y0:y0 + th, x0:x0 + tw].contiguous() for y0, x0, th, tw, _, _ in tiles]
        outs = [self._run(crops[i:i + self.batch], reverse_channels) for i in range(0, len(crops), self.batch)]
        if self.full_image:
            outs.append(self._run([image], reverse_channels))
        if "cand_capacity" in outs[0]:          # the detector's overflow rule, one host read for all chunks
            fcos = self.model.proposal_generator
            worst = torch.stack([o["cand_counts"].max() for o in outs]).cpu().tolist()
            outs = [o["_redo"](fcos.resolve_overflow(o)) if n > o["cand_capacity"] else o for o, n in zip(outs, worst)]
        det = {k: torch.cat([o[k] for o in outs]) for k in ("box", "score", "cls", "loc", "counts")}
        cand, merged = self.merge(det, table, h, w)
        n = int(merged["counts"][0])
        res = Instances((h, w))
        res.pred_boxes = Boxes(merged["box"][0, :n])
        res.scores = merged["score"][0, :n]
        res.pred_classes = merged["cls"][0, :n]
        res.locations = merged["loc"][0, :n]
        if self.mask_on:                        # the padded slot a*K + k every survivor came from
            src = cand["src"].index_select(0, merged["idx"][0, :n].long()).long()
            masks = torch.cat([o["pred_masks"] for o in outs])
            res.pred_masks = masks.reshape((-1,) + tuple(masks.shape[2:])).index_select(0, src)
            if "mask_scores" in outs[0]:
                res.mask_scores = torch.cat([o["mask_scores"] for o in outs]).reshape(-1).index_select(0, src)
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
                raise ops._lib.CmkError("SlicedInference: need a (3,h,w) uint8 image tensor, got {}".format(
                    "{} {}".format(im.dtype, tuple(im.shape)) if torch.is_tensor(im) else type(im).__name__))
            hwc = im.to(self.model.device).permute(1, 2, 0).contiguous()
            out.append({"instances": self.inference_one_image(hwc, x.get("height", im.shape[1]), x.get("width", im.shape[2]))})
        return out
