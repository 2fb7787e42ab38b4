"""Video mode: instance ids that follow objects from frame to frame, and a visualizer that colours by them (csrc/visualize.hip).

    vis = VideoVisualizer(class_names=COCO_CLASSES)
    for frame in frames:
        out = vis.draw(frame, pred(frame)["instances"])            # the same object keeps its colour; instances.track_ids holds the ids

The reference's demo.py --video-input draws with detectron2's VideoVisualizer, whose _assign_colors matches every frame's instances to the
previous frame's by IoU on the host.  The rule here is that one (DESIGN §3 "Video"; the C contract is in include/cmk.h), but the track
table, the IoU table, the matching and the counters stay on the device: `update` and `draw` launch a fixed sequence of kernels on the
current stream and read nothing back.  This project's own choices: mask IoU is an option beside box IoU, ids are
deterministic (next_id counts up) and a colour is palette[id mod 64] instead of a random one, and nothing is pinned against a real
detectron2."""
from typing import Optional

import torch

from . import ops
from ._lib import CmkError
from .structures import Instances
from .visualize import Visualizer

__all__ = ["InstanceTracker", "VideoVisualizer"]

BOX_IOU_THRESHOLD = 0.6          # detectron2's VideoVisualizer: boxes
MASK_IOU_THRESHOLD = 0.5         # ... and masks


class InstanceTracker:
    """match: "box" (IoU of the boxes) or "mask" (IoU of the pasted bitmasks, from packed bits); iou_threshold: None for detectron2's
    0.6 / 0.5; ttl: a track that is not matched for `ttl` frames in a row is forgotten; max_tracks: rows of the table (1..1024), also the
    most instances one frame may hold.  Mask mode keeps 2 * max_tracks packed masks of the frame's size on the device."""

    def __init__(self, match: str = "box", iou_threshold: Optional[float] = None, ttl: int = 8, max_tracks: int = 256):
        if match not in ("box", "mask"):
            raise CmkError("InstanceTracker: match must be 'box' or 'mask', got {!r}".format(match))
        if iou_threshold is None:
            iou_threshold = BOX_IOU_THRESHOLD if match == "box" else MASK_IOU_THRESHOLD
        if not 0.0 <= float(iou_threshold) <= 1.0:
            raise CmkError("InstanceTracker: iou_threshold = {} outside [0, 1]".format(iou_threshold))
        if int(ttl) != ttl or not 1 <= int(ttl) <= 255:
            raise CmkError("InstanceTracker: ttl = {} is not an integer in [1, 255]".format(ttl))
        if int(max_tracks) != max_tracks or not 1 <= int(max_tracks) <= ops.MAX_TRACKS:
            raise CmkError("InstanceTracker: max_tracks = {} is not an integer in [1, {}]".format(max_tracks, ops.MAX_TRACKS))
        self.match, self.iou_threshold, self.ttl, self.max_tracks = match, float(iou_threshold), int(ttl), int(max_tracks)
        self._state = None                                          # allocated by the first update, on its device
        self.frame_size = None                                      # mask mode: the (h, w) the table's masks have

    # ---- state -----------------------------------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """Forget every track; ids start again at 0.  The next frame may have another size.  Only the counters are cleared: rows at or
        beyond n_tracks are never read."""
        self.frame_size = None
        s = self._state
        if s is not None:
            s["counters"].zero_()
            s["bound"] = 0

    def _half(self, dev, nw):
        cap = self.max_tracks
        half = {"boxes": torch.zeros((cap, 4), dtype=torch.float32, device=dev), "classes": torch.zeros((cap,), dtype=torch.int64, device=dev),
                "ids": torch.zeros((cap,), dtype=torch.int32, device=dev), "ttl": torch.zeros((cap,), dtype=torch.int32, device=dev)}
        if nw is not None:
            half["words"] = torch.zeros((cap, nw), dtype=torch.int64, device=dev)
            half["areas"] = torch.zeros((cap,), dtype=torch.int32, device=dev)
        return half

    def _device_state(self, dev):
        s = self._state
        if s is not None and s["device"] != dev:
            raise CmkError("InstanceTracker: the table is on {}, this frame on {}; reset() does not move it, use one tracker per device".format(
                s["device"], dev))
        if s is None:
            cap = self.max_tracks
            s = {"device": dev, "halves": [self._half(dev, None), self._half(dev, None)], "cur": 0, "bound": 0,
                 "counters": torch.zeros((4,), dtype=torch.int32, device=dev), "src": torch.zeros((cap,), dtype=torch.int32, device=dev),
                 "table": torch.zeros((cap * cap,), dtype=torch.float64 if self.match == "box" else torch.int32, device=dev)}
            self._state = s
        return s

    def table(self) -> dict:
        """The current table's device tensors (boxes, classes, ids, ttl and, in mask mode, words and areas; the first n_tracks rows are
        live) and `counters` (n_tracks, next_id, dropped, spare).  Views, not copies: the next update rewrites the other half."""
        if self._state is None:
            return {}
        return dict(self._state["halves"][self._state["cur"]], counters=self._state["counters"])

    def _counter(self, k: int) -> int:
        return 0 if self._state is None else int(self._state["counters"][k])

    @property
    def n_tracks(self) -> int:
        """Rows of the table in use.  Reading it synchronises with the device; `update` never does."""
        return self._counter(0)

    @property
    def next_id(self) -> int:
        return self._counter(1)

    @property
    def dropped(self) -> int:
        """Surviving tracks that found no room in max_tracks rows, so far (a device-side counter, read here)."""
        return self._counter(2)

    # ---- one frame -------------------------------------------------------------------------------------------------------------------
    def update(self, instances: Instances, words: Optional[torch.Tensor] = None, areas: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Match this frame's instances to the table -> track_ids (n,) int32 on the device, also set as instances.track_ids.  Mask mode
        packs instances.pred_masks ((n,h,w) bool) unless the caller hands in the (words, areas) of ops.mask_pack_bits."""
        if not isinstance(instances, Instances) or not instances.has("pred_boxes") or not instances.has("pred_classes"):
            raise CmkError("InstanceTracker.update: need Instances with pred_boxes and pred_classes")
        boxes = instances.pred_boxes.tensor
        if self.match == "mask" and words is None and not instances.has("pred_masks"):
            raise CmkError("InstanceTracker.update: match='mask' needs pred_masks (or packed words and areas)")
        if boxes.shape[0] > self.max_tracks:
            raise CmkError("InstanceTracker.update: {} instances (boxes {}) but max_tracks = {}".format(boxes.shape[0], tuple(boxes.shape), self.max_tracks))
        if not boxes.is_cuda:
            raise CmkError("InstanceTracker.update: the Instances are on {} with boxes {}; the tracker runs on the GPU (no CPU fallback)".format(
                boxes.device, tuple(boxes.shape)))
        ops._need_current_device(boxes, "InstanceTracker.update")
        dev, n = boxes.device, int(boxes.shape[0])
        classes = instances.pred_classes
        if tuple(boxes.shape) != (n, 4) or tuple(classes.shape) != (n,):
            raise CmkError("InstanceTracker.update: boxes {} and classes {} do not describe {} instances".format(tuple(boxes.shape), tuple(classes.shape), n))
        boxes = boxes.detach().to(torch.float32).contiguous()
        classes = classes.detach().to(device=dev, dtype=torch.int64).contiguous()
        track_ids = self._update(boxes, classes, instances, words, areas, tuple(int(v) for v in instances.image_size))
        instances.track_ids = track_ids
        return track_ids

    def _update(self, boxes, classes, instances, words, areas, size):
        dev, n, cap = boxes.device, int(boxes.shape[0]), self.max_tracks
        s = self._device_state(dev)
        old, out = s["halves"][s["cur"]], s["halves"][1 - s["cur"]]
        rows = s["bound"]                                           # n_tracks <= rows, known without reading the counter
        bound = min(cap, n + rows)
        if self.match == "mask":
            h, w = size
            if words is None:
                if instances is None or not instances.has("pred_masks"):
                    raise CmkError("InstanceTracker.update: match='mask' needs pred_masks (or packed words and areas)")
                masks = instances.pred_masks
                if masks.dtype != torch.bool or tuple(masks.shape) != (n, h, w) or masks.device != dev:
                    raise CmkError("InstanceTracker.update: pred_masks must be ({},{},{}) bool on {}, got {} {} on {}".format(
                        n, h, w, dev, tuple(masks.shape), masks.dtype, masks.device))
                words, areas = ops.mask_pack_bits(masks)
            nw = ops.mask_words(h, w)
            if areas is None or not torch.is_tensor(words) or tuple(words.shape) != (n, nw) or tuple(areas.shape) != (n,):
                raise CmkError("InstanceTracker.update: words must be ({}, {}) int64 with areas ({},) int32 for a {}x{} frame".format(n, nw, n, h, w))
            if self.frame_size is None:
                self.frame_size = (h, w)
                for half in s["halves"]:
                    if "words" not in half or half["words"].shape[1] != nw:
                        half["words"] = torch.zeros((cap, nw), dtype=torch.int64, device=dev)
                        half["areas"] = torch.zeros((cap,), dtype=torch.int32, device=dev)
            elif self.frame_size != (h, w):
                raise CmkError("InstanceTracker.update: this frame is {}x{}, the tracked masks are {}x{}; call reset() when the frame size changes".format(
                    h, w, self.frame_size[0], self.frame_size[1]))
            if n and rows:
                ops.check(ops._lib.load().cmk_mask_intersections(old["words"].data_ptr(), rows, words.data_ptr(), n, h, w, s["table"].data_ptr(),
                                                                 ops._stream()), "cmk_mask_intersections")
            track_ids = ops.vis_track_assign(old, out, boxes, classes, rows, self.ttl, self.iou_threshold, s["src"], s["counters"],
                                             inter=s["table"], new_areas=areas)
            ops.vis_track_gather(s["src"], s["counters"], old, out, words, areas, bound, h, w)
        else:
            ops.vis_track_iou_boxes(old["boxes"], rows, boxes, s["table"])
            track_ids = ops.vis_track_assign(old, out, boxes, classes, rows, self.ttl, self.iou_threshold, s["src"], s["counters"], iou=s["table"])
        s["cur"], s["bound"] = 1 - s["cur"], bound
        return track_ids


class VideoVisualizer(Visualizer):
    """A Visualizer that owns an InstanceTracker: `draw` matches the frame's instances to the earlier frames' and colours every instance
    by its track id (palette[id mod 64]), so an object keeps its colour while the detector's output order changes.  The masks are packed
    once for the tracker and the picture.  match / iou_threshold / ttl / max_tracks are the tracker's; everything else is Visualizer's
    (color_by is not consulted).  After a draw, instances.track_ids holds the ids."""

    def __init__(self, *args, match: str = "box", iou_threshold: Optional[float] = None, ttl: int = 8, max_tracks: int = 256, **kw):
        super().__init__(*args, **kw)
        self.tracker = InstanceTracker(match=match, iou_threshold=iou_threshold, ttl=ttl, max_tracks=max_tracks)

    def reset(self) -> None:
        self.tracker.reset()

    def _color_ids(self, instances, boxes, classes, words, areas, h, w):
        n = int(boxes.shape[0])
        if n > self.tracker.max_tracks:
            raise CmkError("VideoVisualizer.draw: {} instances (boxes {}) but max_tracks = {}".format(n, tuple(boxes.shape), self.tracker.max_tracks))
        if self.tracker.match == "mask" and n and words is None:
            raise CmkError("VideoVisualizer.draw: match='mask' needs pred_masks")
        if self.tracker.match == "mask" and words is None:        # an empty frame without masks still ages the table
            words = boxes.new_zeros((0, ops.mask_words(h, w)), dtype=torch.int64)
            areas = boxes.new_zeros((0,), dtype=torch.int32)
        track_ids = self.tracker._update(boxes, classes, None, words, areas, (h, w))
        instances.track_ids = track_ids
        return track_ids
