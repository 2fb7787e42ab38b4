"""See a detection: boxes, masks, labels and keypoints drawn onto the image on the device (csrc/visualize.hip).

    vis = Visualizer(class_names=COCO_CLASSES)
    out = vis.draw(image_bgr_u8, pred(image_bgr_u8)["instances"])      # a new (h,w,3) uint8 tensor on the GPU
    write_png("out.png", out)

The reference's visualizer.py:21-38 hands the Instances to detectron2's Visualizer.draw_instance_predictions, which draws on the host with
matplotlib.  The picture here follows that call in ColorMode.IMAGE (largest instance first; box, half-transparent mask with an outline,
"NAME score%" on a dark plate, keypoints on top) but is this package's own: every step is integer arithmetic (DESIGN §3 "Visualizer"), not
anti-aliased, and unpinned against a real detectron2.  The pasted bitmasks never leave the device, and `draw` does not synchronise with
the host for GPU inputs: it can be captured in a torch.cuda.graph once the tables of a device are uploaded (by the first `draw` there).
No imaging library is used: write_png is zlib + struct, read_ppm reads binary P6."""
import colorsys
import math
import struct
import zlib
from typing import List, Optional, Sequence

import torch

from . import ops
from ._lib import CmkError
from .structures import Instances

__all__ = ["Visualizer", "draw_instance_predictions", "write_png", "write_ppm", "read_ppm", "COCO_CLASSES", "COCO_PERSON_SKELETON", "FONT_CHARS", "FONT_5X7",
           "PALETTE_RGB", "KEYPOINT_RGB", "label_glyphs"]

COCO_CLASSES = (
    "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light", "fire hydrant", "stop sign",
    "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow", "elephant", "bear", "zebra", "giraffe", "backpack", "umbrella",
    "handbag", "tie", "suitcase", "frisbee", "skis", "snowboard", "sports ball", "kite", "baseball bat", "baseball glove", "skateboard",
    "surfboard", "tennis racket", "bottle", "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple", "sandwich", "orange",
    "broccoli", "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch", "potted plant", "bed", "dining table", "toilet", "tv",
    "laptop", "mouse", "remote", "keyboard", "cell phone", "microwave", "oven", "toaster", "sink", "refrigerator", "book", "clock", "vase",
    "scissors", "teddy bear", "hair drier", "toothbrush")

# the "skeleton" of COCO's person_keypoints annotations, zero-based
COCO_PERSON_SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10), (1, 2),
                        (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))

# 5x7 font: per glyph 7 rows top to bottom, bit 4 of a row is its left column.  Any character outside FONT_CHARS draws "?".
FONT_CHARS = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ%.-?"
FONT_5X7 = (
    (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00),  # space
    (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E),  # 0
    (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),  # 1
    (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),  # 2
    (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E),  # 3
    (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02),  # 4
    (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),  # 5
    (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E),  # 6
    (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),  # 7
    (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),  # 8
    (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C),  # 9
    (0x0E, 0x11, 0x11, 0x11, 0x1F, 0x11, 0x11),  # A
    (0x1E, 0x11, 0x11, 0x1E, 0x11, 0x11, 0x1E),  # B
    (0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E),  # C
    (0x1C, 0x12, 0x11, 0x11, 0x11, 0x12, 0x1C),  # D
    (0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x1F),  # E
    (0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x10),  # F
    (0x0E, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0F),  # G
    (0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11),  # H
    (0x0E, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E),  # I
    (0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C),  # J
    (0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11),  # K
    (0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F),  # L
    (0x11, 0x1B, 0x15, 0x15, 0x11, 0x11, 0x11),  # M
    (0x11, 0x11, 0x19, 0x15, 0x13, 0x11, 0x11),  # N
    (0x0E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),  # O
    (0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10),  # P
    (0x0E, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0D),  # Q
    (0x1E, 0x11, 0x11, 0x1E, 0x14, 0x12, 0x11),  # R
    (0x0F, 0x10, 0x10, 0x0E, 0x01, 0x01, 0x1E),  # S
    (0x1F, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04),  # T
    (0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),  # U
    (0x11, 0x11, 0x11, 0x11, 0x11, 0x0A, 0x04),  # V
    (0x11, 0x11, 0x11, 0x15, 0x15, 0x15, 0x0A),  # W
    (0x11, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0x11),  # X
    (0x11, 0x11, 0x11, 0x0A, 0x04, 0x04, 0x04),  # Y
    (0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F),  # Z
    (0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03),  # %
    (0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C),  # .
    (0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00),  # -
    (0x0E, 0x11, 0x01, 0x02, 0x04, 0x00, 0x04),  # ?
)
_GLYPH_OF = {c: i for i, c in enumerate(FONT_CHARS)}
MAX_LABEL = 32


def _palette():
    """64 colours: golden-ratio hues at fixed saturation and value, float64, rounded."""
    out = []
    for i in range(64):
        r, g, b = colorsys.hsv_to_rgb((i * 0.6180339887498949) % 1.0, 0.75, 0.95)
        out.append((int(math.floor(r * 255.0 + 0.5)), int(math.floor(g * 255.0 + 0.5)), int(math.floor(b * 255.0 + 0.5))))
    return tuple(out)


PALETTE_RGB = _palette()
KEYPOINT_RGB = (255, 0, 0)


def label_glyphs(text: str) -> List[int]:
    """Upper-case, cut to 32 characters, every character outside the font becomes "?": the glyph indices a label draws."""
    return [_GLYPH_OF.get(c, _GLYPH_OF["?"]) for c in text.upper()[:MAX_LABEL]]


def _default_width(h: int, w: int, per: int) -> int:
    return max(1, int(math.floor(min(h, w) / per + 0.5)))


class Visualizer:
    """class_names: names by class id (None: "C<id>"); alpha: mask opacity; line_width / font_scale: integers, by default
    max(1, round(min(h,w)/400)) / max(1, round(min(h,w)/500)); color_by: "instance" or "class"; skeleton: pairs of keypoint indices
    (None: COCO_PERSON_SKELETON for 17 keypoints, no segments otherwise); input_format: the image's channel order, "BGR" or "RGB"."""

    def __init__(self, class_names: Optional[Sequence[str]] = None, alpha: float = 0.5, line_width: Optional[int] = None,
                 font_scale: Optional[int] = None, color_by: str = "instance", keypoint_threshold: float = 0.05, skeleton=None,
                 input_format: str = "BGR"):
        if color_by not in ("instance", "class"):
            raise CmkError("Visualizer: color_by must be 'instance' or 'class', got {!r}".format(color_by))
        if input_format not in ("BGR", "RGB"):
            raise CmkError("Visualizer: input_format must be BGR or RGB, got {!r}".format(input_format))
        self.alpha256 = int(math.floor(float(alpha) * 256.0 + 0.5)) if alpha == alpha else -1
        if not 0 <= self.alpha256 <= 256:
            raise CmkError("Visualizer: alpha = {} outside [0, 1]".format(alpha))
        for name, v in (("line_width", line_width), ("font_scale", font_scale)):
            if v is not None and (int(v) != v or not 1 <= int(v) <= 16):
                raise CmkError("Visualizer: {} = {} is not an integer in [1, 16]".format(name, v))
        self.class_names = None if class_names is None else [str(s) for s in class_names]
        if self.class_names is not None and len(self.class_names) > 65535:
            raise CmkError("Visualizer: {} class names, at most 65535".format(len(self.class_names)))
        self.line_width = None if line_width is None else int(line_width)
        self.font_scale = None if font_scale is None else int(font_scale)
        self.color_by = color_by
        self.keypoint_threshold = float(keypoint_threshold)
        self.skeleton = None if skeleton is None else [(int(a), int(b)) for a, b in skeleton]
        if self.skeleton is not None and len(self.skeleton) > 4096:
            raise CmkError("Visualizer: {} skeleton segments, at most 4096".format(len(self.skeleton)))
        self.input_format = input_format
        self._tables = {}                                           # device -> uploaded palette, font, names, skeletons

    # ---- host data, uploaded once per device -------------------------------------------------------------------------------------
    def _channel_order(self, rgb):
        return tuple(rgb[::-1]) if self.input_format == "BGR" else tuple(rgb)

    def _device_tables(self, dev: torch.device):
        t = self._tables.get(dev)
        if t is None:
            names = self.class_names or []
            rows = torch.zeros((max(len(names), 1), MAX_LABEL), dtype=torch.uint8)
            lens = torch.zeros((max(len(names), 1),), dtype=torch.int32)
            for i, s in enumerate(names):
                g = label_glyphs(s)
                rows[i, :len(g)] = torch.tensor(g, dtype=torch.uint8)
                lens[i] = len(g)
            t = {"palette": torch.tensor([self._channel_order(c) for c in PALETTE_RGB], dtype=torch.uint8).to(dev),
                 "font": torch.tensor(FONT_5X7, dtype=torch.uint8).to(dev),
                 "names": rows.to(dev), "name_lens": lens.to(dev), "num_names": len(names), "skeleton": {}}
            self._tables[dev] = t
        return t

    def _device_skeleton(self, t, k: int, dev: torch.device):
        sk = t["skeleton"].get(k)
        if sk is None:
            pairs = self.skeleton if self.skeleton is not None else (list(COCO_PERSON_SKELETON) if k == 17 else [])
            for a, b in pairs:
                if not (0 <= a < k and 0 <= b < k):
                    raise CmkError("Visualizer: skeleton pair ({}, {}) names a keypoint outside the {} of pred_keypoints".format(a, b, k))
            sk = (torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(dev), len(pairs))
            t["skeleton"][k] = sk
        return sk

    # ---- drawing -----------------------------------------------------------------------------------------------------------------
    def _color_ids(self, instances, boxes, classes, words, areas, h, w):
        """The colour index per instance, (n,) int32 on the device, or None for color_by's rule.  Called once per draw, empty frames
        included, with the frame's float32 boxes, int64 classes and packed masks (video.VideoVisualizer tracks here)."""
        return None

    def draw(self, image, instances: Instances) -> torch.Tensor:
        """-> a new (h,w,3) uint8 tensor on the instances' device; `image` is left as it is."""
        if not isinstance(instances, Instances) or not instances.has("pred_boxes") or not instances.has("scores") or not instances.has("pred_classes"):
            raise CmkError("Visualizer.draw: need Instances with pred_boxes, scores and pred_classes")
        boxes = instances.pred_boxes.tensor
        if not boxes.is_cuda:
            raise CmkError("Visualizer.draw: the Instances are on {} with boxes {}; the visualizer runs on the GPU (no CPU fallback)".format(
                boxes.device, tuple(boxes.shape)))
        dev = boxes.device
        ops._need_current_device(boxes, "Visualizer.draw")
        if not torch.is_tensor(image):
            import numpy as np
            if not isinstance(image, np.ndarray):
                raise CmkError("Visualizer.draw: need an (h,w,3) uint8 numpy array or torch tensor, got {}".format(type(image).__name__))
            image = torch.from_numpy(np.ascontiguousarray(image))
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
            raise CmkError("Visualizer.draw: need an (h,w,3) uint8 image, got {} {}".format(image.dtype, tuple(image.shape)))
        if image.is_cuda and image.device != dev:
            raise CmkError("Visualizer.draw: the image is on {}, the Instances on {}".format(image.device, dev))
        image = image.to(dev).contiguous()
        h, w = int(image.shape[0]), int(image.shape[1])
        if tuple(int(v) for v in instances.image_size) != (h, w):
            raise CmkError("Visualizer.draw: the Instances are of a {}x{} image, this one is {}x{}".format(
                instances.image_size[0], instances.image_size[1], h, w))
        if h * w >= 2 ** 31 - 1:
            raise CmkError("Visualizer.draw: image {}x{} is outside what int32 pixel positions hold".format(h, w))
        n = int(boxes.shape[0])
        if n > 65535:
            raise CmkError("Visualizer.draw: {} instances (boxes {}), at most 65535".format(n, tuple(boxes.shape)))
        scores, classes = instances.scores, instances.pred_classes
        if tuple(boxes.shape) != (n, 4) or tuple(scores.shape) != (n,) or tuple(classes.shape) != (n,):
            raise CmkError("Visualizer.draw: boxes {}, scores {}, classes {} do not describe {} instances".format(
                tuple(boxes.shape), tuple(scores.shape), tuple(classes.shape), n))
        masks = instances.pred_masks if instances.has("pred_masks") else None
        if masks is not None and (masks.dtype != torch.bool or tuple(masks.shape) != (n, h, w) or masks.device != dev):
            raise CmkError("Visualizer.draw: pred_masks must be ({},{},{}) bool on {}, got {} {} on {}".format(
                n, h, w, dev, tuple(masks.shape), masks.dtype, masks.device))
        kps = instances.pred_keypoints if instances.has("pred_keypoints") else None
        if kps is not None and (kps.dim() != 3 or kps.shape[0] != n or kps.shape[2] != 3 or not 1 <= kps.shape[1] <= 1024 or kps.device != dev):
            raise CmkError("Visualizer.draw: pred_keypoints must be ({},K,3) with K in [1, 1024] on {}, got {} on {}".format(
                n, dev, tuple(kps.shape), kps.device))
        lw = self.line_width if self.line_width is not None else min(16, _default_width(h, w, 400))
        fs = self.font_scale if self.font_scale is not None else min(16, _default_width(h, w, 500))

        t = self._device_tables(dev)
        words = None
        if n:
            boxes = boxes.detach().to(torch.float32).contiguous()
            scores = scores.detach().to(device=dev, dtype=torch.float32).contiguous()
            classes = classes.detach().to(device=dev, dtype=torch.int64).contiguous()
            area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
            order = torch.sort(area, descending=True, stable=True).indices.contiguous()       # plumbing; everything else is the library's
            areas = None
            if masks is not None:
                words, areas = ops.mask_pack_bits(masks)
            color_ids = self._color_ids(instances, boxes, classes, words, areas, h, w)
            if color_ids is None:
                records = ops.vis_prepare(boxes, scores, classes, order, t["names"], t["name_lens"], t["num_names"], t["palette"], h, w, fs,
                                          self.color_by == "class")
            else:
                records = ops.vis_prepare_ids(boxes, scores, classes, order, t["names"], t["name_lens"], t["num_names"], t["palette"], h, w, fs,
                                              self.color_by == "class", color_ids)
        else:
            self._color_ids(instances, boxes.detach().to(torch.float32).reshape(0, 4), classes.detach().to(device=dev, dtype=torch.int64), None, None, h, w)
            records = t["font"].new_empty((0,), dtype=torch.int32)
        out = ops.vis_compose(image, words, records, n, t["font"], lw, fs, self.alpha256)
        if kps is not None and n:
            skel, nseg = self._device_skeleton(t, int(kps.shape[1]), dev)
            r, g, b = self._channel_order(KEYPOINT_RGB)
            ops.vis_keypoints(out, kps.detach().to(torch.float32).contiguous(), records, skel if nseg else None, self.keypoint_threshold, lw,
                              r | (g << 8) | (b << 16))
        return out

    def draw_batch(self, images: Sequence, instances: Sequence[Instances]) -> List[torch.Tensor]:
        if len(images) != len(instances):
            raise CmkError("Visualizer.draw_batch: {} images but {} Instances".format(len(images), len(instances)))
        return [self.draw(im, inst) for im, inst in zip(images, instances)]


def draw_instance_predictions(image, instances: Instances, **kw) -> torch.Tensor:
    """One-shot form of Visualizer(**kw).draw(image, instances) (visualizer.py:21-38)."""
    return Visualizer(**kw).draw(image, instances)


# ---- files, without an imaging library ---------------------------------------------------------------------------------------------
def _host_u8(image):
    import numpy as np
    if torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise CmkError("need an (h,w,3) uint8 image, got {} {}".format(image.dtype, image.shape))
    return image


def write_png(path: str, image, input_format: str = "BGR") -> None:
    """An (h,w,3) uint8 image (tensor or array) -> 8-bit RGB PNG, filter 0 on every row."""
    if input_format not in ("BGR", "RGB"):
        raise CmkError("write_png: input_format must be BGR or RGB, got {!r}".format(input_format))
    import numpy as np
    img = _host_u8(image)
    if input_format == "BGR":
        img = img[:, :, ::-1]
    h, w = img.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 1:] = img.reshape(h, 3 * w)

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


def write_ppm(path: str, image, input_format: str = "BGR") -> None:
    """The counterpart of read_ppm: binary P6, maxval 255."""
    img = _host_u8(image)
    if input_format == "BGR":
        img = img[:, :, ::-1]
    with open(path, "wb") as f:
        f.write("P6\n{} {}\n255\n".format(img.shape[1], img.shape[0]).encode() + img.tobytes())


def read_ppm(path: str, output_format: str = "BGR"):
    """Binary P6 with maxval 255 -> (h,w,3) uint8 numpy array in `output_format` channel order."""
    import numpy as np
    data = open(path, "rb").read()
    tokens, pos = [], 0
    while len(tokens) < 4:                                          # magic, width, height, maxval; '#' comments run to the line's end
        while pos < len(data) and (data[pos:pos + 1].isspace() or data[pos:pos + 1] == b"#"):
            if data[pos:pos + 1] == b"#":
                while pos < len(data) and data[pos:pos + 1] != b"\n":
                    pos += 1
            else:
                pos += 1
        start = pos
        while pos < len(data) and not data[pos:pos + 1].isspace():
            pos += 1
        if start == pos:
            raise CmkError("read_ppm: {} ends inside its header".format(path))
        tokens.append(data[start:pos])
    pos += 1                                                        # the single whitespace after maxval
    try:
        w, h, maxval = int(tokens[1]), int(tokens[2]), int(tokens[3])
    except ValueError:
        raise CmkError("read_ppm: {} has a malformed header {}".format(path, tokens)) from None
    if tokens[0] != b"P6" or maxval != 255 or w < 1 or h < 1:
        raise CmkError("read_ppm: {} is not a binary P6 with maxval 255 (header {})".format(path, tokens))
    if len(data) - pos < 3 * w * h:
        raise CmkError("read_ppm: {} holds {} pixel bytes, a {}x{} image needs {}".format(path, len(data) - pos, w, h, 3 * w * h))
    img = np.frombuffer(data, dtype=np.uint8, count=3 * w * h, offset=pos).reshape(h, w, 3)
    return np.ascontiguousarray(img[:, :, ::-1] if output_format == "BGR" else img)
