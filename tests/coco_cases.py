"""Hand-built COCO datasets and Instances shared by tests/test_cpu_coco_eval.py and tests/test_gpu_coco_eval.py (no test in here)."""
import numpy as np
import torch

from centermask2_amd import wire
from centermask2_amd.structures import Boxes, Instances


def rect_poly(x0, y0, x1, y1):
    return [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]


def rect_mask(h, w, x0, y0, x1, y1):
    m = np.zeros((h, w), dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


def ann(aid, img, cat, box, iscrowd=0, area=None, seg=None, **extra):
    """box = integer (x0, y0, x1, y1); the segmentation defaults to the rectangle as one polygon, the area to the rectangle's."""
    x0, y0, x1, y1 = box
    a = {"id": aid, "image_id": img, "category_id": cat, "bbox": [x0, y0, x1 - x0, y1 - y0], "iscrowd": iscrowd,
         "area": float((x1 - x0) * (y1 - y0)) if area is None else float(area),
         "segmentation": [rect_poly(*box)] if seg is None else seg}
    a.update(extra)
    return a


def dataset(sizes, anns, cats=(1,)):
    """sizes: {image id: (h, w)}."""
    return {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in sorted(sizes.items())],
            "categories": [{"id": c, "name": "c{}".format(c)} for c in cats], "annotations": list(anns)}


def instances(h, w, boxes, scores, classes=None, masks="rect", mask_scores=None):
    """Instances of integer xyxy boxes; masks="rect" -> each box's own rectangle, None -> no masks, else an (n,h,w) bool array."""
    n = len(boxes)
    inst = Instances((h, w), pred_boxes=Boxes(torch.tensor(boxes, dtype=torch.float32).reshape(n, 4)),
                     scores=torch.tensor(scores, dtype=torch.float32),
                     pred_classes=torch.tensor(classes if classes is not None else [0] * n, dtype=torch.int64))
    if masks is not None:
        if isinstance(masks, str):
            masks = np.stack([rect_mask(h, w, *[int(v) for v in b]) for b in boxes]) if n else np.zeros((0, h, w), dtype=bool)
        inst.pred_masks = torch.from_numpy(np.asarray(masks, dtype=bool))
        inst.mask_scores = torch.tensor(mask_scores if mask_scores is not None else scores, dtype=torch.float32)
    return inst


def same(a, b):
    """Result dicts equal with ==, NaN equal to NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float) and a != a:
        return b != b
    return a == b


def blob(h, w, rng):
    """A seeded non-rectangular shape: an ellipse with a wavy edge."""
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0.25, 0.75) * h, rng.uniform(0.25, 0.75) * w
    ry, rx = rng.uniform(0.12, 0.3) * h, rng.uniform(0.12, 0.3) * w
    ang = np.arctan2(yy - cy, xx - cx)
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= (1 + 0.2 * np.sin(rng.randint(2, 6) * ang + rng.uniform(0, 6))) ** 2


def mask_box(m):
    ys, xs = np.nonzero(m)
    return [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


def mixed_case(seed=5):
    """Two images (97x131, 257x130), categories (1, 3, 7): ground truths as polygon, compressed RLE, uncompressed RLE and a crowd
    (uncompressed RLE), and seeded detections: shifted copies of the ground truths plus strays.  -> (dataset, [(image id, Instances)])."""
    rng = np.random.RandomState(seed)
    sizes = {11: (97, 131), 12: (257, 130)}
    cats = (1, 3, 7)
    anns, per_image, aid = [], [], 1
    for img, (h, w) in sorted(sizes.items()):
        gts = []
        box = (w // 8, h // 6, w // 2, h // 2)
        gts.append((ann(aid, img, 1, box), rect_mask(h, w, *box)))
        tri = [w * 0.55, h * 0.1, w * 0.95, h * 0.15, w * 0.6, h * 0.45]
        gts.append((ann(aid + 1, img, 3, (int(w * 0.55), int(h * 0.1), int(w * 0.95), int(h * 0.45)), seg=[tri], area=0.5 * w * 0.4 * h * 0.3), None))
        m = blob(h, w, rng)
        gts.append((ann(aid + 2, img, 7, mask_box(m), seg=wire.rle_encode(m), area=int(m.sum())), m))
        m = blob(h, w, rng)
        gts.append((ann(aid + 3, img, 1, mask_box(m), seg={"size": [h, w], "counts": wire.rle_counts(m)}, area=int(m.sum())), m))
        m = rect_mask(h, w, w // 3, h * 2 // 3, w - 2, h - 1)
        gts.append((ann(aid + 4, img, 3, mask_box(m), iscrowd=1, seg={"size": [h, w], "counts": wire.rle_counts(m)}, area=int(m.sum())), m))
        aid += 5
        anns += [g[0] for g in gts]
        masks, boxes, classes = [], [], []
        for a, m in gts:
            if m is None:
                m = rect_mask(h, w, *[int(v) for v in (a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3])])
            for _ in range(2):
                d = np.roll(m, (rng.randint(-4, 5), rng.randint(-4, 5)), axis=(0, 1))
                masks.append(d)
                boxes.append(mask_box(d))
                classes.append(cats.index(a["category_id"]))
        for _ in range(3):
            m = blob(h, w, rng)
            masks.append(m)
            boxes.append(mask_box(m))
            classes.append(int(rng.randint(0, 3)))
        n = len(masks)
        inst = instances(h, w, boxes, rng.rand(n).tolist(), classes, np.stack(masks), rng.rand(n).tolist())
        per_image.append((img, inst))
    return dataset(sizes, anns, cats), per_image
