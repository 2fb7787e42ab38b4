"""Self-contained COCO-style AP for fixed inputs (the "AP delta" half of the metric).

COCO val2017 and pycocotools are not available offline, so AP is computed against a pseudo ground truth (the detections of
the CPU restatement of the reference on the same images): AP@[.50:.05:.95], 101-point interpolation, per class then
averaged, boxes by box IoU and masks by the IoU of the pasted bitmasks.  As in the reference's evaluator
(evaluation/coco_evaluation.py:557-563) segmentation predictions are ranked by `mask_scores`, boxes by `scores`.
"""
from typing import Dict, List

import numpy as np
import torch


def box_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    area_a = (a[:, 2] - a[:, 0]).clamp(min=0) * (a[:, 3] - a[:, 1]).clamp(min=0)
    area_b = (b[:, 2] - b[:, 0]).clamp(min=0) * (b[:, 3] - b[:, 1]).clamp(min=0)
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b[None, :] - inter).clamp(min=1e-12)


def mask_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a (n,H,W) bool, b (m,H,W) bool."""
    af, bf = a.flatten(1).float(), b.flatten(1).float()
    inter = af @ bf.t()
    union = af.sum(1)[:, None] + bf.sum(1)[None, :] - inter
    iou = inter / union.clamp(min=1.0)
    return torch.where(union == 0, torch.ones_like(iou), iou)      # two empty masks (box outside the image) coincide


def average_precision(preds: List[Dict[str, torch.Tensor]], gts: List[Dict[str, torch.Tensor]], kind: str = "box") -> float:
    """preds[i] / gts[i]: per image dict(boxes (n,4), classes (n), scores (n) [, masks (n,H,W) bool, mask_scores (n)])."""
    thresholds = np.arange(0.5, 0.96, 0.05)
    classes = sorted(set(int(c) for g in gts for c in g["classes"].tolist()))
    aps = []
    for c in classes:
        per_thr = []
        for thr in thresholds:
            scores, tps, n_gt = [], [], 0
            for p, g in zip(preds, gts):
                gi = (g["classes"] == c).nonzero().flatten()
                pi = (p["classes"] == c).nonzero().flatten()
                n_gt += len(gi)
                if len(pi) == 0:
                    continue
                sc = (p["mask_scores"] if kind == "mask" and "mask_scores" in p else p["scores"])[pi]
                order = torch.argsort(sc, descending=True, stable=True)
                pi, sc = pi[order], sc[order]
                if len(gi):
                    iou = box_iou(p["boxes"][pi], g["boxes"][gi]) if kind == "box" else mask_iou(p["masks"][pi], g["masks"][gi])
                taken = torch.zeros(len(gi), dtype=torch.bool)
                for k in range(len(pi)):
                    hit = False
                    if len(gi):
                        cand = iou[k].clone()
                        cand[taken] = -1
                        j = int(torch.argmax(cand))
                        if cand[j] >= thr - 1e-9:
                            taken[j] = True
                            hit = True
                    scores.append(float(sc[k]))
                    tps.append(hit)
            if n_gt == 0:
                continue
            if not scores:
                per_thr.append(0.0)
                continue
            o = np.argsort(-np.asarray(scores), kind="stable")
            tp = np.cumsum(np.asarray(tps, dtype=np.float64)[o])
            fp = np.cumsum(1.0 - np.asarray(tps, dtype=np.float64)[o])
            recall = tp / n_gt
            precision = tp / np.maximum(tp + fp, 1e-12)
            for i in range(len(precision) - 2, -1, -1):
                precision[i] = max(precision[i], precision[i + 1])
            rs = np.linspace(0, 1, 101)
            idx = np.searchsorted(recall, rs, side="left")
            per_thr.append(float(np.mean([precision[i] if i < len(precision) else 0.0 for i in idx])))
        if per_thr:
            aps.append(float(np.mean(per_thr)))
    return float(np.mean(aps)) if aps else float("nan")


class COCOEvaluator:
    """Box and mask AP / AR against a COCO annotation file, with detectron2's reset / process / evaluate protocol: the counterpart of
    the reference's centermask.evaluation.COCOEvaluator (evaluation/coco_evaluation.py:33-359), segm ranked by `mask_score` (:551-563).

    annotations: path of a COCO json, or the loaded dict.  Model class k is the k-th category id in ascending order
    (`thing_dataset_id_to_contiguous_id`, as detectron2's COCO registration builds it); predictions are mapped back through it.
    The scoring protocol is coco_eval.py's restatement of pycocotools, never run beside the real one (see its docstring).

    process() keeps, per image, the COCO result records (wire.instances_to_coco_json) and, when masks are present, the table of
    integer counts mask IoU is formed from: pixels of every detection in every ground truth of the image, and both areas.  For
    Instances on a GPU the table comes from ops.mask_intersections and the bitmasks are never downloaded; for CPU Instances from NumPy
    on the same bits — selected by where the input lies, as in wire.rle_encode_batch.  evaluate() touches no bitmap.

    tasks: None means bbox, and segm when masks are present.  "boundary" is opt-in: Boundary AP (Cheng et al., CVPR 2021), COCOeval as
    for segm with IoU = min(mask IoU, IoU of the mask boundaries at erosion distance round(boundary_dilation_ratio * image diagonal)).
    process() then also keeps pred["boundary_table"], the same counts for the boundaries (ops.mask_boundary_intersections on the GPU,
    coco_eval.boundary_intersections_host on the host).  The rule is restated from the publication in coco_eval.boundary_host and is
    unpinned against the real boundary-iou-api, as the rest is against pycocotools.

    Not built, refused by name: tasks containing "keypoints" (OKS), and the proposals branch."""

    def __init__(self, annotations, tasks=None, distributed: bool = False, output_dir=None, boundary_dilation_ratio: float = 0.02):
        import json
        from . import coco_eval
        if isinstance(annotations, (str, bytes)) or hasattr(annotations, "__fspath__"):
            with open(annotations) as f:
                annotations = json.load(f)
        if tasks is not None:
            tasks = tuple(tasks)
            for t in tasks:
                if t == "keypoints":
                    raise NotImplementedError('COCOEvaluator: task "keypoints" (OKS) is not built')
                if t not in ("bbox", "segm", "boundary"):
                    raise ValueError("COCOEvaluator: unknown task {!r}".format(t))
        self._tasks = tasks
        self._boundary = tasks is not None and "boundary" in tasks
        self._boundary_ratio = float(boundary_dilation_ratio)
        self._distributed = distributed
        self._output_dir = output_dir
        self._gt = coco_eval.GroundTruth(annotations)
        self._do_evaluation = self._gt.has_annotations         # test-set files carry no annotations
        self.thing_dataset_id_to_contiguous_id = {c: k for k, c in enumerate(self._gt.cat_ids)}
        self.thing_classes = [self._gt.cat_names[c] for c in self._gt.cat_ids]
        self.reset()

    def reset(self):
        self._predictions = []

    def _table(self, instances, img_id):
        from . import coco_eval, ops
        if img_id not in self._gt.images:
            raise ValueError("COCOEvaluator: image_id {!r} is not in the annotation file".format(img_id))
        h, w = self._gt.size(img_id)
        masks = instances.pred_masks
        if masks.dim() != 3 or tuple(masks.shape[1:]) != (h, w):
            raise ValueError("COCOEvaluator: pred_masks of image {!r} are {}, the annotated size is {}x{}: post-process the instances to the "
                             "annotated size".format(img_id, "x".join(str(int(v)) for v in masks.shape[1:]), h, w))
        counts = self._gt.counts(img_id)
        if self._boundary:                                      # both tables from one pass: (mask 3-tuple, boundary 3-tuple)
            d = coco_eval.boundary_dilation(h, w, self._boundary_ratio)
            if masks.is_cuda:
                six = tuple(t.numpy() for t in ops.mask_boundary_intersections(masks, counts, h, w, d))
            else:
                six = coco_eval.boundary_intersections_host(masks.numpy(), counts, h, w, d)
            return six[:3], six[3:]
        if masks.is_cuda:
            inter, a_dt, a_gt = (t.numpy() for t in ops.mask_intersections(masks, counts, h, w))
        else:
            inter, a_dt, a_gt = coco_eval.intersections_host(masks.numpy(), counts, h, w)
        return (inter, a_dt, a_gt), None

    def process(self, inputs, outputs):
        from . import wire
        for inp, out in zip(inputs, outputs):
            if "proposals" in out:
                raise NotImplementedError('COCOEvaluator: the "proposals" branch (box proposal AR) is not built')
            if "instances" not in out:
                continue
            inst, img_id = out["instances"], inp["image_id"]
            pred = {"image_id": img_id, "instances": wire.instances_to_coco_json(inst, img_id)}
            if self._do_evaluation and len(inst) and inst.has("pred_masks"):
                pred["table"], btable = self._table(inst, img_id)
                if btable is not None:
                    pred["boundary_table"] = btable
            self._predictions.append(pred)

    def _gathered(self):
        import torch.distributed as dist
        if not (self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return self._predictions
        rank = dist.get_rank()
        parts = [None] * dist.get_world_size() if rank == 0 else None
        dist.gather_object(self._predictions, parts, dst=0)
        return [p for part in parts for p in part] if rank == 0 else None

    def evaluate(self, img_ids=None):
        import json
        import os
        from . import coco_eval, wire
        predictions = self._gathered()
        if predictions is None:                                 # not the main process
            return {}
        if len(predictions) == 0:
            return {}
        num_classes = len(self._gt.cat_ids)
        results, tables, btables = [], {}, {}
        for p in predictions:
            if "table" in p:
                tables[p["image_id"]] = p["table"]
            if "boundary_table" in p:
                btables[p["image_id"]] = p["boundary_table"]
            for k, r in enumerate(p["instances"]):
                c = r["category_id"]
                if not 0 <= c < num_classes:
                    raise ValueError("COCOEvaluator: a prediction has class {}, the annotation file has {} categories".format(c, num_classes))
                results.append(dict(r, category_id=self._gt.cat_ids[c], _k=k))
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, "coco_instances_results.json"), "w") as f:
                json.dump([{k: v for k, v in r.items() if k != "_k"} for r in results], f)
        if not self._do_evaluation:
            return {}
        tasks = self._tasks or (("bbox", "segm") if any("segmentation" in r for r in results) else ("bbox",))
        out = {}
        for task in sorted(tasks):
            names = ("AP", "AP50", "AP75", "APs", "APm", "APl")
            if not results:
                out[task] = {n: float("nan") for n in names}
                continue
            if task in ("segm", "boundary"):
                have = set(tables) if task == "segm" else set(tables) & set(btables)
                missing = sorted(set(r["image_id"] for r in results) - have)
                if missing:
                    raise ValueError("COCOEvaluator: no mask table for images {}: their instances had no pred_masks".format(missing[:5]))
            rs = wire.segm_results_ranked_by_mask_score(results) if task in ("segm", "boundary") else results
            acc = coco_eval.score(self._gt, rs, task, tables, img_ids, btables)
            res = {n: (float(v) * 100 if v >= 0 else float("nan")) for n, v in zip(coco_eval.STAT_NAMES, acc["stats"])}
            if num_classes > 1:
                for k, name in enumerate(self.thing_classes):
                    pr = acc["precision"][:, :, k, 0, -1]
                    pr = pr[pr > -1]
                    res["AP-" + name] = float(np.mean(pr) * 100) if pr.size else float("nan")
            out[task] = res
        return out


class CityscapesInstanceEvaluator:
    """Instance-level AP on Cityscapes ground truth, with the reset / process / evaluate protocol of COCOEvaluator: the counterpart of
    the reference's centermask.evaluation.CityscapesInstanceEvaluator (evaluation/cityscapes_evaluation.py:47-130), predictions ranked
    by `mask_scores` when present (:77).  The scoring rule is cityscapes_eval.py's restatement of cityscapesscripts'
    evalInstanceLevelSemanticLabeling, never run beside the real scripts (see its docstring).

    ground_truth: dict <city>_<seq>_<frame> -> (H,W) integer array of *_gtFine_instanceIds values; otherwise gt_dir is globbed for
    */*_gtFine_instanceIds.png and the files are read with `loader` (default cityscapes_eval.read_label_png) when their image is
    processed.  thing_classes[k] names model class k; a name outside the dataset's labels is refused here, one that is not an
    evaluated class is skipped.  An input's file_name .../<city>_<seq>_<frame>_leftImg8bit.png selects its ground truth.

    process() turns the label image into columns (void, other, one per ground-truth region) and keeps, per prediction, its pixel count
    and its pixels on void and on each region of its class.  For Instances on a GPU the table comes from ops.mask_label_counts and
    no bitmap is downloaded or written as a file; for CPU Instances from cityscapes_eval.label_counts_host, the same integers —
    selected by where the input lies.  An image with more than 4094 regions takes the host path.  evaluate() touches no bitmap."""

    def __init__(self, gt_dir=None, ground_truth=None, thing_classes=None, distributed: bool = False, loader=None):
        import glob
        import os
        from . import cityscapes_eval as ce
        self.thing_classes = list(ce.THING_CLASSES if thing_classes is None else thing_classes)
        unknown = [n for n in self.thing_classes if n not in ce.LABEL_NAMES]
        if unknown:
            raise ValueError("CityscapesInstanceEvaluator: {} are not Cityscapes label names".format(unknown))
        self._labels = [ce.CLASS_ID.get(n) for n in self.thing_classes]
        self._loader = loader or ce.read_label_png
        self._distributed = distributed
        if ground_truth is not None:
            self._gt = dict(ground_truth)
        elif gt_dir is not None:
            files = sorted(glob.glob(os.path.join(str(gt_dir), "*", "*_gtFine_instanceIds.png")))
            if not files:
                raise ValueError("CityscapesInstanceEvaluator: no */*_gtFine_instanceIds.png under {}".format(gt_dir))
            self._gt = {ce.image_name(f): f for f in files}
        else:
            raise ValueError("CityscapesInstanceEvaluator: give gt_dir or ground_truth")
        self.reset()

    def reset(self):
        self._predictions = []

    def _label_image(self, name):
        gt = self._gt[name]
        if isinstance(gt, (str, bytes)) or hasattr(gt, "__fspath__"):
            gt = self._loader(gt)
        return gt

    def process(self, inputs, outputs):
        from . import cityscapes_eval as ce, ops
        for inp, out in zip(inputs, outputs):
            name = ce.image_name(inp["file_name"])
            if name not in self._gt:
                raise ValueError("CityscapesInstanceEvaluator: no ground truth for {!r} (file_name {!r})".format(name, inp["file_name"]))
            cols, regions = ce.columns(self._label_image(name))
            inst = out.get("instances")
            if inst is None or len(inst) == 0:                          # an image without predictions still counts its ground truth
                self._predictions.append(ce.image_record(name, regions, [], [], None, None))
                continue
            h, w = cols.shape
            masks = inst.pred_masks
            if masks.dim() != 3 or tuple(masks.shape[1:]) != (h, w):
                raise ValueError("CityscapesInstanceEvaluator: pred_masks of image {!r} are {}, the ground truth is {}x{}: post-process the "
                                 "instances to the ground-truth size".format(name, "x".join(str(int(v)) for v in masks.shape[1:]), h, w))
            classes = inst.pred_classes.cpu().tolist()
            bad = [c for c in classes if not 0 <= c < len(self._labels)]
            if bad:
                raise ValueError("CityscapesInstanceEvaluator: a prediction has class {}, thing_classes has {} names".format(bad[0], len(self._labels)))
            conf = (inst.mask_scores if inst.has("mask_scores") else inst.scores).cpu().tolist()
            num_cols = 2 + len(regions)
            if masks.is_cuda and num_cols <= ce.MAX_DEVICE_COLS:
                table, areas = (t.numpy() for t in ops.mask_label_counts(masks, cols, num_cols))
            else:
                table, areas = ce.label_counts_host(masks.cpu().numpy(), cols, num_cols)
            self._predictions.append(ce.image_record(name, regions, [self._labels[c] for c in classes], conf, table, areas))

    _gathered = COCOEvaluator._gathered

    def evaluate(self):
        from . import cityscapes_eval as ce
        predictions = self._gathered()
        if predictions is None:                                         # not the main process
            return {}
        records = {p["name"]: p for p in predictions}
        missing = sorted(set(self._gt) - set(records))
        if missing:
            raise ValueError("CityscapesInstanceEvaluator: {} ground truths were never processed, among them {}".format(len(missing), missing[:5]))
        res = ce.score([records[k] for k in sorted(records)])
        out = {"AP": res["AP"] * 100, "AP50": res["AP50"] * 100}
        for name, v in res["classes"].items():
            out["AP-" + name] = v * 100
        return {"segm": out}
