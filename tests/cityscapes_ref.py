"""A brute-force restatement of Cityscapes instance-level scoring that works the way the published scripts do: every prediction is a
whole bitmap, compared with `gt == instID` over the whole image once per ground-truth instance of its class, and the matches are
walked with growing curTrue / curScore / curMatch arrays.  It shares no code with centermask2_amd.cityscapes_eval (no columns, no
table): the two agree only if both state the same rule.  Also the shared two-image, three-class case of the CPU and GPU tests."""
import numpy as np

CLASS_IDS = {"person": 24, "rider": 25, "car": 26, "truck": 27, "bus": 28, "train": 31, "motorcycle": 32, "bicycle": 33}
VOID = [0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30]
OVERLAPS = np.arange(0.5, 1.0, 0.05)


def match_image(gt, preds):
    """gt (H,W) ints; preds: list of (class name, confidence, (H,W) bool) -> (gt instances per class name, pred instances per class name),
    each instance a dict that lists its partners with the intersection."""
    gt = np.asarray(gt).astype(np.int64)
    gts = {name: [] for name in CLASS_IDS}
    for v in np.unique(gt):
        label = int(v) if v < 1000 else int(v) // 1000
        for name, i in CLASS_IDS.items():
            if i == label:
                gts[name].append({"instID": int(v), "pixelCount": int(np.count_nonzero(gt == v)), "matchedPred": []})
    void = np.isin(gt, VOID)
    out = {name: [] for name in CLASS_IDS}
    for name, conf, mask in preds:
        if name not in CLASS_IDS:
            continue
        mask = np.asarray(mask).astype(bool)
        p = {"confidence": float(conf), "pixelCount": int(np.count_nonzero(mask)), "matchedGt": [],
             "voidIntersection": int(np.count_nonzero(np.logical_and(void, mask)))}
        if p["pixelCount"] == 0:
            continue
        for g in gts[name]:
            inter = int(np.count_nonzero(np.logical_and(gt == g["instID"], mask)))
            if inter > 0:
                p["matchedGt"].append(dict(instID=g["instID"], pixelCount=g["pixelCount"], intersection=inter))
                g["matchedPred"].append(dict(confidence=p["confidence"], pixelCount=p["pixelCount"], intersection=inter))
        out[name].append(p)
    return gts, out


def class_ap(matches, name, t):
    y_true, y_score, hard_fns, have_gt, have_pred = np.empty(0), np.empty(0), 0, False, False
    for gts, preds in matches:
        pred_inst = preds[name]
        gt_inst = [g for g in gts[name] if g["instID"] >= 1000 and g["pixelCount"] >= 100]
        if gt_inst:
            have_gt = True
        if pred_inst:
            have_pred = True
        cur_true, cur_score, cur_match = np.ones(len(gt_inst)), np.full(len(gt_inst), -np.inf), np.zeros(len(gt_inst), dtype=bool)
        for gi, g in enumerate(gt_inst):
            found = False
            for p in g["matchedPred"]:
                overlap = float(p["intersection"]) / (g["pixelCount"] + p["pixelCount"] - p["intersection"])
                if overlap > t:
                    if cur_match[gi]:
                        hi, lo = max(cur_score[gi], p["confidence"]), min(cur_score[gi], p["confidence"])
                        cur_score[gi] = hi
                        cur_true, cur_score, cur_match = np.append(cur_true, 0), np.append(cur_score, lo), np.append(cur_match, True)
                    else:
                        found = True
                        cur_match[gi] = True
                        cur_score[gi] = p["confidence"]
            if not found:
                hard_fns += 1
        cur_true, cur_score = cur_true[cur_match], cur_score[cur_match]
        for p in pred_inst:
            found = False
            for g in p["matchedGt"]:
                if float(g["intersection"]) / (g["pixelCount"] + p["pixelCount"] - g["intersection"]) > t:
                    found = True
                    break
            if not found:
                ignore = p["voidIntersection"]
                for g in p["matchedGt"]:
                    if g["instID"] < 1000:
                        ignore += g["intersection"]
                    if g["pixelCount"] < 100:
                        ignore += g["intersection"]
                if float(ignore) / p["pixelCount"] <= t:
                    cur_true, cur_score = np.append(cur_true, 0), np.append(cur_score, p["confidence"])
        y_true, y_score = np.append(y_true, cur_true), np.append(y_score, cur_score)
    if not have_gt:
        return float("nan")
    if not have_pred or len(y_true) == 0:
        return 0.0
    order = np.argsort(y_score)
    ys, yt = y_score[order], y_true[order]
    cum = np.cumsum(yt)
    thresholds, idx = np.unique(ys, return_index=True)
    n_prec = len(idx) + 1
    n, total = len(ys), cum[-1]
    precision, recall = np.zeros(n_prec), np.zeros(n_prec)
    cum = np.append(cum, 0)
    for k, j in enumerate(idx):
        c = cum[j - 1]
        tp = total - c
        fp = n - j - tp
        fn = c + hard_fns
        precision[k] = tp / (tp + fp)
        recall[k] = tp / (tp + fn)
    precision[-1], recall[-1] = 1.0, 0.0
    rc = np.append(np.append(recall[0], recall), 0.0)
    return float(np.dot(precision, np.convolve(rc, [-0.5, 0, 0.5], "valid")))


def evaluate(images):
    """images: list of (gt (H,W), [(class name, confidence, mask)]) -> {"AP", "AP50", "AP-<class>"} as fractions."""
    matches = [match_image(gt, preds) for gt, preds in images]
    ap = np.array([[class_ap(matches, name, float(t)) for t in OVERLAPS] for name in CLASS_IDS])

    def nanmean(a):
        a = a[~np.isnan(a)]
        return float(a.mean()) if a.size else float("nan")

    out = {"AP": nanmean(ap), "AP50": nanmean(ap[:, 0])}
    for k, name in enumerate(CLASS_IDS):
        out["AP-" + name] = float(np.mean(ap[k]))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the shared case: two images, ground truth of three classes (car, person, bicycle)
# ---------------------------------------------------------------------------------------------------------------
H, W = 48, 80
NAMES = ("aachen_000000_000019", "aachen_000001_000019")


def rect(y0, x0, y1, x1):
    m = np.zeros((H, W), dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


def two_image_case():
    """-> (ground_truth {name: (H,W) uint16}, predictions {name: [(class name, score, mask_score, mask)]}).  Road (7) fills each image.
    Image 0: cars 26001 and 26002 (12x12), a small car 26003 (5x5), a car group 26 (8x10), person 24001 (10x12), an ego-vehicle strip
    (void 1), a caravan 29001 (no evaluated class, not void).  Image 1: persons 24001 and 24002, bicycle 33001, car 26001."""
    g0 = np.full((H, W), 7, dtype=np.uint16)
    g0[2:14, 2:14] = 26001
    g0[2:14, 20:32] = 26002
    g0[20:25, 2:7] = 26003
    g0[20:28, 20:30] = 26
    g0[30:40, 40:52] = 24001
    g0[44:48, :] = 1
    g0[2:10, 60:72] = 29001
    g1 = np.full((H, W), 7, dtype=np.uint16)
    g1[4:16, 4:14] = 24001
    g1[4:16, 30:41] = 24002
    g1[24:36, 10:22] = 33001
    g1[24:38, 50:66] = 26001
    g1[0:2, :] = 3
    p0 = [("car", 0.90, 0.80, rect(2, 2, 14, 14)),            # exact
          ("car", 0.80, 0.85, rect(3, 21, 14, 32)),           # inside 26002: IoU 121/144, a match up to 0.8
          ("car", 0.70, 0.60, rect(2, 20, 14, 31)),           # a second, weaker match of 26002 (IoU 132/144)
          ("car", 0.60, 0.95, rect(20, 20, 28, 30)),          # on the group: ignored
          ("car", 0.50, 0.50, rect(19, 1, 26, 8)),            # over the small car, 25 of 49 > 0.5: ignored at t = 0.5, a false positive above
          ("car", 0.40, 0.88, rect(40, 10, 48, 20)),          # half on road, half on void: a false positive exactly at t = 0.5 and above
          ("car", 0.30, 0.30, rect(30, 60, 36, 70)),          # on road: a false positive
          ("person", 0.90, 0.70, rect(30, 40, 40, 50)),       # 100 of 120
          ("person", 0.20, 0.90, rect(2, 60, 10, 72)),        # on the caravan: a false positive
          ("bicycle", 0.60, 0.60, rect(14, 40, 20, 50)),      # no bicycle ground truth in this image
          ("truck", 0.99, 0.99, rect(2, 2, 14, 14)),          # a class without ground truth anywhere
          ("car", 0.99, 0.99, rect(0, 0, 0, 0))]              # no pixels: dropped
    p1 = [("person", 0.95, 0.65, rect(4, 4, 16, 14)),
          ("person", 0.85, 0.65, rect(4, 30, 15, 41)),        # the same mask score as the one above: a tie
          ("bicycle", 0.75, 0.40, rect(24, 10, 36, 20)),
          ("bicycle", 0.65, 0.45, rect(26, 10, 36, 22)),
          ("car", 0.55, 0.90, rect(24, 50, 38, 64)),
          ("car", 0.45, 0.20, rect(0, 50, 4, 66))]            # half on void 3, half on road
    gt = {NAMES[0]: g0, NAMES[1]: g1}
    return gt, {NAMES[0]: p0, NAMES[1]: p1}


def instances_of(preds, device="cpu", with_mask_scores=True):
    """The predictions of one image of the case as Instances (classes index the eight evaluated names in their order)."""
    import torch
    from centermask2_amd.structures import Instances
    names = list(CLASS_IDS)
    inst = Instances((H, W), pred_masks=torch.from_numpy(np.stack([m for _, _, _, m in preds])).to(device),
                     pred_classes=torch.tensor([names.index(c) for c, _, _, _ in preds], dtype=torch.int64, device=device),
                     scores=torch.tensor([s for _, s, _, _ in preds], dtype=torch.float32, device=device))
    if with_mask_scores:
        inst.mask_scores = torch.tensor([ms for _, _, ms, _ in preds], dtype=torch.float32, device=device)
    return inst


def bitmap_images(gt, preds, with_mask_scores=True):
    """The case as evaluate() takes it; confidences pass through float32 as they do in Instances."""
    return [(gt[n], [(c, float(np.float32(ms if with_mask_scores else s)), m) for c, s, ms, m in preds[n]]) for n in NAMES]
