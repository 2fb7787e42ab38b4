"""Cityscapes instance-level scoring on the host (NumPy, float64): the protocol behind evaluation.CityscapesInstanceEvaluator.

The reference (evaluation/cityscapes_evaluation.py:47-130) writes every predicted mask as a PNG and calls cityscapesscripts'
evalInstanceLevelSemanticLabeling.  That package is not available here, so its rule is RESTATED below from the published scripts, from
memory, and has never been run beside them: it is unpinned against the real scripts, and the text of this module is the specification
the tests hold it to (a brute-force restatement on whole bitmaps, tests/cityscapes_ref.py, and hand-worked known answers).

What the rule needs of the pixels is one table of integers per image: for each prediction, how many of its pixels fall on each
ground-truth region.  The label image is turned into COLUMNS (column 0: void pixels, column 1: everything else that is no region,
columns 2..: the ground-truth regions in ascending pixel value) and the table is ops.mask_label_counts on the GPU or label_counts_host
here, the same integers.

Labels.  A pixel value v of *_gtFine_instanceIds.png has label v if v < 1000, else v // 1000.  Every distinct v whose label is an
evaluated class is a ground-truth region of that class (instID = v), the "group" regions v < 1000 included.  A pixel is void if v itself
is one of VOID_IDS (so v = 29xxx and 30xxx are not void, as in the scripts).

One choice here is this project's own: a class that has ground truth but no list entry at a threshold scores 0.0 (the scripts raise
there).  Predictions without pixels are dropped when the records are made and count for nothing."""
import os
import struct
import zlib

import numpy as np

# the evaluated classes in detectron2's thing_classes order, with their Cityscapes label ids
CLASSES = (("person", 24), ("rider", 25), ("car", 26), ("truck", 27), ("bus", 28), ("train", 31), ("motorcycle", 32), ("bicycle", 33))
THING_CLASSES = tuple(n for n, _ in CLASSES)
CLASS_ID = dict(CLASSES)
VOID_IDS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)
# every label name of the dataset: a thing_classes entry outside this list is a mistake, one inside it that is not evaluated is skipped
LABEL_NAMES = ("unlabeled", "ego vehicle", "rectification border", "out of roi", "static", "dynamic", "ground", "road", "sidewalk",
               "parking", "rail track", "building", "wall", "fence", "guard rail", "bridge", "tunnel", "pole", "polegroup",
               "traffic light", "traffic sign", "vegetation", "terrain", "sky", "person", "rider", "car", "truck", "bus", "caravan",
               "trailer", "train", "motorcycle", "bicycle", "license plate")
OVERLAPS = np.arange(0.5, 1.0, 0.05)
MIN_REGION_SIZE = 100
MAX_DEVICE_COLS = 4096          # CMK_LABEL_MAX_COLS: above it an image's table is made by label_counts_host


# ---------------------------------------------------------------------------------------------------------------
# label images
# ---------------------------------------------------------------------------------------------------------------
def _unfilter(raw, h, stride, bpp):
    """PNG filter types 0-4 undone: raw is h rows of 1 + stride bytes -> (h, stride) uint8."""
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=y * (stride + 1) + 1)
        if ft == 0:
            cur = line
        elif ft == 1:                                                   # Sub: a running sum per byte lane, modulo 256
            n = -(-stride // bpp)
            pad = np.zeros(n * bpp, dtype=np.uint8)
            pad[:stride] = line
            cur = np.cumsum(pad.reshape(n, bpp), axis=0, dtype=np.uint8).reshape(-1)[:stride]
        elif ft == 2:                                                   # Up
            cur = line + prev
        elif ft in (3, 4):                                              # Average, Paeth: sequential along the row
            cur = bytearray(stride)
            src, up = line.tolist(), prev.tolist()
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = up[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = up[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (src[i] + pred) & 255
            cur = np.frombuffer(bytes(cur), dtype=np.uint8)
        else:
            raise ValueError("read_label_png: filter type {} in row {} is not one of 0-4".format(ft, y))
        out[y] = cur
        prev = out[y]
    return out


def read_label_png(path):
    """An 8- or 16-bit greyscale, non-interlaced PNG -> (H,W) uint8 or uint16, with zlib only (the default loader of the evaluator;
    rows filtered with Average or Paeth are undone in a Python loop, so pass loader= where speed matters).  Anything else is refused by
    name."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("read_label_png: {} is not a PNG file".format(path))
    pos, ihdr, idat, ended = 8, None, [], False
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError("read_label_png: {} is truncated in its {} chunk".format(path, kind.decode("latin1")))
        if zlib.crc32(kind + body) & 0xffffffff != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise ValueError("read_label_png: {} has a bad CRC in its {} chunk".format(path, kind.decode("latin1")))
        pos += 12 + n
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
    if ihdr is None or not ended:
        raise ValueError("read_label_png: {} lacks its IHDR or IEND chunk".format(path))
    w, h, depth, colour, compression, filt, interlace = ihdr
    if colour != 0:
        raise ValueError("read_label_png: {} has colour type {} (RGB, palette or alpha); only greyscale label images are read".format(path, colour))
    if depth not in (8, 16):
        raise ValueError("read_label_png: {} has bit depth {}; only 8 and 16 are read".format(path, depth))
    if interlace != 0:
        raise ValueError("read_label_png: {} is interlaced (Adam7); only non-interlaced files are read".format(path))
    if compression != 0 or filt != 0 or w < 1 or h < 1:
        raise ValueError("read_label_png: {} has an IHDR outside the PNG standard".format(path))
    bpp = depth // 8
    stride = w * bpp
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (stride + 1):
        raise ValueError("read_label_png: {} holds {} bytes of pixel data, {}x{} at {} bits needs {}".format(path, len(raw), h, w, depth, h * (stride + 1)))
    rows = _unfilter(raw, h, stride, bpp)
    if depth == 8:
        return rows
    return rows.view(">u2").astype(np.uint16)


def image_name(file_name):
    """.../<city>_<seq>_<frame>_leftImg8bit.png (or ..._gtFine_instanceIds.png) -> <city>_<seq>_<frame>."""
    stem = os.path.splitext(os.path.basename(str(file_name)))[0]
    for suffix in ("_leftImg8bit", "_gtFine_instanceIds"):
        if stem.endswith(suffix):
            return stem[:-len(suffix)]
    return stem


def columns(label_image):
    """(H,W) integer label image -> (cols (H,W), regions): cols is uint16 when there are at most 65536 columns (int32 otherwise),
    regions the list of (instID, label id, pixelCount) of columns 2, 3, .. in that order."""
    v = np.asarray(label_image)
    if v.ndim != 2 or v.dtype.kind not in "iu" or v.size == 0:
        raise ValueError("cityscapes_eval.columns: expected a non-empty (H,W) integer label image, got {} {}".format(v.dtype, v.shape))
    if int(v.min()) < 0:
        raise ValueError("cityscapes_eval.columns: the label image holds the negative value {}".format(int(v.min())))
    small = int(v.max()) < 1 << 20                                      # every real label image: a histogram and a lookup, no sort
    if small:
        hist = np.bincount(v.reshape(-1))
        uniq = np.flatnonzero(hist)
        counts = hist[uniq]
    else:
        uniq, inverse, counts = np.unique(v.reshape(-1), return_inverse=True, return_counts=True)
        uniq = uniq.astype(np.int64)
    label = np.where(uniq < 1000, uniq, uniq // 1000)
    is_region = np.isin(label, [i for _, i in CLASSES])
    is_void = np.isin(uniq, VOID_IDS)
    n_cols = 2 + int(is_region.sum())
    col = np.where(is_region, 1 + np.cumsum(is_region), np.where(is_void, 0, 1)).astype(np.uint16 if n_cols <= 65536 else np.int32)
    if small:
        lut = np.zeros(len(hist), dtype=col.dtype)
        lut[uniq] = col
        cols = lut[v]
    else:
        cols = col[inverse.reshape(-1)].reshape(v.shape)
    regions = [(int(u), int(l), int(c)) for u, l, c in zip(uniq[is_region], label[is_region], counts[is_region])]
    return cols, regions


def label_counts_host(masks, cols, num_cols):
    """The host path of ops.mask_label_counts, the same integers: masks (N,H,W) bool, cols (H,W) -> (table (N,num_cols), areas (N,))
    int32; a column >= num_cols is counted nowhere."""
    masks = np.asarray(masks).astype(bool)
    cols = np.asarray(cols)
    if masks.ndim != 3 or masks.shape[1:] != cols.shape:
        raise ValueError("label_counts_host: masks {} against columns {}".format(masks.shape, cols.shape))
    c = int(num_cols)
    table = np.zeros((masks.shape[0], c), dtype=np.int32)
    for n, m in enumerate(masks):
        under = cols[m].astype(np.int64)
        table[n] = np.bincount(under[under < c], minlength=c)
    return table, masks.sum(axis=(1, 2)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# records and the score
# ---------------------------------------------------------------------------------------------------------------
def image_record(name, regions, labels, confidences, table, areas):
    """What evaluate() needs of one image.  regions: columns()'s list.  Per prediction in Instances order: labels[n], its Cityscapes
    label id or None where its class is not evaluated (skipped), confidences[n], row n of the table and areas[n].  A prediction keeps
    pixelCount, voidIntersection and, as `inter`, {region index: pixels} over the regions of its own class it touches."""
    preds = []
    for n, (lab, conf) in enumerate(zip(labels, confidences)):
        if lab is None or int(areas[n]) == 0:
            continue
        inter = {r: int(table[n][2 + r]) for r, (_, rl, _) in enumerate(regions) if rl == lab and table[n][2 + r] > 0}
        preds.append({"label": int(lab), "confidence": float(conf), "pixelCount": int(areas[n]), "void": int(table[n][0]), "inter": inter})
    return {"name": name, "regions": [tuple(r) for r in regions], "preds": preds}


def _entries(records, label, t):
    """The (true, score) list of one class at one overlap threshold -> (trues, scores, hardFns, haveGt, havePred)."""
    trues, scores, hard_fns, have_gt, have_pred = [], [], 0, False, False
    for rec in records:
        regions = rec["regions"]
        preds = [p for p in rec["preds"] if p["label"] == label]
        kept = [r for r, (inst, lab, px) in enumerate(regions) if lab == label and inst >= 1000 and px >= MIN_REGION_SIZE]
        have_gt = have_gt or bool(kept)
        have_pred = have_pred or bool(preds)

        def overlap(p, r):
            i = p["inter"][r]
            return float(i) / float(regions[r][2] + p["pixelCount"] - i)

        extra = []
        for r in kept:
            best = None
            for p in preds:
                if r in p["inter"] and overlap(p, r) > t:
                    if best is None:
                        best = p["confidence"]
                    else:                                              # a further match: the region keeps the larger confidence
                        extra.append(min(best, p["confidence"]))
                        best = max(best, p["confidence"])
            if best is None:
                hard_fns += 1
            else:
                trues.append(1)
                scores.append(best)
        trues += [0] * len(extra)
        scores += extra
        for p in preds:
            if any(overlap(p, r) > t for r in p["inter"]):
                continue
            ignore = p["void"]
            for r, i in p["inter"].items():
                if regions[r][0] < 1000:
                    ignore += i
                if regions[r][2] < MIN_REGION_SIZE:
                    ignore += i
            if float(ignore) / p["pixelCount"] <= t:
                trues.append(0)
                scores.append(p["confidence"])
    return np.asarray(trues, dtype=np.float64), np.asarray(scores, dtype=np.float64), hard_fns, have_gt, have_pred


def average_precision(trues, scores, hard_fns):
    """The area under the precision-recall curve as the scripts integrate it."""
    order = np.argsort(scores, kind="stable")
    ys, yt = scores[order], trues[order]
    cum = np.cumsum(yt)
    _, first = np.unique(ys, return_index=True)
    n, total = len(ys), cum[-1]
    precision, recall = np.zeros(len(first) + 1), np.zeros(len(first) + 1)
    for k, j in enumerate(first):
        before = cum[j - 1] if j > 0 else 0.0
        tp = total - before
        fp = n - j - tp
        fn = before + hard_fns
        precision[k] = tp / (tp + fp)
        recall[k] = tp / (tp + fn)
    precision[-1], recall[-1] = 1.0, 0.0
    r = np.concatenate([recall[:1], recall, [0.0]])
    return float(np.dot(precision, np.convolve(r, [-0.5, 0, 0.5], "valid")))


def score(records, overlaps=OVERLAPS):
    """records: image_record()s -> {"ap": (classes, overlaps) float64 with nan where a class has no ground truth, "AP", "AP50",
    "classes": {name: mean over the overlaps}} as fractions."""
    ap = np.full((len(CLASSES), len(overlaps)), np.nan)
    for ci, (_, label) in enumerate(CLASSES):
        for ti, t in enumerate(overlaps):
            trues, scores, hard_fns, have_gt, have_pred = _entries(records, label, float(t))
            if not have_gt:
                continue
            ap[ci, ti] = average_precision(trues, scores, hard_fns) if have_pred and len(trues) else 0.0

    def nanmean(a):
        return float(np.mean(a[~np.isnan(a)])) if (~np.isnan(a)).any() else float("nan")

    return {"ap": ap, "AP": nanmean(ap), "AP50": nanmean(ap[:, 0]),
            "classes": {name: float(np.mean(ap[ci])) for ci, (name, _) in enumerate(CLASSES)}}
