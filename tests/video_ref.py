"""The tests' own NumPy restatement of the video association rule (DESIGN §3 "Video"): detectron2's VideoVisualizer._assign_colors written
literally and sequentially, in float64.  It reads (n,h,w) bool masks directly, never packed words, and shares nothing with
csrc/visualize.hip.  `RefTracker.update` returns the frame's track ids; the table is a list of dicts in table order."""
import numpy as np

BOX_THRESHOLD = 0.6
MASK_THRESHOLD = 0.5


def box_iou(a, b) -> float:
    """pycocotools' bbIou on the corners of two float32 (x1, y1, x2, y2) boxes, every operation rounded to float64 on its own; a NaN
    coordinate, a zero union or a NaN result give 0."""
    ax1, ay1, ax2, ay2 = (np.float64(np.float32(v)) for v in a)
    bx1, by1, bx2, by2 = (np.float64(np.float32(v)) for v in b)
    if any(v != v for v in (ax1, ay1, ax2, ay2, bx1, by1, bx2, by2)):
        return 0.0
    with np.errstate(all="ignore"):
        iw = (ax2 if ax2 < bx2 else bx2) - (ax1 if ax1 > bx1 else bx1)
        ih = (ay2 if ay2 < by2 else by2) - (ay1 if ay1 > by1 else by1)
        inter = iw * ih if iw > 0.0 and ih > 0.0 else np.float64(0.0)
        union = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1) - inter
        if not union != 0.0:
            return 0.0
        v = inter / union
    return 0.0 if v != v else float(v)


def mask_iou(a, b) -> float:
    """Two (h,w) bool masks: pixels in both over pixels in either, float64; an empty union gives 0."""
    inter = int(np.count_nonzero(a & b))
    union = int(np.count_nonzero(a)) + int(np.count_nonzero(b)) - inter
    return 0.0 if union == 0 else float(np.float64(inter) / np.float64(union))


class RefTracker:
    def __init__(self, match="box", iou_threshold=None, ttl=8, max_tracks=256):
        self.match, self.ttl, self.max_tracks = match, int(ttl), int(max_tracks)
        self.threshold = float(iou_threshold) if iou_threshold is not None else (BOX_THRESHOLD if match == "box" else MASK_THRESHOLD)
        self.tracks = []            # dicts: box (4,) float32, cls int, id int, ttl int, mask (h,w) bool or None
        self.next_id = 0
        self.dropped = 0

    def iou_table_scalar(self, boxes, classes, masks):
        """The table pair by pair, from box_iou / mask_iou."""
        old = self.tracks
        table = np.zeros((len(old), len(boxes)), dtype=np.float64)
        for i, tr in enumerate(old):
            for j in range(len(boxes)):
                if tr["cls"] != int(classes[j]):
                    continue
                table[i, j] = box_iou(tr["box"], boxes[j]) if self.match == "box" else mask_iou(tr["mask"], masks[j])
        return table

    def iou_table(self, boxes, classes, masks):
        """The same table as whole-array float64 operations (NumPy rounds every operation on its own, as the scalars do); the CPU tests
        hold the two equal bit for bit."""
        old = self.tracks
        t, n = len(old), len(boxes)
        if t == 0 or n == 0:
            return np.zeros((t, n), dtype=np.float64)
        same = np.array([tr["cls"] for tr in old], dtype=np.int64)[:, None] == np.asarray(classes, dtype=np.int64)[None, :]
        with np.errstate(all="ignore"):
            if self.match == "box":
                o = np.array([tr["box"] for tr in old], dtype=np.float32).astype(np.float64)[:, None, :]
                b = np.asarray(boxes, dtype=np.float32).astype(np.float64)[None, :, :]
                ok = ~(np.isnan(o).any(axis=2) | np.isnan(b).any(axis=2))
                iw = np.minimum(o[..., 2], b[..., 2]) - np.maximum(o[..., 0], b[..., 0])
                ih = np.minimum(o[..., 3], b[..., 3]) - np.maximum(o[..., 1], b[..., 1])
                inter = np.where((iw > 0.0) & (ih > 0.0), iw * ih, 0.0)
                union = (o[..., 2] - o[..., 0]) * (o[..., 3] - o[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter
            else:
                om = np.array([tr["mask"].reshape(-1) for tr in old], dtype=np.int64)
                nm = np.asarray(masks, dtype=bool).reshape(n, -1).astype(np.int64)
                inter = (om @ nm.T).astype(np.float64)
                union = (om.sum(axis=1)[:, None] + nm.sum(axis=1)[None, :]).astype(np.float64) - inter        # integers below 2^53: exact
                ok = np.ones((t, n), dtype=bool)
            v = inter / union
        v = np.where(ok & same & (union != 0.0) & ~np.isnan(v), v, 0.0)
        return v

    def update(self, boxes, classes, masks=None):
        boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
        n = len(boxes)
        assert n <= self.max_tracks
        new = [dict(box=boxes[j].copy(), cls=int(classes[j]), id=None, ttl=self.ttl, mask=None if masks is None else np.asarray(masks[j], dtype=bool).copy())
               for j in range(n)]
        table = self.iou_table(boxes, classes, masks)
        extras = []
        for i, tr in enumerate(self.tracks):                          # old instances in index order
            matched = False
            if n:
                j = int(np.argmax(table[i]))                          # the first j that attains the row maximum
                if table[i, j] > self.threshold and new[j]["id"] is None:       # "if the new one has no id yet"
                    new[j]["id"] = tr["id"]
                    matched = True
            if not matched:
                tr = dict(tr, ttl=tr["ttl"] - 1)
                if tr["ttl"] > 0:
                    extras.append(tr)
        for inst in new:                                              # unmatched new instances, in order of j
            if inst["id"] is None:
                inst["id"] = self.next_id
                self.next_id += 1
        room = self.max_tracks - n
        self.dropped += max(0, len(extras) - room)
        self.tracks = new + extras[:room]
        return np.array([inst["id"] for inst in new], dtype=np.int32)

    # the table as arrays, for comparison with the device's
    def arrays(self):
        t = self.tracks
        out = dict(boxes=np.array([tr["box"] for tr in t], dtype=np.float32).reshape(-1, 4), classes=np.array([tr["cls"] for tr in t], dtype=np.int64),
                   ids=np.array([tr["id"] for tr in t], dtype=np.int32), ttl=np.array([tr["ttl"] for tr in t], dtype=np.int32))
        if self.match == "mask":
            out["masks"] = np.array([tr["mask"] for tr in t], dtype=bool)
            out["areas"] = np.array([int(np.count_nonzero(tr["mask"])) for tr in t], dtype=np.int32)
        return out


def mask_values(inter, old_areas, new_areas):
    """The mask-mode value table of cmk_vis_track_assign: inter[i][j] / (old_areas[i] + new_areas[j] - inter[i][j]) in float64 from
    Python integers, a zero union gives 0."""
    rows, n = len(old_areas), len(new_areas)
    out = np.zeros((rows, n), dtype=np.float64)
    for i in range(rows):
        for j in range(n):
            it = int(inter[i][j])
            u = int(old_areas[i]) + int(new_areas[j]) - it
            out[i, j] = 0.0 if u == 0 else float(np.float64(it) / np.float64(u))
    return out


def assign_tables(value, old, counters, new, n, cap, ttl, threshold):
    """One frame of the association rule of include/cmk.h (cmk_vis_track_assign) on tables, in plain loops.  value: (rows, n) float64,
    the iou table or mask_values(...), before the class gate; old / new: dicts of boxes (., 4) float32, classes, and for old ids and ttl,
    `rows` and `n` rows long; counters: the four int32.  -> (out table as a dict of boxes, classes, ids, ttl with the new n_tracks rows,
    src, track_ids, counters)."""
    rows = len(old["classes"])
    tracks = min(max(int(counters[0]), 0), rows)
    next_id, dropped = int(counters[1]), int(counters[2])
    best = [-1] * tracks
    for i in range(tracks):
        top, at = None, -1
        for j in range(n):
            v = float(value[i][j]) if int(old["classes"][i]) == int(new["classes"][j]) else 0.0
            if v != v:
                v = 0.0
            if at < 0 or v > top:                                    # the first j that attains the row maximum
                top, at = v, j
        if at >= 0 and top > threshold:
            best[i] = at
    owner = [None] * n
    for i in range(tracks):                                          # in index order: the smallest candidate i claims j
        if best[i] >= 0 and owner[best[i]] is None:
            owner[best[i]] = i
    track_ids = []
    for j in range(n):
        if owner[j] is None:
            track_ids.append(next_id)
            next_id += 1
        else:
            track_ids.append(int(old["ids"][owner[j]]))
    table = [(new["boxes"][j], int(new["classes"][j]), track_ids[j], int(ttl), j) for j in range(n)]
    extras = []
    for i in range(tracks):
        if best[i] >= 0 and owner[best[i]] == i:
            continue
        left = int(old["ttl"][i]) - 1
        if left > 0:
            extras.append((old["boxes"][i], int(old["classes"][i]), int(old["ids"][i]), left, n + i))
    room = cap - n
    dropped += max(0, len(extras) - room)
    table += extras[:room]
    out = dict(boxes=np.array([r[0] for r in table], dtype=np.float32).reshape(-1, 4), classes=np.array([r[1] for r in table], dtype=np.int64),
               ids=np.array([r[2] for r in table], dtype=np.int64).astype(np.int32), ttl=np.array([r[3] for r in table], dtype=np.int32))
    src = np.array([r[4] for r in table], dtype=np.int32)
    new_counters = np.array([len(table), next_id, dropped, int(counters[3])], dtype=np.int64).astype(np.int32)
    return out, src, np.array(track_ids, dtype=np.int64).astype(np.int32), new_counters


def gather_rows(src, n_tracks, old_words, old_areas, new_words, new_areas, n, cap, rows):
    """cmk_vis_track_gather as a plain copy: {out row s: (words, area)} for s < min(n_tracks, cap, rows) whose src[s] names a new instance
    (0 <= v < n) or an old row (n <= v < n + cap); every other row is not written."""
    out = {}
    for s in range(max(0, min(int(n_tracks), cap, rows))):
        v = int(src[s])
        if 0 <= v < n:
            out[s] = (np.array(new_words[v]), int(new_areas[v]))
        elif n <= v < n + cap:
            out[s] = (np.array(old_words[v - n]), int(old_areas[v - n]))
    return out


def sequence(n, frames=12, seed=0, size=(480, 640), with_masks=False, pool_factor=1.5):
    """A seeded sequence of `frames` frames of about n instances: a pool of objects (boxes inside `size`, 3 classes), of which every frame
    shows a shuffled subset with jitter: mostly small (the IoU stays above the thresholds), sometimes large (it does not).  On purpose:
    frame 5 is empty and frame 8 shows half as many; some objects are exact duplicates of others (ties in a row, two old rows claiming
    one new instance), some duplicates differ only in class (IoU 1, no match), one box of the pool has a NaN, one is empty.  Masks are the
    boxes' pixel rectangles (an empty box gives an empty mask).  -> a list of dicts of boxes (m,4) float32, classes (m,) int64, scores
    (m,) float32 and masks (m,h,w) bool or None."""
    rng = np.random.RandomState(seed)
    h, w = size
    pool = max(int(n * pool_factor), n)
    x1, y1 = rng.uniform(0, 0.8 * w, pool), rng.uniform(0, 0.8 * h, pool)
    bw, bh = rng.uniform(0.1 * w, 0.4 * w, pool), rng.uniform(0.1 * h, 0.4 * h, pool)
    boxes = np.stack([x1, y1, np.minimum(x1 + bw, w), np.minimum(y1 + bh, h)], axis=1).astype(np.float32)
    classes = rng.randint(0, 3, pool).astype(np.int64)
    for k in range(3, pool, 7):                                      # duplicates of the object before, every other one of another class
        boxes[k] = boxes[k - 1]
        classes[k] = classes[k - 1] if (k // 7) % 2 == 0 else (classes[k - 1] + 1) % 3
    if pool > 4:
        boxes[4, 1] = np.nan
    if pool > 5:
        boxes[5, 2:] = boxes[5, :2]
    out = []
    for f in range(frames):
        m = 0 if f == 5 else (n // 2 if f == 8 else n)
        pick = rng.permutation(pool)[:m]
        big = rng.rand(m) < 0.15
        jitter = rng.uniform(-1, 1, (m, 4)) * np.where(big, 0.25 * min(h, w), 0.01 * min(h, w))[:, None]
        jitter[rng.rand(m) < 0.3] = 0.0                              # some do not move at all: IoU exactly 1
        b = (boxes[pick] + jitter.astype(np.float32)).astype(np.float32)
        b[pick == 5] = boxes[5] if pool > 5 else 0                   # the empty box stays empty
        masks = None
        if with_masks:
            masks = np.zeros((m, h, w), dtype=bool)
            for j in range(m):
                if not np.isnan(b[j]).any():
                    c = np.clip(np.floor(b[j]), 0, [w, h, w, h]).astype(int)
                    masks[j, c[1]:c[3], c[0]:c[2]] = True
        out.append(dict(boxes=b, classes=classes[pick].copy(), scores=rng.uniform(0.1, 1.0, m).astype(np.float32), masks=masks))
    return out


def pack_words(masks):
    """(R,h,w) bool -> (R, ceil(h*w/64)) int64: bit p % 64 of word p / 64 is the row-major pixel p, unused high bits zero."""
    masks = np.asarray(masks, dtype=bool)
    r = masks.shape[0]
    hw = int(np.prod(masks.shape[1:]))
    nw = (hw + 63) // 64
    bits = np.zeros((r, nw * 64), dtype=np.uint8)
    bits[:, :hw] = masks.reshape(r, hw)
    return np.packbits(bits.reshape(r, nw, 64), axis=2, bitorder="little").reshape(r, nw, 8).copy().view("<u8").reshape(r, nw).astype(np.uint64).view(np.int64)
