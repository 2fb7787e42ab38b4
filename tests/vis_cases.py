"""The conformance table of csrc/visualize.hip: the visualizer (vis_prepare, vis_compose, three vis_kp_*), the video tracker
(vis_track_iou, vis_track_assign, vis_track_gather) and the nine vis_contour_* kernels, through their seven entries.  One row per case,
in the shape of tests/image_cases.py: the C entry, the kernels it launches (their cmk:: names as `nm -C` prints them), the geometry, the
feature cell, the answer the library is declared to give (accept or refuse) and `expect`, the quantity the row exists for, restated here
from the launch code (geometry()) and asserted by the CPU module.  Plain data plus call().  No tests here:
tests/test_cpu_vis_conformance.py checks the census, the cells, the restated geometry, the byte caps and every refusal on dummy pointers,
tests/test_gpu_vis_conformance.py launches every row on guarded buffers against its reference.

A row is a dict (case() gives the defaults of its entry, DEFAULTS):
  entry, feature, answer "accept" | "refuse", kernels [names], why, data (how the GPU module fills the inputs), null (the pointer handed
  in as NULL), host_only (a refusal whose buffers no test allocates), wrapper (the census row of cmk_vis_prepare), expect {name: value of
  geometry(row)}, and the arguments of its entry under the names of DEFAULTS[entry].  *_off arguments are BYTE offsets of a pointer
  (in_off and out_off of the compose are where the GPU module's buffers start, the others are added by call()); overlap = (out pointer,
  in pointer, k): the out pointer handed in is the in pointer plus k rows of its table (k times 16 bytes in the contour pair; for the
  compose an int, image_out that many image rows into image_in, -1 for the same address)."""
import ctypes

ENTRIES = ["cmk_vis_prepare_ids", "cmk_vis_compose", "cmk_vis_keypoints", "cmk_vis_track_iou_boxes", "cmk_vis_track_assign",
           "cmk_vis_track_gather", "cmk_vis_contour_count+cmk_vis_contour_trace"]
PREP, COMP, KP, IOU, ASSIGN, GATHER, CONT = ENTRIES
WRAPPER = "cmk_vis_prepare"          # cmk_vis_prepare_ids with a null color_ids: one census row, bit-equal to the _ids call
FILES = ("visualize.hip",)

FEATURES = [
    "census",        # one plain accepted case per kernel
    "unaligned",     # a buffer that starts at a byte offset the fast path does not accept
    "edge",          # the smallest geometries at which the index arithmetic or the algorithm branches
    "second_trip",   # a loop over rounds, trips or a capped grid takes a second iteration
    "ties",          # equal values where the rule names the winner
    "clamped",       # a bad value in an argument the header promises to clamp: nothing outside the inputs is read, nothing outside the outputs written
    "nonfinite",     # NaN and Inf: the answer is what the restatement gives
    "refuse",        # CMK_EINVAL with an error text, nothing launched
]

CMK_EINVAL = -1
REC_INTS = 28
TOO_BIG = 46341                      # 46341^2 >= 2^31 - 1
MAX_BYTES = 64 << 20                 # no buffer of an accepted row is larger
BIG_BYTES = 8 << 20                  # ... and one row alone is above this: the 725 x 725 checkerboard
INT32_MIN, INT32_MAX, INT64_MIN, INT64_MAX = -2 ** 31, 2 ** 31 - 1, -2 ** 63, 2 ** 63 - 1

DEFAULTS = {
    PREP: dict(n=5, h=48, w=64, num_names=3, font_scale=1, by_class=0, ids=1),
    COMP: dict(h=37, w=70, n=5, words=1, alpha256=128, line_width=2, font_scale=1, in_off=0, out_off=0, rec_off=0, overlap=0),
    KP: dict(h=40, w=60, n=3, k=17, s=19, line_width=2, thr=0.05),
    IOU: dict(rows=5, n=7),
    ASSIGN: dict(n=5, rows=7, cap=16, ttl=8, thr=0.6, mode="box", tracks=None, next_id=100, overlap=None),      # tracks: counters[0] (None: rows)
    GATHER: dict(n=3, rows=6, cap=8, h=5, w=13, tracks=None, overlap=None),
    CONT: dict(r=5, h=13, w=67, phase="both", ws_off=0, ws_short=0, sc_off=0, sc_short=0, host=None, overlap=None),      # host: the trace's n_corners
}

N_A = {}
for _e in ENTRIES:
    if _e != COMP:
        N_A[(_e, "unaligned")] = "typed loads and stores at the natural alignment of int32, float, int64 and double, no path that a byte offset " \
                                 "would leave; the alignments the entries demand (records, ws, scratch) are refuse rows"
    if _e in (PREP, IOU, ASSIGN):
        N_A[(_e, "second_trip")] = "the grid covers the work one to one; the row and lane trips inside the assign workgroup are edge and ties rows" \
            if _e != PREP else "one thread per instance, the grid covers them one to one (n = 65 and 130 are edge rows)"
    if _e not in (ASSIGN,):
        N_A[(_e, "ties")] = "no rule of the entry picks between equal values" + \
                            (" (draw order is the records' order; two instances on one pixel are second_trip rows)" if _e == COMP else
                             " (the latest primitive wins a pixel: an edge row)" if _e == KP else "")
    if _e in (COMP, IOU):
        N_A[(_e, "clamped")] = "glyph bytes are the one clamp and records that vis_prepare did not write are outside the precondition" \
            if _e == COMP else "boxes in, a table out: no index or count is read on the device"
    if _e in (COMP, GATHER, CONT):
        N_A[(_e, "nonfinite")] = "integer kernel: bytes, bits and int32 in, integers out"
del _e
NO_ROW = {"the link kernel's grid cap (2^22 workgroups)": "needs T > 2^24 corners, a scratch of 800 MB: the checkerboard row reaches 2^20",
          "a count of corners beyond int32 (n_corners = -1)": "needs a mask of more than 2^31 corners"}
PRECONDITIONS = {
    PREP: "typed pointers hold their natural alignment (float, int32 4 bytes, int64 8): a misaligned one has no row",
    COMP: "records are what vis_prepare wrote: the original index (the row of `words`) is not checked again, so other records have no row",
    KP: "records are what vis_prepare wrote (the original index selects the keypoints and is not checked again)",
    ASSIGN: "src, track_ids and counters alias no other argument; typed pointers hold their natural alignment",
    GATHER: "src and counters alias no other argument",
    CONT: "words hold zero in the unused high bits of the last word, as the two producers write them",
}

CONTOUR_COUNT = ["vis_contour_count_kernel", "vis_contour_offsets_kernel"]
CONTOUR_TRACE = ["vis_contour_emit_kernel", "vis_contour_link_kernel", "vis_contour_jump_kernel", "vis_contour_lens_kernel",
                 "vis_contour_blocks_kernel", "vis_contour_place_kernel", "vis_contour_write_kernel"]
AWKWARD = [(1, 1), (1, 200), (200, 1), (5, 7), (13, 67), (64, 64), (3, 130)]           # tests/test_gpu_contours.py::test_awkward_word_alignment


def cdiv(a, b):
    return -(-a // b)


def nwords(h, w):
    return (h * w + 63) // 64


def contour_lw(w):
    return (w + 1 + 63) // 64


def contour_ws_bytes(r, h, w):
    """cmk_vis_contour_ws_bytes restated: R + 1 int64 offsets, an int64 per (mask, 1024 lattice words), an int32 per (mask, lattice word)."""
    ne = (h + 1) * contour_lw(w)
    return 8 * (r + 1) + 8 * r * cdiv(ne, 1024) + 4 * r * ne


def trace_ws_bytes(t):
    """cmk_vis_contour_trace_ws_bytes restated: 16 T of corner records, 8 x 4 T of links and ranks, an int32 per 1024 records."""
    return 0 if t <= 0 else 48 * t + 4 * cdiv(t, 1024)


def checker_corners(side, parity):
    """The corners of a side x side checkerboard whose pixel (0, 0) is set iff parity == 0: four per set pixel, every one its own loop."""
    return 4 * ((side * side + 1 - parity) // 2)


def stream_grid(items):
    return min(max(cdiv(items, 256), 1), 4096)


def corners_known(c):
    """T of a contour row whose data has a formula, else None."""
    if c["data"].startswith("checker"):
        return checker_corners(c["h"], int(c["data"][-1]))
    if c["data"] == "full":
        return 4 * c["r"]
    if c["data"] == "alternate":
        return 4 * ((c["r"] + 1) // 2)
    return None


def geometry(c):
    """What the launch code makes of a row's arguments, restated: the names a row's `expect` may use."""
    e = c["entry"]
    if e == PREP:
        return dict(blocks=cdiv(c["n"], 64), last=c["n"] - 64 * ((c["n"] - 1) // 64))
    if e == COMP:
        hw = c["h"] * c["w"]
        vec = int(c["in_off"] % 4 == 0 and c["out_off"] % 4 == 0)
        return dict(nw=nwords(c["h"], c["w"]), vec=vec, rounds=cdiv(c["n"], 64), full=(hw // 64) * vec, tail=hw % 64, grid=cdiv(nwords(c["h"], c["w"]), 4))
    if e == KP:
        hw = c["h"] * c["w"]
        return dict(prims=c["n"] * (c["s"] + c["k"]), grid=stream_grid(hw), trips=cdiv(hw, 256 * stream_grid(hw)))
    if e == IOU:
        pairs = c["rows"] * c["n"]
        return dict(pairs=pairs, blocks=cdiv(pairs, 256), last=pairs - 256 * ((pairs - 1) // 256) if pairs else 0)
    if e == ASSIGN:
        t = min(max(c["rows"] if c["tracks"] is None else c["tracks"], 0), c["rows"])
        return dict(T=t, row_trips=cdiv(t, 16), lane_trips=cdiv(c["n"], 64))
    if e == GATHER:
        nw = nwords(c["h"], c["w"])
        gx = min(cdiv(nw, 256), 256)
        return dict(nw=nw, gx=gx, trips=cdiv(nw, 256 * gx))
    if e == CONT:
        lw = contour_lw(c["w"])
        ne = (c["h"] + 1) * lw
        nb = cdiv(ne, 1024)
        g = dict(LW=lw, NE=ne, NB=nb, offsets_trips=cdiv(max(c["r"], 0) * nb, 1024), link_trips=cdiv(c["h"], 64) + 1)
        t = corners_known(c)
        if t is not None:
            longest = t if c["r"] == 1 else 4
            g.update(T=t, nb=cdiv(t, 1024), blocks_trips=cdiv(cdiv(t, 1024), 1024), jump_rounds=max(0, (longest - 1).bit_length()), scratch=trace_ws_bytes(t))
        return g
    raise KeyError(e)


def kernels_of(c):
    """The kernels an accepted row launches."""
    e = c["entry"]
    if e == PREP:
        return ["vis_prepare_kernel"] if c["n"] else []
    if e == COMP:
        return ["vis_compose_kernel"]
    if e == KP:
        return ["vis_kp_clear_kernel", "vis_kp_raise_kernel", "vis_kp_colour_kernel"] if c["n"] else []
    if e == IOU:
        return ["vis_track_iou_kernel"] if c["rows"] and c["n"] else []
    if e == ASSIGN:
        return ["vis_track_assign_kernel"]
    if e == GATHER:
        return ["vis_track_gather_kernel"] if c["rows"] else []
    if e == CONT:
        if not c["r"]:
            return []
        return CONTOUR_COUNT + (CONTOUR_TRACE if c["data"] != "empty" else [])
    raise KeyError(e)


def case(entry, feature, why="", data="", null=None, host_only=False, wrapper=False, expect=None, **kw):
    c = dict(DEFAULTS[entry])
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    c.update(id="", entry=entry, feature=feature, answer="refuse" if feature == "refuse" else "accept", why=why, data=data, null=null,
             host_only=host_only, wrapper=wrapper, expect=dict(expect or {}), kernels=[])
    if c["answer"] == "accept":
        c["kernels"] = kernels_of(c)
    return c


# the pointers of each entry (the names call() takes) in the order of the C signature(s)
POINTERS = {
    PREP: ("boxes", "scores", "classes", "order", "names", "name_lens", "palette", "color_ids", "records"),
    COMP: ("image_in", "image_out", "words", "records", "font"),
    KP: ("image", "keypoints", "records", "skeleton", "winner"),
    IOU: ("old_boxes", "new_boxes", "iou"),
    ASSIGN: ("iou", "inter", "old_areas", "new_areas", "old_boxes", "old_classes", "old_ids", "old_ttl", "new_boxes", "new_classes", "out_boxes",
             "out_classes", "out_ids", "out_ttl", "src", "track_ids", "counters"),
    GATHER: ("src", "counters", "old_words", "old_areas", "new_words", "new_areas", "out_words", "out_areas"),
    CONT: ("words", "ws", "n_corners", "host_corners", "scratch", "xy", "head"),
}
HOST_ARRAYS = ("host_corners",)                      # built by call() on the host: a row can only NULL it
NULLABLE = {e: POINTERS[e] for e in ENTRIES}
NULLABLE[PREP] = tuple(p for p in POINTERS[PREP] if p != "color_ids")          # a null color_ids is cmk_vis_prepare: the wrapper's census row
NULLABLE[COMP] = ("image_in", "image_out", "records", "font")                  # a null words draws no masks: an accepted row
# the pair of tables has its own rows (both, neither), the areas are mask mode's (box mode hands none in)
NULLABLE[ASSIGN] = tuple(p for p in POINTERS[ASSIGN] if p not in ("iou", "inter", "old_areas", "new_areas"))
COUNT_PHASE = ("words", "ws", "n_corners")
# the four arrays of the track table and the element bytes of a row of each
TABLE_ARRAYS = {"boxes": 16, "classes": 8, "ids": 4, "ttl": 4}


def _nulls(entry, **kw):
    rows = []
    for p in NULLABLE[entry]:
        if entry == CONT:
            rows += [case(entry, "refuse", "null {} ({})".format(p, ph), null=p, **dict(kw, phase=ph)) for ph in ("count", "trace")
                     if (ph == "trace" and p != "n_corners") or (ph == "count" and p in COUNT_PHASE)]
        else:
            rows.append(case(entry, "refuse", "null " + p, null=p, **kw))
    return rows


def _image_refusals(entry, **kw):
    return [case(entry, "refuse", "H = 0", **dict(kw, h=0)), case(entry, "refuse", "W = 0", **dict(kw, w=0)), case(entry, "refuse", "H = -1", **dict(kw, h=-1)),
            case(entry, "refuse", "H*W >= 2^31 - 1", host_only=True, **dict(kw, h=TOO_BIG, w=TOO_BIG))]


def _prepare_rows():
    r = [case(PREP, "census", "five instances, three names, colours by the caller's ids", data="plain", expect=dict(blocks=1)),
         case(PREP, "census", "cmk_vis_prepare: the _ids call with a null color_ids, bit for bit", data="plain", ids=0, wrapper=True)]
    for n in (1, 63, 64, 65, 130):
        r.append(case(PREP, "edge", "n = {}: {} workgroup{} of 64, {} in the last".format(n, cdiv(n, 64), "s" if n > 64 else "", n - 64 * ((n - 1) // 64)),
                      data="plain", n=n, expect=dict(blocks=cdiv(n, 64), last=n - 64 * ((n - 1) // 64))))
    r += [case(PREP, "edge", "n = 0 returns OK and touches nothing", n=0),
          case(PREP, "edge", "names of 0, 32 and 40 glyphs: the label is cut at 32", data="names"),
          case(PREP, "edge", "classes outside the names, both signs, and the two int64 extremes (C-9223372036854775808 0%)", data="classes", n=8),
          case(PREP, "edge", "no names at all: num_names = 0 with null names and name_lens", data="plain", num_names=0),
          case(PREP, "edge", "scores 0.004999, 0.005, 0.995, 1.0, 1e30 and their negatives", data="scores", n=10),
          case(PREP, "edge", "plates clamped at both edges of the image", data="plates", n=6),
          case(PREP, "edge", "an image smaller than any plate, 5 x 3", data="plates", n=6, h=3, w=5),
          case(PREP, "edge", "font_scale 16", data="plates", n=6, h=200, w=300, font_scale=16),
          case(PREP, "edge", "color_by_class = 1 without ids", data="classes", n=8, by_class=1, ids=0),
          case(PREP, "edge", "color_ids negative, INT32_MIN and INT32_MAX: the remainder is the non-negative one", data="ids", n=6),
          case(PREP, "clamped", "order holding -1, n, 2^40 and duplicates: such a j draws instance j, nothing outside the inputs is read", data="order", n=7),
          case(PREP, "clamped", "name_lens of -5 and 99 and glyph bytes of 41 and 255", data="lens"),
          case(PREP, "nonfinite", "NaN, +Inf and -Inf in each box coordinate: a NaN box has no frame and no label, an Inf is clamped to 2^20", data="nonfinite_boxes", n=12),
          case(PREP, "nonfinite", "NaN, +Inf and -Inf scores: 0 %, 100 %, 0 %", data="nonfinite_scores", n=3)]
    small = dict(n=2, data="plain")
    r += _nulls(PREP, **small)
    r += _image_refusals(PREP, **small)
    r += [case(PREP, "refuse", "n = -1", **dict(small, n=-1)), case(PREP, "refuse", "n = 65536", **dict(small, n=65536)),
          case(PREP, "refuse", "font_scale = 0", font_scale=0, **small), case(PREP, "refuse", "font_scale = 17", font_scale=17, **small),
          case(PREP, "refuse", "num_names = -1", num_names=-1, **small), case(PREP, "refuse", "num_names = 65536", num_names=65536, **small)]
    return r


COMPOSE_SHAPES = [(3, 5), (8, 8), (5, 13), (37, 70), (16, 64), (40, 129)]            # H*W = 15, 64, 65, 2590, 1024, 5160


def _compose_rows():
    r = [case(COMP, "census", "37 x 70, five instances with masks: 40 full words and a tail of 30 pixels", data="scene", expect=dict(nw=41, vec=1, full=40, tail=30, rounds=1))]
    for h, w in COMPOSE_SHAPES:
        hw = h * w
        r.append(case(COMP, "edge", "H*W = {}: {} full word{} and a tail of {}".format(hw, hw // 64, "" if hw // 64 == 1 else "s", hw % 64), data="scene", h=h, w=w, n=3,
                      expect=dict(full=hw // 64, tail=hw % 64)))
    r += [case(COMP, "edge", "n = 0 copies the image", data="scene", n=0, expect=dict(rounds=0)),
          case(COMP, "edge", "n = 1", data="scene", n=1, expect=dict(rounds=1)),
          case(COMP, "edge", "n = 64: one full round of instances", data="rounds", h=40, w=129, n=64, expect=dict(rounds=1)),
          case(COMP, "edge", "words null: boxes and labels alone", data="scene", words=0),
          case(COMP, "edge", "alpha256 = 0: the fill keeps the pixel, the outline stays", data="scene", alpha256=0),
          case(COMP, "edge", "alpha256 = 256: the fill is the colour", data="scene", alpha256=256),
          case(COMP, "edge", "line_width 1 and font_scale 1 on 16 x 64", data="scene", h=16, w=64, line_width=1),
          case(COMP, "edge", "line_width 16 and font_scale 16 on 160 x 300", data="scene", h=160, w=300, n=3, line_width=16, font_scale=16),
          case(COMP, "second_trip", "n = 65: the second round of 64 instances holds one; words that only it touches, words one instance of each "
               "round touches", data="rounds", h=40, w=129, n=65, expect=dict(rounds=2)),
          case(COMP, "second_trip", "n = 129: a third round of one instance", data="rounds", h=40, w=129, n=129, expect=dict(rounds=3))]
    for off in (1, 2, 3):
        r.append(case(COMP, "unaligned", "image_in {} byte{} off a dword: the scalar path, the bits of the aligned call".format(off, "s" if off > 1 else ""),
                      data="scene", in_off=off, expect=dict(vec=0, full=0)))
        r.append(case(COMP, "unaligned", "image_out {} byte{} off a dword: the scalar path, the bits of the aligned call".format(off, "s" if off > 1 else ""),
                      data="scene", out_off=off, expect=dict(vec=0, full=0)))
    r.append(case(COMP, "unaligned", "both images 4 bytes off: the vector path", data="scene", in_off=4, out_off=4, expect=dict(vec=1, full=40)))
    small = dict(h=5, w=13, n=2, data="scene")
    r += _nulls(COMP, **small)
    r += _image_refusals(COMP, **small)
    r += [case(COMP, "refuse", "n = -1", **dict(small, n=-1)), case(COMP, "refuse", "n = 65536", **dict(small, n=65536)),
          case(COMP, "refuse", "line_width = 0", line_width=0, **small), case(COMP, "refuse", "line_width = 17", line_width=17, **small),
          case(COMP, "refuse", "font_scale = 0", font_scale=0, **small), case(COMP, "refuse", "font_scale = 17", font_scale=17, **small),
          case(COMP, "refuse", "alpha256 = -1", alpha256=-1, **small), case(COMP, "refuse", "alpha256 = 257", alpha256=257, **small),
          case(COMP, "refuse", "records 4 bytes off a 16-byte boundary", rec_off=4, **small),
          case(COMP, "refuse", "records 8 bytes off a 16-byte boundary", rec_off=8, **small),
          case(COMP, "refuse", "image_out == image_in", overlap=-1, **small),
          case(COMP, "refuse", "image_out one image row into image_in", overlap=1, **small)]
    return r


def _keypoint_rows():
    r = [case(KP, "census", "three instances, 17 keypoints, the 19 segments of the COCO skeleton", data="pose", expect=dict(prims=108, trips=1))]
    for k, s in ((1, 0), (3, 4), (17, 19)):
        for lw in (1, 16):
            r.append(case(KP, "edge", "K = {}, S = {}, line_width {}".format(k, s, lw), data="pose", k=k, s=s, line_width=lw, h=64, w=96, expect=dict(prims=3 * (k + s))))
    r += [case(KP, "edge", "n = 0 returns OK and touches nothing", n=0),
          case(KP, "edge", "segments of zero length: both ends on one pixel", data="zero_length", k=3, s=4, n=2),
          case(KP, "edge", "segments across several 16 x 16 tiles at shallow and steep slopes, widths 1 and 16: the float tile skip beside the exact test",
               data="long", h=150, w=200, k=8, s=8, n=2, line_width=1),
          case(KP, "edge", "... at line_width 16", data="long", h=150, w=200, k=8, s=8, n=2, line_width=16),
          case(KP, "edge", "discs and segments of later instances over earlier ones: the latest primitive wins the pixel", data="stacked", k=3, s=4, n=3, line_width=5),
          case(KP, "second_trip", "1025 x 1024 with a handful of primitives: 1,049,600 pixels > 4096 x 256 threads in the clear and colour passes",
               data="pose", h=1025, w=1024, n=2, k=3, s=4, expect=dict(grid=4096, trips=2)),
          case(KP, "clamped", "skeleton indices -1, K and INT32_MAX draw nothing and read nothing", data="bad_skeleton", k=3, s=6, n=2),
          case(KP, "nonfinite", "NaN coordinates and scores hide a point; an Inf coordinate is clamped to +-32768: a segment from inside the image "
               "to x = 32768", data="nonfinite", k=6, s=5, n=2),
          case(KP, "nonfinite", "scores one ulp below, at and one ulp above the threshold: only the last is drawn", data="ulp", k=3, s=3, n=1)]
    small = dict(h=9, w=11, n=2, k=3, s=2, data="pose")
    r += _nulls(KP, **small)
    r += _image_refusals(KP, **small)
    r += [case(KP, "refuse", "n = -1", **dict(small, n=-1)), case(KP, "refuse", "n = 65536", **dict(small, n=65536)),
          case(KP, "refuse", "line_width = 0", line_width=0, **small), case(KP, "refuse", "line_width = 17", line_width=17, **small),
          case(KP, "refuse", "num_keypoints = 0", **dict(small, k=0)), case(KP, "refuse", "num_keypoints = 1025", **dict(small, k=1025)),
          case(KP, "refuse", "num_segments = -1", **dict(small, s=-1)), case(KP, "refuse", "num_segments = 4097", **dict(small, s=4097))]
    return r


def _iou_rows():
    r = [case(IOU, "census", "5 old rows against 7 new boxes", data="random", expect=dict(pairs=35, blocks=1))]
    for rows, n in ((1, 1), (15, 17), (16, 16), (1, 257)):
        r.append(case(IOU, "edge", "rows * n = {}: {} thread{} in the last workgroup".format(rows * n, rows * n - 256 * ((rows * n - 1) // 256), "" if rows * n in (1, 257) else "s"),
                      data="random", rows=rows, n=n, expect=dict(pairs=rows * n, blocks=cdiv(rows * n, 256))))
    r += [case(IOU, "edge", "rows = 0 returns OK and touches nothing", rows=0), case(IOU, "edge", "n = 0 returns OK and touches nothing", n=0),
          case(IOU, "edge", "zero-area boxes, touching boxes (iw == 0), boxes with x2 < x1, identical boxes, thirds that do not round", data="shapes", rows=8, n=8),
          case(IOU, "nonfinite", "NaN in each of the eight coordinates gives 0; Inf - Inf unions give 0; an Inf box against a finite one", data="nonfinite", rows=10, n=10)]
    small = dict(rows=2, n=3, data="random")
    r += _nulls(IOU, **small)
    r += [case(IOU, "refuse", "rows = -1", **dict(small, rows=-1)), case(IOU, "refuse", "rows = 1025", **dict(small, rows=1025)),
          case(IOU, "refuse", "n = -1", **dict(small, n=-1)), case(IOU, "refuse", "n = 1025", **dict(small, n=1025))]
    return r


ASSIGN_SHAPES = [(0, 0, 1), (1, 1, 1), (0, 5, 8), (5, 0, 8), (3, 8, 8), (65, 130, 130), (1024, 1024, 1024)]           # (n, rows, cap)


def _assign_rows():
    r = [case(ASSIGN, "census", "7 old rows, 5 new instances, a table with matches, misses and a class mismatch", data="random")]
    for n, rows, cap in ASSIGN_SHAPES:
        r.append(case(ASSIGN, "edge", "(n, rows, cap) = ({}, {}, {}): {} row trip{} per wave, {} lane trip{}".format(
            n, rows, cap, cdiv(rows, 16), "" if cdiv(rows, 16) == 1 else "s", cdiv(n, 64), "" if cdiv(n, 64) == 1 else "s"), data="random", n=n, rows=rows, cap=cap,
            expect=dict(T=rows, row_trips=cdiv(rows, 16), lane_trips=cdiv(n, 64))))
    r += [case(ASSIGN, "edge", "ttl = 1: a missed row does not survive (old ttl of 1 among them)", data="random", ttl=1),
          case(ASSIGN, "edge", "ttl = 255", data="random", ttl=255),
          case(ASSIGN, "edge", "overflow: 20 survivors for 6 free rows, dropped grows by 14", data="overflow", n=18, rows=20, cap=24, expect=dict(row_trips=2)),
          case(ASSIGN, "edge", "cap == n: no survivor fits", data="overflow", n=8, rows=8, cap=8),
          case(ASSIGN, "edge", "mask mode: inter with unions of 0 (empty masks) and an inter larger than either area", data="mask", mode="mask", n=6, rows=6, cap=16, thr=0.5),
          case(ASSIGN, "edge", "mask mode on the random table", data="random", mode="mask", thr=0.5)]
    big = dict(n=1024, rows=1024, cap=1024)
    mid = dict(n=130, rows=40, cap=256)
    r += [case(ASSIGN, "ties", "equal row maxima at j = (3, 67): one lane on two trips", data="tie_j:3,67", **mid),
          case(ASSIGN, "ties", "equal row maxima at j = (5, 6): neighbouring lanes", data="tie_j:5,6", **mid),
          case(ASSIGN, "ties", "equal row maxima at j = (63, 64): the last lane of a trip and the first of the next", data="tie_j:63,64", **mid),
          case(ASSIGN, "ties", "equal row maxima at j = (0, 1023)", data="tie_j:0,1023", **big),
          case(ASSIGN, "ties", "two old rows with the same best j at i = (2, 18): one wave, two trips", data="tie_i:2,18", **mid),
          case(ASSIGN, "ties", "two old rows with the same best j at i = (2, 3): two waves", data="tie_i:2,3", **mid),
          case(ASSIGN, "ties", "two old rows with the same best j at i = (0, 1023)", data="tie_i:0,1023", **big),
          case(ASSIGN, "ties", "a maximum exactly equal to the threshold is not a candidate; the next double above it is", data="at_threshold", n=4, rows=4, cap=8),
          case(ASSIGN, "ties", "threshold 0 with an all-zero row: no candidate", data="zero_row", thr=0.0, n=4, rows=4, cap=8),
          case(ASSIGN, "ties", "threshold 1: an IoU of exactly 1 is not above it", data="ones", thr=1.0, n=4, rows=4, cap=8),
          case(ASSIGN, "clamped", "counters[0] = -3: the table counts as empty", data="random", tracks=-3, expect=dict(T=0)),
          case(ASSIGN, "clamped", "counters[0] = rows + 5: clamped to rows", data="random", tracks=12, expect=dict(T=7)),
          case(ASSIGN, "clamped", "rows at and beyond n_tracks hold NaN boxes, a new instance's class and table value 1.0 and are never matched",
               data="stale", tracks=4, expect=dict(T=4)),
          case(ASSIGN, "nonfinite", "NaN (counts as 0), +Inf and -Inf in the iou table", data="nonfinite_table", n=6, rows=6, cap=16),
          case(ASSIGN, "nonfinite", "NaN and Inf boxes are carried through bit for bit, new and surviving", data="nonfinite_boxes")]
    small = dict(n=2, rows=3, cap=4, data="random")
    r += _nulls(ASSIGN, **small)
    r += [case(ASSIGN, "refuse", "null new_areas in mask mode", null="new_areas", **dict(small, mode="mask")),
          case(ASSIGN, "refuse", "null old_areas in mask mode", null="old_areas", **dict(small, mode="mask")),
          case(ASSIGN, "refuse", "both tables given", **dict(small, mode="both")), case(ASSIGN, "refuse", "neither table given", **dict(small, mode="neither")),
          case(ASSIGN, "refuse", "max_tracks = 0", **dict(small, cap=0)), case(ASSIGN, "refuse", "max_tracks = 1025", **dict(small, cap=1025)),
          case(ASSIGN, "refuse", "n above max_tracks", **dict(small, n=5)), case(ASSIGN, "refuse", "rows above max_tracks", **dict(small, rows=5)),
          case(ASSIGN, "refuse", "n = -1", **dict(small, n=-1)), case(ASSIGN, "refuse", "rows = -1", **dict(small, rows=-1)),
          case(ASSIGN, "refuse", "ttl = 0", ttl=0, **small), case(ASSIGN, "refuse", "ttl = 256", ttl=256, **small),
          case(ASSIGN, "refuse", "threshold -0.1", thr=-0.1, **small), case(ASSIGN, "refuse", "threshold 1.1", thr=1.1, **small),
          case(ASSIGN, "refuse", "threshold NaN", thr=float("nan"), **small)]
    for a in TABLE_ARRAYS:
        r += [case(ASSIGN, "refuse", "out_{0} == old_{0}".format(a), overlap=("out_" + a, "old_" + a, 0), **small),
              case(ASSIGN, "refuse", "out_{0} one row into old_{0}: the kernel would read rows that other threads have overwritten".format(a),
                   overlap=("out_" + a, "old_" + a, 1), **small),
              case(ASSIGN, "refuse", "out_{0} ending one row into old_{0}".format(a), overlap=("out_" + a, "old_" + a, -3), **small)]
    return r


def _gather_rows():
    r = [case(GATHER, "census", "six rows of a 5 x 13 frame from three new instances and the old table", data="mixed", expect=dict(nw=2, gx=1, trips=1))]
    for h, w, nw in ((8, 8, 1), (128, 128, 256), (128, 129, 258), (127, 129, 256)):
        r.append(case(GATHER, "edge", "nw = {}".format(nwords(h, w)), data="mixed", h=h, w=w, expect=dict(nw=nwords(h, w), trips=1)))
    r += [case(GATHER, "edge", "nw = 257: a second workgroup of one thread", data="mixed", h=257, w=64, expect=dict(nw=257, gx=2, trips=1)),
          case(GATHER, "edge", "rows = 0 returns OK and touches nothing", rows=0),
          case(GATHER, "edge", "n = 0: every row comes from the old table, new_words and new_areas null", data="mixed", n=0),
          case(GATHER, "second_trip", "a 2049 x 2048 frame: 65568 words a row > 256 x 256 threads", data="mixed", n=1, rows=2, cap=2, h=2049, w=2048,
               expect=dict(nw=65568, gx=256, trips=2)),
          case(GATHER, "clamped", "src values of -1, n + cap and INT32_MAX leave their rows as filler", data="bad_src"),
          case(GATHER, "clamped", "counters[0] above cap and above rows: the grid and cap bound the rows", data="mixed", tracks=100),
          case(GATHER, "clamped", "counters[0] = -2: nothing is written", data="mixed", tracks=-2)]
    small = dict(n=2, rows=3, cap=4, data="mixed")
    r += _nulls(GATHER, **small)
    r += _image_refusals(GATHER, **small)
    r += [case(GATHER, "refuse", "max_tracks = 0", **dict(small, cap=0)), case(GATHER, "refuse", "max_tracks = 1025", **dict(small, cap=1025)),
          case(GATHER, "refuse", "n above max_tracks", **dict(small, n=5)), case(GATHER, "refuse", "rows above max_tracks", **dict(small, rows=5)),
          case(GATHER, "refuse", "n = -1", **dict(small, n=-1)), case(GATHER, "refuse", "rows = -1", **dict(small, rows=-1))]
    for o, i in (("out_words", "old_words"), ("out_words", "new_words"), ("out_areas", "old_areas")):
        r += [case(GATHER, "refuse", "{} == {}".format(o, i), overlap=(o, i, 0), **small),
              case(GATHER, "refuse", "{} one row into {}".format(o, i), overlap=(o, i, 1), **small)]
    return r


def _contour_rows():
    r = [case(CONT, "census", "13 x 67: noise at three densities, a blob and the full mask; rows across two words of the lattice", data="awkward",
              expect=dict(LW=2, NE=28, NB=1, link_trips=2))]
    for h, w in AWKWARD:
        if (h, w) != (13, 67):
            r.append(case(CONT, "edge", "{} x {}: {} lattice word{} a row".format(h, w, contour_lw(w), "" if contour_lw(w) == 1 else "s"), data="awkward", h=h, w=w,
                          expect=dict(LW=contour_lw(w))))
    r += [case(CONT, "edge", "W = 63 and W = 64: the lattice row of 64 and of 65 vertices", data="awkward", h=5, w=63, expect=dict(LW=1)),
          case(CONT, "edge", "... W = 64", data="awkward", h=5, w=64, expect=dict(LW=2)),
          case(CONT, "edge", "1024 x 1 full: NE = 1025, the block boundary falls inside the mask; one vertical edge of 1024 rows takes 17 link trips", data="full",
               r=1, h=1024, w=1, expect=dict(NE=1025, NB=2, link_trips=17, T=4))]
    for h in (63, 64, 65, 128, 129):
        r.append(case(CONT, "edge", "columns of height {}: vertical edges around the ballot boundary, {} link trips".format(h, cdiv(h, 64) + 1), data="columns", r=3, h=h, w=5,
                      expect=dict(link_trips=cdiv(h, 64) + 1)))
    r += [case(CONT, "edge", "R = 0 returns OK and touches nothing", r=0),
          case(CONT, "edge", "empty masks: every total is 0 and the trace launches nothing", data="empty", r=3, h=5, w=7),
          case(CONT, "second_trip", "R = 1025 masks of 1 x 1, alternately set: R * NB = 1025, the offsets kernel's second trip holds one block total", data="alternate",
               r=1025, h=1, w=1, expect=dict(NB=1, offsets_trips=2, T=2052)),
          case(CONT, "second_trip", "R = 513 full masks of 1024 x 1: R * NB = 1026", data="full", r=513, h=1024, w=1, expect=dict(NB=2, offsets_trips=2, T=2052)),
          case(CONT, "second_trip", "a 725 x 725 checkerboard, the smallest side with T > 2^20: nb = 1027, the blocks kernel's second trip; 21 jump rounds; "
               "one unit square per set pixel in row-major order", data="checker0", r=1, h=725, w=725,
               expect=dict(T=1051252, nb=1027, blocks_trips=2, jump_rounds=21, scratch=50464204)),
          case(CONT, "clamped", "the host's n_corners smaller than the device's totals (even): nothing is written outside [0, T)", data="awkward", host="smaller"),
          case(CONT, "clamped", "the host's n_corners larger than the device's totals (even): records nobody wrote link to themselves", data="awkward", host="larger")]
    small = dict(r=2, h=5, w=7, data="awkward")
    r += _nulls(CONT, **small)
    for ph in ("count", "trace"):
        s = dict(small, phase=ph)
        r += [case(CONT, "refuse", "H = 0 ({})".format(ph), **dict(s, h=0)), case(CONT, "refuse", "W = 0 ({})".format(ph), **dict(s, w=0)),
              case(CONT, "refuse", "R = -1 ({})".format(ph), **dict(s, r=-1)), case(CONT, "refuse", "R = 65536 ({})".format(ph), **dict(s, r=65536)),
              case(CONT, "refuse", "H*W >= 2^31 - 1 ({})".format(ph), host_only=True, **dict(s, h=TOO_BIG, w=TOO_BIG)),
              case(CONT, "refuse", "ws_bytes one short ({})".format(ph), ws_short=1, **s),
              case(CONT, "refuse", "ws at byte offset 4 ({})".format(ph), ws_off=4, **s)]
    t = dict(small, phase="trace")
    r += [case(CONT, "refuse", "scratch at byte offset 8", sc_off=8, **t), case(CONT, "refuse", "scratch_bytes one short", sc_short=1, **t),
          case(CONT, "refuse", "an odd n_corners", host="odd", **t), case(CONT, "refuse", "a negative n_corners", host="negative", **t),
          case(CONT, "refuse", "n_corners whose sum leaves int32", host="huge", **t)]
    pairs = [("ws", "words", "count"), ("n_corners", "words", "count"), ("n_corners", "ws", "count"), ("head", "xy", "trace"), ("scratch", "xy", "trace"),
             ("scratch", "head", "trace")] + [(o, i, "trace") for o in ("xy", "head", "scratch") for i in ("words", "ws")]
    for o, i, ph in pairs:
        wide = dict(small, h=13, w=67, phase=ph)            # 14 words a mask: 16 bytes in is inside every buffer of the pair
        r += [case(CONT, "refuse", "{} == {} ({})".format(o, i, ph), overlap=(o, i, 0), **wide),
              case(CONT, "refuse", "{} 16 bytes into {} ({})".format(o, i, ph), overlap=(o, i, 1), **wide)]
    return r


def all_cases():
    rows = _prepare_rows() + _compose_rows() + _keypoint_rows() + _iou_rows() + _assign_rows() + _gather_rows() + _contour_rows()
    seen = {}
    for c in rows:
        geo = []
        for k, d in DEFAULTS[c["entry"]].items():
            v = c[k]
            if k in ("h", "w", "n", "rows", "cap", "r", "k", "s") or v != d:
                geo.append("{}{}".format(k, "/".join(str(x) for x in v) if isinstance(v, tuple) else v))
        for k in ("data", "null"):
            if c[k]:
                geo.append(("null-" if k == "null" else "") + c[k])
        name = " | ".join([WRAPPER if c["wrapper"] else c["entry"], c["feature"], " ".join(geo)])
        seen[name] = seen.get(name, 0) + 1
        c["id"] = name if seen[name] == 1 else "{} #{}".format(name, seen[name])
    return rows


def largest_buffer(c):
    """Bytes of the largest buffer of an accepted row (the caps of the CPU module)."""
    e = c["entry"]
    if e == PREP:
        return 4 * REC_INTS * max(c["n"], 1)
    if e == COMP:
        return max(3 * c["h"] * c["w"], 8 * max(c["n"], 1) * nwords(c["h"], c["w"]))
    if e == KP:
        return 4 * c["h"] * c["w"]
    if e == IOU:
        return 8 * max(c["rows"] * c["n"], 1)
    if e == ASSIGN:
        return max(8 * c["rows"] * c["n"], 16 * c["cap"])
    if e == GATHER:
        return 8 * c["cap"] * nwords(c["h"], c["w"])
    if e == CONT:
        t = corners_known(c)
        t = 2 * c["r"] * (c["h"] + 1) * (c["w"] + 1) if t is None else t           # at most two records a vertex
        return max(trace_ws_bytes(t), contour_ws_bytes(c["r"], c["h"], c["w"]), 8 * c["r"] * nwords(c["h"], c["w"]))
    raise KeyError(e)


# ---------------------------------------------------------------------------------------------------------------
# the C call of a row
# ---------------------------------------------------------------------------------------------------------------
def host_corners(c, totals=None):
    """The host n_corners of a trace call: the device's totals (None: 4 a mask, non-zero and even, so that a refusal behind T > 0 is
    reached) as the row's `host` changes them."""
    r = min(max(c["r"], 0), 70000)
    v = [4] * r if totals is None else [int(x) for x in totals]
    how = c["host"]
    if how == "odd":
        v[-1] += 1
    elif how == "negative":
        v[0] = -2
    elif how == "huge":
        v = [INT32_MAX - 1] * len(v)
    elif how == "smaller":
        v = [max(0, x - 2 * (1 + i % 3)) for i, x in enumerate(v)]
    elif how == "larger":
        v = [x + 2 * (1 + i % 3) for i, x in enumerate(v)]
    return v


def dummy_pointers(c, ptr):
    """Every device pointer of a row's call set to one 16-byte aligned address (no refusal follows a pointer's target); the trace's host
    n_corners is built by call(): non-zero and even, since an all-zero one returns CMK_OK before the checks behind T > 0."""
    return {k: ptr for k in POINTERS[c["entry"]] if k not in HOST_ARRAYS}


def call(lib, c, p, stream=None, totals=None):
    """The row's entry on the pointers p (name -> address); the pointer named by c["null"] and the operands a row does without go in as
    NULL, the row's byte offsets and overlaps are applied.  totals: the device's n_corners for the trace's host array.  Returns the
    return code (of the pair: the count's unless it is 0 and the phase goes on)."""
    e = c["entry"]
    p = dict(p)
    null = c["null"]
    if null and null not in HOST_ARRAYS:
        assert null in p, (c["id"], null)
        p[null] = None
    if c.get("overlap") and not isinstance(c["overlap"], int):
        o, i, k = c["overlap"]
        unit = {"boxes": 16, "classes": 8, "ids": 4, "ttl": 4, "areas": 4}.get(o.split("_")[-1])
        if e in (GATHER,) and o == "out_words":
            unit = 8 * nwords(c["h"], c["w"])
        if e == CONT:
            unit = 16
        if p[o] is not None and p[i] is not None:
            p[o] = p[i] + k * unit

    def at(name, off):
        return None if p[name] is None else p[name] + off

    if e == PREP:
        names, lens = (p["names"], p["name_lens"]) if c["num_names"] else (None, None)
        if c["wrapper"]:
            return lib.cmk_vis_prepare(p["boxes"], p["scores"], p["classes"], p["order"], names, lens, c["num_names"], p["palette"], c["n"], c["h"], c["w"],
                                       c["font_scale"], c["by_class"], p["records"], stream)
        return lib.cmk_vis_prepare_ids(p["boxes"], p["scores"], p["classes"], p["order"], names, lens, c["num_names"], p["palette"], c["n"], c["h"], c["w"],
                                       c["font_scale"], c["by_class"], p["color_ids"] if c["ids"] else None, p["records"], stream)
    if e == COMP:
        out = p["image_out"]                                             # in_off and out_off are in the pointers: the buffers start there
        if c["overlap"] and p["image_in"] is not None and out is not None:
            out = p["image_in"] + 3 * max(c["w"], 1) * max(c["overlap"], 0)
        return lib.cmk_vis_compose(p["image_in"], out, c["h"], c["w"], p["words"] if c["words"] else None, at("records", c["rec_off"]), c["n"],
                                   p["font"], c["line_width"], c["font_scale"], c["alpha256"], stream)
    if e == KP:
        return lib.cmk_vis_keypoints(p["image"], c["h"], c["w"], p["keypoints"], p["records"], c["n"], c["k"], p["skeleton"] if c["s"] else None, c["s"],
                                     c["thr"], c["line_width"], 0x0000FF, p["winner"], stream)
    if e == IOU:
        return lib.cmk_vis_track_iou_boxes(p["old_boxes"], c["rows"], p["new_boxes"], c["n"], p["iou"], stream)
    if e == ASSIGN:
        iou = p["iou"] if c["mode"] in ("box", "both") else None
        inter = p["inter"] if c["mode"] in ("mask", "both") else None
        oa, na = (p["old_areas"], p["new_areas"]) if c["mode"] in ("mask", "both") else (None, None)
        return lib.cmk_vis_track_assign(iou, inter, oa, na, c["rows"], p["old_boxes"], p["old_classes"], p["old_ids"], p["old_ttl"], p["new_boxes"],
                                        p["new_classes"], c["n"], c["cap"], c["ttl"], c["thr"], p["out_boxes"], p["out_classes"], p["out_ids"], p["out_ttl"],
                                        p["src"], p["track_ids"], p["counters"], stream)
    if e == GATHER:
        nwd, na = (p["new_words"], p["new_areas"]) if c["n"] else (None, None)
        return lib.cmk_vis_track_gather(p["src"], p["counters"], p["old_words"], p["old_areas"], nwd, na, c["n"], c["rows"], c["cap"], c["h"], c["w"],
                                        p["out_words"], p["out_areas"], stream)
    if e == CONT:
        ok = 0 <= c["r"] <= 65535 and c["h"] >= 1 and c["w"] >= 1 and c["h"] * c["w"] < 2 ** 31 - 1
        ws_bytes = (contour_ws_bytes(c["r"], c["h"], c["w"]) if ok else 1 << 20) - c["ws_short"]
        ws = at("ws", c["ws_off"])
        rc = 0
        if c["phase"] in ("both", "count"):
            rc = lib.cmk_vis_contour_count(p["words"], c["r"], c["h"], c["w"], ws, ws_bytes, p["n_corners"], stream)
        if rc == 0 and c["phase"] in ("both", "trace"):
            v = host_corners(c, totals)
            host = None if null == "host_corners" else (ctypes.c_int32 * max(len(v), 1))(*v)
            t = sum(x for x in v if x > 0)
            sc_bytes = (trace_ws_bytes(t) if t <= INT32_MAX else 1 << 20) - c["sc_short"]
            rc = lib.cmk_vis_contour_trace(p["words"], c["r"], c["h"], c["w"], ws, ws_bytes, host, at("scratch", c["sc_off"]), sc_bytes, p["xy"], p["head"], stream)
        return rc
    raise KeyError(e)
