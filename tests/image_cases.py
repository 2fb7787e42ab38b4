"""The conformance table of the kernels around the model (csrc/resize.hip, csrc/rle.hip, csrc/mask_iou.hip): the Pillow-exact resize front
end, the test-time augmentation maps, the COCO RLE encoder, the packed masks, their intersections and the Boundary IoU erosion.  One row
per case, in the shape of tests/tail_cases.py: the C entry point, the kernels it launches (their cmk:: names as `nm -C` prints them), the
geometry, the feature cell, the answer the library is declared to give (accept or refuse) and `expect`, the geometry the row exists for,
restated here from the launch code (geometry(): mb_geometry, the quads of resize_h, the work items of tta_reduce, ...) and asserted by the CPU module: a row that says
"two tiles across" fails there if the restated nxt is 1.  Plain data plus call().  No tests here: tests/test_cpu_image_conformance.py
checks the census, the cells, the restated geometry and every refusal on dummy pointers, tests/test_gpu_image_conformance.py launches every
row on real buffers against its reference.

A row is a dict (case() gives the defaults of its entry, DEFAULTS):
  entry, feature, answer "accept" | "refuse", kernels [names], why, data (how the GPU module fills the inputs), null (the pointer handed
  in as NULL), host_only (a refusal whose buffers no test allocates), expect {name: value of geometry(row)}, and the integer arguments of
  its entry under the names of DEFAULTS[entry].  *_off arguments are BYTE offsets added to a pointer."""
import ctypes
import math

ENTRIES = ["cmk_resize_h_u8", "cmk_resize_v_u8", "cmk_resize_v_preprocess", "cmk_resize_v_preprocess_hflip", "cmk_tta_boxes_to_image",
           "cmk_tta_boxes_to_aug", "cmk_tta_reduce_masks", "cmk_rle_count+cmk_rle_encode", "cmk_mask_pack_bits", "cmk_rle_decode_pack",
           "cmk_mask_intersections", "cmk_mask_boundary_bits", "cmk_mask_unpack_bits"]
RH, RV, RVP, RVF, TIMG, TAUG, TRED, RLE, PACK, DEC, INTER, BND, UNPACK = ENTRIES
FILES = ("resize.hip", "rle.hip", "mask_iou.hip")

FEATURES = [
    "census",        # one plain accepted case per kernel instantiation
    "unaligned",     # a buffer that starts at a byte offset the fast path does not accept
    "edge",          # the smallest geometries at which the index arithmetic or the algorithm branches
    "second_trip",   # a grid-stride loop or block walk takes a second iteration
    "padded_slots",  # counts of 0, partial, above K and below 0: slots past the clamped count get the declared filler or zeros
    "nonfinite",     # NaN and Inf: the answer is what the fp32 restatement gives
    "determinism",   # the same call again gives the same bits (the GPU module repeats EVERY accepted row; this cell is the plain one)
    "refuse",        # CMK_EINVAL with an error text, nothing launched
]

CMK_EINVAL = -1
CMK_BOUNDARY_MAX_D = 128
MEAN, STD = (103.53, 116.28, 123.675), (1.0, 57.0, 2.0)           # the tail table's PREP_MEAN / PREP_STD
TOO_BIG = 46341                                                   # 46341^2 = 2^31 + 4633 >= 2^31 - 1
MAX_BYTES = 40 << 20                                              # no buffer of an accepted row is larger (the two second_trip rows: 8 and 35 MB)


def mixed(a):
    """Flips of a augmentations, mixed: 1 0 1 0 0 1 0 1 1 1 0 0 1 0 1 1 0 1 ..."""
    return [(0x2D3A5 >> (i % 18)) & 1 for i in range(a)]


_V = dict(h=37, new_h=61, new_w=29, tables=1, ksize_delta=0)
_VP = dict(_V, hp=64, wp=48, reverse=0)
_M = dict(r=3, h=37, w=53)
DEFAULTS = {
    RH: dict(h=37, w=53, new_w=87, ksize_delta=0, dst_off=0),
    RV: dict(_V), RVP: dict(_VP), RVF: dict(_VP),          # tables 0: the skipped pass, no tables and ksize 0
    TIMG: dict(a=2, k=7, counts=[7, 4], flips=[0, 1], img_w=640, img_h=480, box_off=0, cand_off=0),
    TAUG: dict(a=2, k=7, count=5, flips=[0, 1], box_off=0, out_off=0),
    TRED: dict(a=2, k=3, s=28, count=2, flips=[0, 1], scores=1, masks_off=0, out_off=0),
    RLE: dict(r=13, h=97, w=131, off=0, ws_short=0, ws_off=0, phase="both"),      # phase: which of the two calls call() makes
    PACK: dict(_M, off=0), UNPACK: dict(_M, off=0),
    DEC: dict(m=5, h=37, w=53, bitmasks=1, off=0),
    INTER: dict(n=3, m=5, h=37, w=53),
    BND: dict(r=17, h=97, w=131, d=3, overlap=0),          # overlap: bwords = words + 8 * overlap bytes
}

N_A = {}
for _e in ENTRIES:
    if _e not in (TRED, RLE, PACK, UNPACK, DEC):
        N_A[(_e, "unaligned")] = ("the 64-bit words of a packed mask have no narrower path" if _e in (INTER, BND) else
                                  "byte loads and stores or a required alignment: there is no fast path that a byte offset would leave (a "
                                  "misaligned dst of cmk_resize_h_u8 and misaligned boxes of the TTA maps are refuse rows)")
    if _e not in (RH, TRED, RLE):
        N_A[(_e, "second_trip")] = "no grid-stride loop: the grid covers the work one to one (cmk_mask_intersections' walk over the ground-truth " \
                                   "tiles and the boundary kernel's loops inside a workgroup are edge rows)"
    if _e not in (TIMG, TAUG, TRED):
        N_A[(_e, "padded_slots")] = "the entry has no count argument read on the device"
    if _e not in (TIMG, TAUG, TRED):
        N_A[(_e, "nonfinite")] = "integer kernel: bytes, bits and int32 tables in, integers out" + \
                                 (" (mean3 / std3 are host arrays whose arithmetic is one subtraction and one division)" if _e in (RVP, RVF) else "")
del _e
NO_ROW = {"a 7-character count of the RLE string": "needs a run of 2^29 pixels, a 512 MB bitmap: the 1100 x 1000 row reaches 5 characters"}
PRECONDITIONS = {
    RLE: "mask bytes are 0 or 1: the walk compares whole bytes and reads bit 0 of the XOR, so another byte value has no row",
    PACK: "mask bytes are 0 or 1 (the kernel reads != 0; other values are outside the documented input and have no row)",
    DEC: "the last prefix sum of every mask is H*W and the prefix sums do not decrease: the caller checks it, the kernel does not",
    BND: "words hold zero in the unused high bits of the last word, as the two producers write them",
}

WALK = ["rle_count_kernel", "rle_scan_kernel", "rle_offsets_kernel", "rle_starts_kernel", "rle_string_kernel"]


def ksize_of(in_size, out_size):
    """cmk_resize_ksize restated: int(ceil(max(in / out, 1))) * 2 + 1."""
    return int(math.ceil(max(in_size / out_size, 1.0))) * 2 + 1


def rle_ws_bytes(r, h, w):
    """cmk_rle_ws_bytes restated: R + 1 int64 offsets, then an int32 per (mask, 64-row chunk, column)."""
    return 8 * (r + 1) + 4 * r * (-(-h // 64)) * w


def nwords(h, w):
    return (h * w + 63) // 64


def mb_geometry(h, w, d):
    """mb_geometry of csrc/mask_iou.hip restated: halo words q, tile TW words x TR rows, nxt x nyt tiles, the dynamic LDS of the launch."""
    q = (d + 63) // 64
    rw = -(-w // 64)
    for tw in (32, 16, 8):
        TW = min(rw, tw)
        fit = 8192 // (2 * TW + 2 * q) - 2 * d
        if fit >= min(h, 2 * d):
            break
    TR = min(min(fit, h), max(4 * d, 64))
    TR = -(-h // (-(-h // TR)))
    return dict(q=q, TW=TW, TR=TR, nxt=-(-rw // TW), nyt=-(-h // TR), lds=8 * (TR + 2 * d) * (2 * TW + 2 * q), step64=int(d >= 127), shrunk=int(TW < min(rw, 32)))


def tred_vec(c):
    return c["s"] % 4 == 0 and c["masks_off"] % 16 == 0 and c["out_off"] % 16 == 0


def geometry(c):
    """What the launch code makes of a row's arguments, restated: the names a row's `expect` may use."""
    e = c["entry"]
    if e == RH:
        total = 3 * c["new_w"] * c["h"]
        quads = (total + 3) // 4
        return dict(quads=quads, tail=total % 4, trips=-(-quads // (8192 * 256)), ksize=ksize_of(c["w"], c["new_w"]))
    if e in (RV, RVP, RVF):
        width = 3 * c["new_w"] if e == RV else c["wp"]
        return dict(blocks=-(-width // 256), last=width - 256 * (width // 256), ksize=ksize_of(c["h"], c["new_h"]) if c["tables"] else 0,
                    pad=int(e != RV and (c["hp"] > c["new_h"]) + (c["wp"] > c["new_w"])))
    if e in (TIMG, TAUG):
        return dict(blocks=-(-c["k"] // 256))
    if e == TRED:
        v = 4 if tred_vec(c) else 1
        items = c["k"] * c["s"] * (c["s"] // v) + (c["k"] if c["scores"] else 0)
        return dict(v=v, items=items, trips=-(-items // (4096 * 256)))
    hw = c["h"] * c["w"]
    if e == RLE:
        aligned = c["w"] % 4 == 0 and c["off"] % 4 == 0
        return dict(chunks=-(-c["h"] // 64), tiles=-(-c["w"] // 256), scan_trips=-(-c["w"] // 1024), offset_trips=-(-max(c["r"], 1) // 1024),
                    aligned=int(aligned))
    if e in (PACK, UNPACK, DEC):
        return dict(words=nwords(c["h"], c["w"]), waves=-(-nwords(c["h"], c["w"]) // 8), ragged=hw % 64)
    if e == INTER:
        nw = nwords(c["h"], c["w"])
        return dict(words=nw, wblocks=-(-nw // 512), nblocks=-(-c["n"] // 16), gt_tiles=-(-c["m"] // 16))
    if e == BND:
        fits = 2 * c["d"] + 1 <= min(c["h"], c["w"])
        g = mb_geometry(c["h"], c["w"], c["d"]) if fits and 1 <= c["d"] <= CMK_BOUNDARY_MAX_D else {}
        return dict(g, fits=int(fits), words_per_row=c["w"] / 64.0)
    raise KeyError(e)


def kernels_of(c):
    """The kernels an accepted row launches."""
    e = c["entry"]
    if e == RH:
        return ["resize_h_kernel"]
    if e == RV:
        return ["resize_v_u8_kernel"]
    if e == RVP:
        return ["resize_v_preprocess_kernel"]
    if e == RVF:
        return ["resize_v_preprocess_hflip_kernel"]
    if e == TIMG:
        return ["tta_boxes_to_image_kernel"]
    if e == TAUG:
        return ["tta_boxes_to_aug_kernel"]
    if e == TRED:
        return ["tta_reduce_masks_kernel<4>" if tred_vec(c) else "tta_reduce_masks_kernel<1>"]
    if e == RLE:
        return WALK if c["r"] else []
    if e == PACK:
        return ["mask_pack_kernel", "words_area_kernel"] if c["r"] else []
    if e == DEC:
        return ["rle_decode_pack_kernel", "words_area_kernel"] if c["m"] else []
    if e == INTER:
        return ["mask_inter_kernel"] if c["n"] and c["m"] else []
    if e == BND:
        if not c["r"]:
            return []
        return ["mask_boundary_kernel"] if 2 * c["d"] + 1 <= min(c["h"], c["w"]) else ["words_area_kernel"]
    if e == UNPACK:
        return ["mask_unpack_kernel"] if c["r"] else []
    raise KeyError(e)


def case(entry, feature, why="", data="", null=None, host_only=False, expect=None, **kw):
    c = dict(DEFAULTS[entry])
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    c.update(id="", entry=entry, feature=feature, answer="refuse" if feature == "refuse" else "accept", why=why, data=data, null=null,
             host_only=host_only, expect=dict(expect or {}), kernels=[])
    if c["answer"] == "accept":
        c["kernels"] = kernels_of(c)
    return c


# the pointers of each entry (the names call() takes) in the order of the C signature(s)
POINTERS = {RH: ("src", "bounds", "kk", "dst"), RV: ("src", "bounds", "kk", "dst"), RVP: ("src", "bounds", "kk", "dst", "mean", "std"),
            RVF: ("src", "bounds", "kk", "dst", "mean", "std"),
            TIMG: ("det_box", "det_score", "det_cls", "det_loc", "det_counts", "table", "cand_box", "cand_score", "cand_cls", "cand_loc", "cand_count"),
            TAUG: ("box", "count", "table", "out_box", "out_counts"),
            TRED: ("masks", "flips", "mask_scores", "count", "out_masks", "out_scores"),
            RLE: ("masks", "ws", "n_runs", "starts", "counts", "bytes", "lens"),
            PACK: ("masks", "words", "areas"), DEC: ("cum", "off", "words", "areas", "bitmasks"), INTER: ("det", "gt", "inter"),
            BND: ("words", "bwords", "bareas"), UNPACK: ("words", "masks")}
HOST_ARRAYS = ("mean", "std")                        # built by call() on the host: a row can only NULL them
NULLABLE = {e: tuple(p for p in POINTERS[e]) for e in ENTRIES}
NULLABLE[DEC] = ("cum", "off", "words", "areas")                       # bitmasks is optional: an accepted row
NULLABLE[TRED] = ("masks", "flips", "count", "out_masks", "mask_scores", "out_scores")      # one of the score pair alone is refused
COUNT_PHASE = ("masks", "ws", "n_runs")                                # the pointers cmk_rle_count takes


def _nulls(entry, **kw):
    rows = []
    for p in NULLABLE[entry]:
        if entry == RLE:
            rows += [case(entry, "refuse", "null {} ({})".format(p, ph), null=p, **dict(kw, phase=ph)) for ph in ("count", "encode") if ph == "encode" or p in COUNT_PHASE]
        else:
            rows.append(case(entry, "refuse", "null " + p, null=p, **kw))
    return rows


def _resize_rows():
    r = [case(RH, "census", "37 x 53 -> 87 wide: ksize 3, 3 * 87 * 37 = 9657 bytes, one left over after the quads", expect=dict(ksize=3, tail=1, trips=1)),
         case(RH, "edge", "h = 4: the bytes are a whole number of quads, no tail store", h=4, expect=dict(tail=0)),
         case(RH, "edge", "230 -> 31: ksize 17", h=5, w=230, new_w=31, expect=dict(ksize=17)),
         case(RH, "edge", "w = 1: every output pixel is the one input pixel", h=5, w=1, new_w=3),
         case(RH, "edge", "new_w = 1", h=5, w=9, new_w=1, expect=dict(ksize=19)),
         case(RH, "edge", "h = 1", h=1, w=9, new_w=14),
         case(RH, "edge", "a quad straddles rows and pixels: new_w = 1, three bytes per row", h=7, w=2, new_w=1, expect=dict(tail=1)),
         case(RH, "edge", "damaged tables: lo < 0, lo > w, n < 0, n > ksize, lo + n > w, clamped as resize_bounds says; the source's guards "
              "hold another byte on the second call", data="damaged", h=6, w=40, new_w=23),
         case(RH, "second_trip", "1400 x 1000 -> 2001 wide: 2,101,050 quads > 8192 x 256 threads", h=1400, w=1000, new_w=2001,
              expect=dict(quads=2101050, trips=2)),
         case(RH, "determinism", "one thread owns each quad")]
    r += _nulls(RH)
    r += [case(RH, "refuse", "h = 0", h=0), case(RH, "refuse", "w = 0", w=0), case(RH, "refuse", "new_w = 0", new_w=0),
          case(RH, "refuse", "a ksize that does not belong to the sizes", ksize_delta=2),
          case(RH, "refuse", "dst not 4-byte aligned", dst_off=2)]
    for e in (RV, RVP, RVF):
        pre = e != RV
        big = dict(hp=80, wp=257) if pre else {}
        r += [case(e, "census", "37 -> 61 rows of 29 pixels" + (", padding on both sides" if pre else ""), expect=dict(ksize=3, **(dict(pad=2) if pre else {}))),
              case(e, "edge", "230 -> 31 rows: ksize 17", h=230, new_h=31, new_w=5, **(dict(hp=31, wp=5) if pre else {}), expect=dict(ksize=17)),
              case(e, "edge", "the skipped pass: no tables, ksize 0, a copy", new_h=37, tables=0, expect=dict(ksize=0)),
              case(e, "edge", "h = 1", h=1, new_h=3, **(dict(hp=3) if pre else {})),
              case(e, "edge", "new_h = 1", h=9, new_h=1, **(dict(hp=1) if pre else {})),
              case(e, "edge", "new_w = 1", new_w=1, **(dict(wp=1) if pre else {})),
              case(e, "edge", "damaged tables: lo < 0, lo > h, n < 0, n > ksize, lo + n > h, clamped as resize_bounds says; the source's guards "
                   "hold another byte on the second call", data="damaged", h=12, new_h=19, new_w=7, **(dict(hp=19, wp=8) if pre else {})),
              case(e, "determinism", "one thread owns each output")]
        if pre:
            r += [case(e, "edge", "W = 257: a second block of one thread; padding on both sides", new_w=200, **big, expect=dict(blocks=2, last=1, pad=2)),
                  case(e, "edge", "W = 257 = new_w, H = new_h: no padding", new_w=257, hp=61, wp=257, expect=dict(blocks=2, last=1, pad=0)),
                  case(e, "edge", "W = 257 with reverse_channels", new_w=200, reverse=1, **big, expect=dict(blocks=2, last=1))]
        else:
            r.append(case(e, "edge", "3 * new_w = 261: a second block of five threads", new_w=87, expect=dict(blocks=2, last=5)))
        r += _nulls(e)
        r += [case(e, "refuse", "h = 0", h=0), case(e, "refuse", "new_h = 0", new_h=0), case(e, "refuse", "new_w = 0", new_w=0),
              case(e, "refuse", "a ksize that does not belong to the sizes", ksize_delta=2),
              case(e, "refuse", "no tables although new_h != h", tables=0),
              case(e, "refuse", "the skipped pass with a ksize", new_h=37, tables=0, ksize_delta=3)]
        if pre:
            r += [case(e, "refuse", "H < new_h", hp=60), case(e, "refuse", "W < new_w", wp=28),
                  case(e, "refuse", "H above 65535: gridDim.y", host_only=True, hp=65536)]
        else:
            r.append(case(e, "refuse", "new_h above 65535: gridDim.y", host_only=True, new_h=65536))
    return r


def _tta_rows():
    r = [case(TIMG, "census", "two augmentations, the second flipped, counts 7 and 4"),
         case(TIMG, "edge", "A = 1, K = 1", a=1, k=1, counts=[1], flips=[1]),
         case(TIMG, "edge", "boxes that clip at both image edges, flipped and not", data="clip", a=4, k=9, counts=[9, 9, 9, 9], flips=[0, 1, 1, 0]),
         case(TIMG, "edge", "K = 257: a second block of one thread", a=2, k=257, counts=[257, 256], expect=dict(blocks=2)),
         case(TIMG, "padded_slots", "A = 4, K = 300: counts 0, full, partial and above K (clamped); the slots past the compacted total stay filler",
              a=4, k=300, counts=[0, 300, 17, 500], flips=[0, 1, 0, 1], expect=dict(blocks=2)),
         case(TIMG, "padded_slots", "a count of -3 is clamped to 0", a=4, k=300, counts=[-3, 5, 300, 0], flips=[1, 0, 1, 0]),
         case(TIMG, "padded_slots", "no detection at all: cand_count 0, nothing else written", a=3, k=5, counts=[0, 0, -1], flips=[0, 1, 0]),
         case(TIMG, "nonfinite", "NaN and Inf box coordinates clip as fminf / fmaxf do (np.fmin / np.fmax); a NaN location and score stay", data="nonfinite",
              a=2, k=9, counts=[9, 9]),
         case(TIMG, "determinism", "every thread owns its slot: the offsets are sums of the counts")]
    small = dict(a=2, k=5, counts=[5, 3])
    r += _nulls(TIMG, **small)
    r += [case(TIMG, "refuse", "A = 0", **dict(small, a=0)), case(TIMG, "refuse", "A = 4097", **dict(small, a=4097)),
          case(TIMG, "refuse", "K = 0", **dict(small, k=0)), case(TIMG, "refuse", "K = 65536", **dict(small, k=65536)),
          case(TIMG, "refuse", "img_w = 0", img_w=0, **small), case(TIMG, "refuse", "img_w = 65536", img_w=65536, **small),
          case(TIMG, "refuse", "img_h = 0", img_h=0, **small), case(TIMG, "refuse", "img_h = 65536", img_h=65536, **small),
          case(TIMG, "refuse", "det_box not 16-byte aligned", box_off=4, **small), case(TIMG, "refuse", "cand_box not 16-byte aligned", cand_off=8, **small)]

    r += [case(TAUG, "census", "two augmentations, the second flipped, 5 of 7 rows"),
          case(TAUG, "edge", "A = 1, K = 1", a=1, k=1, count=1, flips=[1]),
          case(TAUG, "edge", "K = 257, all rows valid: a second block of one thread", a=3, k=257, count=257, flips=[1, 0, 1], expect=dict(blocks=2)),
          case(TAUG, "padded_slots", "K = 257, count 0: zeros everywhere, out_counts 0", a=3, k=257, count=0, flips=[1, 0, 1]),
          case(TAUG, "padded_slots", "K = 257, count 100: zero rows from 100 on (their boxes are NaN)", a=3, k=257, count=100, flips=[1, 0, 1]),
          case(TAUG, "padded_slots", "K = 257, count 999 > K is clamped to K", a=3, k=257, count=999, flips=[1, 0, 1]),
          case(TAUG, "padded_slots", "K = 257, count -4 < 0 is clamped to 0", a=3, k=257, count=-4, flips=[1, 0, 1]),
          case(TAUG, "nonfinite", "NaN and Inf coordinates go through the multiplication and the flip as IEEE says", data="nonfinite", k=9, count=9),
          case(TAUG, "determinism", "one thread owns each row")]
    small = dict(a=2, k=5, count=3)
    r += _nulls(TAUG, **small)
    r += [case(TAUG, "refuse", "A = 0", **dict(small, a=0)), case(TAUG, "refuse", "A = 4097", **dict(small, a=4097)),
          case(TAUG, "refuse", "K = 0", **dict(small, k=0)), case(TAUG, "refuse", "K = 65536", **dict(small, k=65536)),
          case(TAUG, "refuse", "box not 16-byte aligned", box_off=4, **small), case(TAUG, "refuse", "out_box not 16-byte aligned", out_off=4, **small)]

    r += [case(TRED, "census", "S = 28, rows of seven float4: the vector kernel", expect=dict(v=4)),
          case(TRED, "census", "S = 3: the scalar kernel", s=3, expect=dict(v=1))]
    for s in (1, 3, 4, 12, 28):
        for a in (1, 2, 18):
            r.append(case(TRED, "edge", "S {} A {}, mixed flips".format(s, a), s=s, a=a, flips=mixed(a), expect=dict(v=4 if s % 4 == 0 else 1)))
    r += [case(TRED, "edge", "without mask_scores / out_scores", scores=0, a=3, flips=[1, 0, 1]),
          case(TRED, "edge", "K = 1, count 1", k=1, count=1),
          case(TRED, "unaligned", "S = 28 with masks 4 bytes off a 16-byte boundary: the scalar kernel, bit-equal to the aligned launch on the same data",
               masks_off=4, expect=dict(v=1)),
          case(TRED, "unaligned", "S = 28 with out_masks 4 bytes off: the scalar kernel, the same bits again", out_off=4, expect=dict(v=1)),
          case(TRED, "second_trip", "K 100, S 208, A 2: 1,081,600 mask work items + 100 scores > 4096 x 256 threads", k=100, s=208, count=97, flips=[1, 0],
               expect=dict(v=4, items=1081700, trips=2)),
          case(TRED, "second_trip", "the scalar kernel's second trip: K 8, S 387", k=8, s=387, count=7, flips=[0, 1], expect=dict(v=1, trips=2)),
          case(TRED, "padded_slots", "count 0: zeros", count=0), case(TRED, "padded_slots", "count above K is clamped", count=9),
          case(TRED, "padded_slots", "count below 0 is clamped", count=-2), case(TRED, "padded_slots", "count 2 of 3, S = 3: rows past the count are zeros, their masks NaN", s=3),
          case(TRED, "nonfinite", "a NaN and an Inf mask value stay in their own pixel, mirrored under flip; a NaN score stays in its row", data="nonfinite", count=3),
          case(TRED, "nonfinite", "... in the scalar kernel", data="nonfinite", s=3, count=3),
          case(TRED, "determinism", "a fixed order of additions, no atomics")]
    small = dict(s=4)
    r += _nulls(TRED, **small)
    r += [case(TRED, "refuse", "A = 0", a=0, **small), case(TRED, "refuse", "A = 4097", a=4097, **small), case(TRED, "refuse", "K = 0", k=0, **small),
          case(TRED, "refuse", "K = 65536", k=65536, **small), case(TRED, "refuse", "S = 0", s=0), case(TRED, "refuse", "S = 1025", s=1025, host_only=True)]
    return r


def _rle_rows():
    r = [case(RLE, "census", "97 x 131, the pattern set: odd W, every row at another alignment (the funnel), a second chunk", expect=dict(chunks=2, aligned=0)),
         case(RLE, "edge", "1 x 1", h=1, w=1), case(RLE, "edge", "64 x 64: one chunk, aligned rows", h=64, w=64, expect=dict(chunks=1, aligned=1)),
         case(RLE, "edge", "65 x 4: aligned, a second chunk of one row", h=65, w=4, expect=dict(chunks=2, aligned=1)),
         case(RLE, "edge", "65 x 5: the funnel, a second chunk of one row", h=65, w=5, expect=dict(chunks=2, aligned=0)),
         case(RLE, "edge", "W = 256: exactly one tile of columns", h=3, w=256, expect=dict(tiles=1, aligned=1)),
         case(RLE, "edge", "W = 257: a second tile of one column", h=3, w=257, expect=dict(tiles=2, aligned=0)),
         case(RLE, "edge", "W = 1024: exactly one trip of the column scan", h=3, w=1024, expect=dict(tiles=4, scan_trips=1)),
         case(RLE, "second_trip", "W = 1025: the column scan's second trip holds one column", h=3, w=1025, expect=dict(tiles=5, scan_trips=2)),
         case(RLE, "second_trip", "R = 1025 masks of 3 x 5: the offset scan's second trip holds one mask", data="random", r=1025, h=3, w=5, expect=dict(offset_trips=2)),
         case(RLE, "second_trip", "33 x 65 with the checkerboard's 2145 and the 2146 single-pixel runs: the string kernel walks its runs three times", h=33, w=65),
         case(RLE, "edge", "1100 x 1000 long runs: counts of up to five characters and negative differences", data="long", r=2, h=1100, w=1000,
              expect=dict(chunks=18, tiles=4, aligned=1)),
         case(RLE, "edge", "R = 0 returns OK and touches nothing", r=0, h=5, w=3),
         case(RLE, "determinism", "scans in a fixed order, no atomics", h=33, w=65)]
    for off in (1, 2, 3):
        r.append(case(RLE, "unaligned", "the batch starts {} bytes off a dword: W % 4 == 0 and still not aligned, bytes on the first and last waves".format(off),
                      h=66, w=8, off=off, expect=dict(aligned=0)))
    r.append(case(RLE, "unaligned", "97 x 131 from byte 1", off=1, expect=dict(aligned=0)))
    small = dict(r=2, h=5, w=3, data="random")
    r += _nulls(RLE, **small)
    for ph in ("count", "encode"):
        s = dict(small, phase=ph)
        r += [case(RLE, "refuse", "H = 0 ({})".format(ph), **dict(s, h=0)), case(RLE, "refuse", "W = 0 ({})".format(ph), **dict(s, w=0)),
              case(RLE, "refuse", "R = -1 ({})".format(ph), **dict(s, r=-1)), case(RLE, "refuse", "R = 65536 ({})".format(ph), **dict(s, r=65536)),
              case(RLE, "refuse", "H*W >= 2^31 - 1 ({})".format(ph), host_only=True, **dict(s, h=TOO_BIG, w=TOO_BIG)),
              case(RLE, "refuse", "a workspace one byte short ({})".format(ph), ws_short=1, **s),
              case(RLE, "refuse", "a workspace that is not 8-byte aligned ({})".format(ph), ws_off=4, **s)]
    return r


HW_SHAPES = [(1, 1), (8, 8), (5, 13), (16, 32), (27, 19), (32, 64), (3, 683)]            # H*W = 1, 64, 65, 512, 513, 2048, 2049


def _mask_rows():
    r = []
    for e in (PACK, UNPACK, DEC):
        n = "m" if e == DEC else "r"
        r.append(case(e, "census", "37 x 53 = 1961 pixels: 31 words, the last ragged", expect=dict(words=31, ragged=41)))
        for h, w in HW_SHAPES:
            hw = h * w
            r.append(case(e, "edge", "H*W = {}: {}".format(hw, "whole words" if hw % 64 == 0 else "a last word of {} bit{}".format(hw % 64, "s" if hw % 64 > 1 else "")) +
                          (", whole waves of 8 words" if hw % 512 == 0 else ""), h=h, w=w, expect=dict(words=-(-hw // 64), ragged=hw % 64)))
        r.append(case(e, "edge", "no mask returns OK and touches nothing", **{n: 0}))
        r.append(case(e, "unaligned", "the byte " + ("bitmasks" if e == DEC else "masks") + " start at an odd offset", off=3, h=27, w=19))
        r.append(case(e, "determinism", "ballots, no atomics"))
        small = dict(h=5, w=13)
        r += _nulls(e, **small)
        r += [case(e, "refuse", "H = 0", **dict(small, h=0)), case(e, "refuse", "W = 0", **dict(small, w=0)), case(e, "refuse", "a count of -1", **dict(small, **{n: -1})),
              case(e, "refuse", "a count of 65536", **dict(small, **{n: 65536})),
              case(e, "refuse", "H*W >= 2^31 - 1", host_only=True, h=TOO_BIG, w=TOO_BIG)]
    r += [case(DEC, "edge", "5 x 13, the runs [3, 0, 2, 0, 0, 5, 55]: zero-length runs in the middle are passed over", data="middle", m=3, h=5, w=13),
          case(DEC, "edge", "without bitmasks", bitmasks=0, h=27, w=19)]

    for n, m in ((1, 1), (16, 16), (17, 17), (3, 33)):
        for h, w in ((8, 8), (128, 256), (113, 290)):
            nw = nwords(h, w)
            r.append(case(INTER, "census" if (n, m, nw) == (17, 17, 513) else "edge", "N {} M {}, {} words".format(n, m, nw), n=n, m=m, h=h, w=w,
                          expect=dict(words=nw, wblocks=-(-nw // 512), nblocks=-(-n // 16), gt_tiles=-(-m // 16))))
    r += [case(INTER, "edge", "N = 0 returns OK and touches nothing", n=0), case(INTER, "edge", "M = 0 returns OK and touches nothing", m=0),
          case(INTER, "determinism", "integer atomics: three workgroups add into every cell", n=17, m=33, h=130, w=520, expect=dict(wblocks=3, nblocks=2, gt_tiles=3))]
    small = dict(h=5, w=13)
    r += _nulls(INTER, **small)
    r += [case(INTER, "refuse", "H = 0", **dict(small, h=0)), case(INTER, "refuse", "W = 0", **dict(small, w=0)), case(INTER, "refuse", "N = -1", n=-1, **small),
          case(INTER, "refuse", "M = 65536", m=65536, **small), case(INTER, "refuse", "H*W >= 2^31 - 1", host_only=True, h=TOO_BIG, w=TOO_BIG)]
    return r


def _boundary_rows():
    hi = dict(data="solid", r=4)
    r = [case(BND, "census", "97 x 131 at d = 3, the pattern set: two tiles down", expect=dict(fits=1, q=1, nxt=1, nyt=2)),
         case(BND, "edge", "d = 1 on 40 x 20: several rows in a word", h=40, w=20, d=1, expect=dict(fits=1, q=1)),
         case(BND, "edge", "128 x 128 at d = 5: every row starts on a word, no shift on the way in or out", h=128, w=128, d=5, data="solid", r=4,
              expect=dict(fits=1, words_per_row=2.0)),
         case(BND, "edge", "2d + 1 == min(H, W): one square just fits", h=21, w=30, d=10, expect=dict(fits=1), data="solid", r=4),
         case(BND, "edge", "2d + 1 == min(H, W) + 1: no square fits, the boundary is the mask (a copy and the areas)", h=20, w=30, d=10, expect=dict(fits=0)),
         case(BND, "edge", "d = 200 where no square fits: any d >= 1 is accepted", h=40, w=20, d=200, expect=dict(fits=0)),
         case(BND, "edge", "131 x 131 at d = 64: the last d with one halo word", h=131, w=131, d=64, expect=dict(q=1, fits=1), **hi),
         case(BND, "edge", "131 x 131 at d = 65: two halo words", h=131, w=131, d=65, expect=dict(q=2, fits=1), **hi),
         case(BND, "edge", "257 x 259 at d = 127: the doubling's 64-pixel step", h=257, w=259, d=127, expect=dict(q=2, step64=1, fits=1, TW=5, nxt=1), **hi),
         case(BND, "edge", "257 x 259 at d = 128 (CMK_BOUNDARY_MAX_D): nearly all of the LDS", h=257, w=259, d=128,
              expect=dict(q=2, step64=1, fits=1, TW=5, TR=257, lds=57456), **hi),
         case(BND, "edge", "512 x 330 at d = 128: the launch asks for exactly 64 KiB of LDS, two tiles down", h=512, w=330, d=128,
              expect=dict(q=2, TW=6, TR=256, nyt=2, nxt=1, lds=65536), data="solid", r=3),
         case(BND, "edge", "259 x 600 at d = 100: the tile width shrunk to 8 words, two tiles across a row", h=259, w=600, d=100,
              expect=dict(q=2, TW=8, shrunk=1, nxt=2, TR=130, nyt=2), data="solid", r=3),
         case(BND, "edge", "262 x 2100 at d = 40: three tiles across a row, 32.8 words per row", h=262, w=2100, d=40,
              expect=dict(q=1, TW=16, shrunk=1, nxt=3, TR=131, nyt=2), data="solid", r=3),
         case(BND, "edge", "R = 0 returns OK and touches nothing", r=0),
         case(BND, "determinism", "64-bit OR and integer add atomics: neighbouring tiles write the same words", h=90, w=2100, d=20, data="solid", r=4,
              expect=dict(TW=32, nxt=2, nyt=2, fits=1))]
    small = dict(r=2, h=21, w=30, d=2, data="solid")
    r += _nulls(BND, **small)
    r += [case(BND, "refuse", "d = 0", **dict(small, d=0)), case(BND, "refuse", "d = -5", **dict(small, d=-5)),
          case(BND, "refuse", "d = 129 where a square fits", **dict(small, h=259, w=300, d=129)),
          case(BND, "refuse", "bwords one word into words", overlap=1, **small), case(BND, "refuse", "bwords == words", overlap=-1, **small),
          case(BND, "refuse", "H = 0", **dict(small, h=0)), case(BND, "refuse", "W = 0", **dict(small, w=0)), case(BND, "refuse", "R = -1", **dict(small, r=-1)),
          case(BND, "refuse", "R = 65536", **dict(small, r=65536)), case(BND, "refuse", "H*W >= 2^31 - 1", host_only=True, **dict(small, h=TOO_BIG, w=TOO_BIG))]
    return r


def all_cases():
    rows = _resize_rows() + _tta_rows() + _rle_rows() + _mask_rows() + _boundary_rows()
    seen = {}
    for c in rows:
        geo = []
        for k, d in DEFAULTS[c["entry"]].items():
            v = c[k]
            if isinstance(v, list):
                geo.append(k + "/".join(str(x) for x in v) if len(v) <= 6 else "{}x{}".format(k, len(v)))
            elif k in ("h", "w", "new_h", "new_w", "a", "k", "s", "r", "m", "n", "d") or v != d:
                geo.append("{}{}".format(k, v))
        for k in ("data", "null"):
            if c[k]:
                geo.append(("null-" if k == "null" else "") + c[k])
        name = " | ".join([c["entry"], c["feature"], " ".join(geo)])
        seen[name] = seen.get(name, 0) + 1
        c["id"] = name if seen[name] == 1 else "{} #{}".format(name, seen[name])
    return rows


def largest_buffer(c):
    """Bytes of the largest buffer of an accepted row (the cap of the CPU module)."""
    e = c["entry"]
    if e == RH:
        return 3 * c["h"] * max(c["w"], c["new_w"])
    if e in (RV, RVP, RVF):
        return max(3 * c["new_w"] * max(c["h"], c["new_h"]), 12 * c.get("hp", 0) * c.get("wp", 0))
    if e in (TIMG, TAUG):
        return 16 * c["a"] * c["k"]
    if e == TRED:
        return 4 * c["a"] * c["k"] * c["s"] * c["s"]
    if e == RLE:
        return max(1, c["r"]) * c["h"] * c["w"] * 8 + rle_ws_bytes(max(c["r"], 0), c["h"], c["w"])      # 7 bytes per run, at most a run per pixel
    if e == INTER:
        return 8 * max(c["n"], c["m"]) * nwords(c["h"], c["w"])
    return max(1, c.get("r", c.get("m", 1))) * c["h"] * c["w"] * 4


# ---------------------------------------------------------------------------------------------------------------
# the C call of a row
# ---------------------------------------------------------------------------------------------------------------
def dummy_pointers(c, ptr):
    """Every pointer of a row's call set to one 16-byte aligned address (no refusal follows a pointer's target)."""
    return {k: ptr for k in POINTERS[c["entry"]] if k not in HOST_ARRAYS}


def call(lib, c, p, stream=None):
    """The row's entry on the pointers p (name -> address); the pointer named by c["null"] and the operands a row does without go in as
    NULL, the row's byte offsets are added.  Returns the return code (of the pair: cmk_rle_count's unless it is 0 and the phase goes on)."""
    e = c["entry"]
    p = dict(p)
    null = c["null"]
    if null and null not in HOST_ARRAYS:
        assert null in p, (c["id"], null)
        p[null] = None

    def at(name, off):
        return None if p[name] is None else p[name] + off

    def arr(values, name):
        return None if null == name else (ctypes.c_float * 3)(*values)

    if e in (RH, RV, RVP, RVF):
        if e == RH:
            ks = ksize_of(max(1, c["w"]), max(1, c["new_w"])) + c["ksize_delta"]
            return lib.cmk_resize_h_u8(p["src"], c["h"], c["w"], c["new_w"], p["bounds"], p["kk"], ks, at("dst", c["dst_off"]), stream)
        ks = (ksize_of(max(1, c["h"]), max(1, c["new_h"])) if c["tables"] else 0) + c["ksize_delta"]
        bounds, kk = (p["bounds"], p["kk"]) if c["tables"] else (None, None)
        if e == RV:
            return lib.cmk_resize_v_u8(p["src"], c["h"], c["new_h"], c["new_w"], bounds, kk, ks, p["dst"], stream)
        fn = lib.cmk_resize_v_preprocess if e == RVP else lib.cmk_resize_v_preprocess_hflip
        return fn(p["src"], c["h"], c["new_h"], c["new_w"], bounds, kk, ks, p["dst"], c["hp"], c["wp"], arr(MEAN, "mean"), arr(STD, "std"), c["reverse"], stream)
    if e == TIMG:
        return lib.cmk_tta_boxes_to_image(at("det_box", c["box_off"]), p["det_score"], p["det_cls"], p["det_loc"], p["det_counts"], p["table"], c["a"], c["k"],
                                          c["img_w"], c["img_h"], at("cand_box", c["cand_off"]), p["cand_score"], p["cand_cls"], p["cand_loc"], p["cand_count"], stream)
    if e == TAUG:
        return lib.cmk_tta_boxes_to_aug(at("box", c["box_off"]), p["count"], p["table"], c["a"], c["k"], at("out_box", c["out_off"]), p["out_counts"], stream)
    if e == TRED:
        ms, os_ = (p["mask_scores"], p["out_scores"]) if c["scores"] else (None, None)
        return lib.cmk_tta_reduce_masks(p["masks"], p["flips"], ms, p["count"], c["a"], c["k"], c["s"], p["out_masks"], os_, stream)      # (the offsets are in the pointers)
    if e == RLE:
        ok = c["r"] >= 0 and c["h"] >= 1 and c["w"] >= 1 and c["h"] * c["w"] < 2 ** 31 - 1
        ws_bytes = (rle_ws_bytes(c["r"], c["h"], c["w"]) if ok else 1 << 20) - c["ws_short"]
        ws = at("ws", c["ws_off"])
        rc = 0
        if c["phase"] in ("both", "count"):
            rc = lib.cmk_rle_count(p["masks"], c["r"], c["h"], c["w"], ws, ws_bytes, p["n_runs"], stream)
        if rc == 0 and c["phase"] in ("both", "encode"):
            rc = lib.cmk_rle_encode(p["masks"], c["r"], c["h"], c["w"], ws, ws_bytes, p["n_runs"], p["starts"], p["counts"], p["bytes"], p["lens"], stream)
        return rc
    if e == PACK:
        return lib.cmk_mask_pack_bits(p["masks"], c["r"], c["h"], c["w"], p["words"], p["areas"], stream)
    if e == DEC:
        return lib.cmk_rle_decode_pack(p["cum"], p["off"], c["m"], c["h"], c["w"], p["words"], p["areas"], p["bitmasks"] if c["bitmasks"] else None, stream)
    if e == INTER:
        return lib.cmk_mask_intersections(p["det"], c["n"], p["gt"], c["m"], c["h"], c["w"], p["inter"], stream)
    if e == BND:
        bw = p["bwords"]
        if c["overlap"] and p["words"] is not None and bw is not None:
            bw = p["words"] + 8 * max(c["overlap"], 0)
        return lib.cmk_mask_boundary_bits(p["words"], c["r"], c["h"], c["w"], c["d"], bw, p["bareas"], stream)
    if e == UNPACK:
        return lib.cmk_mask_unpack_bits(p["words"], c["r"], c["h"], c["w"], p["masks"], stream)
    raise KeyError(e)
