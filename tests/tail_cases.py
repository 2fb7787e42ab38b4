"""The conformance table of the kernels that run after the FCOS head and around the model (csrc/detect.hip, csrc/roi.hip, csrc/prepost.hip,
csrc/keypoint.hip): candidate selection, sort + NMS + top-k, RoIAlign, SAG-Mask attention, the class-selected mask predictor, the MaskIoU
input pooling and score, the mask paste, the all-gather records, the image preprocessing and the keypoint decode.  One row per case: the C
entry point, the kernels it launches (their cmk:: names as `nm -C` prints them), the geometry, the feature cell and the answer the library
is declared to give, accept or refuse.  Plain data plus call(), which turns a row and a dict of pointers into the C call.  No tests here:
tests/test_cpu_tail_conformance.py checks the census, the cells and every refusal on dummy pointers, tests/test_gpu_tail_conformance.py
launches every row on real buffers against its reference.

A row is a dict (case() below gives the defaults of its entry point, DEFAULTS):
  entry, feature, answer "accept" | "refuse", kernels [names], why (what the row is there for), data (how the GPU module fills the inputs),
  null (the pointer handed in as NULL), host_only (a refusal whose buffers no test allocates: the row runs on dummy pointers only),
  and the integer arguments of its entry point under the names of DEFAULTS[entry]; counts are the per-image valid slots."""
import ctypes

ENTRIES = ["cmk_fcos_select", "cmk_nms_topk", "cmk_roi_align_pool", "cmk_spatial_attention", "cmk_mask_predict", "cmk_mask_pool_concat",
           "cmk_mask_iou_score", "cmk_paste_masks", "cmk_pack_records", "cmk_pack_records_kp", "cmk_preprocess_chw", "cmk_keypoint_decode"]
WRAPPER = "cmk_roi_align_ratio"       # cmk_roi_align_pool with aligned = 1 and the ratio rule: one census row, bit-equal to the _pool call

FEATURES = [
    "census",        # one plain accepted case per kernel instantiation
    "views",         # input or output is a channel slice at a non-zero offset of a wider tensor
    "edge",          # the smallest geometries at which the index arithmetic or the algorithm branches
    "second_trip",   # a grid-stride loop or block walk takes a second iteration
    "padded_slots",  # counts of 0, partial and full in one launch: slots past counts get the declared filler, their inputs hold NaN
    "nonfinite",     # NaN and Inf: the answer is what the fp32 torch restatement gives
    "determinism",   # the same call again gives the same bits (the GPU module repeats EVERY accepted row; this cell is the plain one)
    "refuse",        # a non-zero return with an error text, nothing launched
]

SELECT, NMS, ROI, SAM, PREDICT, POOL, IOU, PASTE, PACK, PACK_KP, PREP, KPD = ENTRIES

RAGGED5 = [(25, 40), (13, 20), (7, 10), (4, 5), (2, 3)]          # test_detect_random_levels_vs_oracle
ROI3 = [(16, 20), (8, 10), (4, 5)]                                # a 128 x 160 padded batch at strides 8, 16, 32
SMALL = dict(n=3, topk=6, counts=[6, 0, 4])                       # test_gpu_roi_tail_ops.SMALL
CMK_EINVAL = -1                                                   # include/cmk.h: a refused argument (CMK_ELAUNCH = -2: a launch that failed)
KP_WS_WORDS = 36                                                  # keypoint.hip: 4 * (KP_SPLIT + 1) words per (RoI, keypoint)

# entry -> the arguments of a row and their defaults.  ws_short: words taken off the workspace length handed in.
DEFAULTS = {
    SELECT: dict(n=2, c=80, levels=RAGGED5, with_ctr=0, cap=16384, bias=-4.5, ws_short=0),
    NMS: dict(n=1, cap=1024, topk=50, counts=[900]),
    ROI: dict(n=2, topk=7, counts=[7, 4], c=8, levels=ROI3, out=14, sr=0, aligned=1, by_area=0, canonical=40.0, y_pad=0),
    SAM: dict(s=7, c=4, **SMALL),
    PREDICT: dict(s=7, c=4, classes=80, logits=1, **SMALL),
    POOL: dict(r=18, s=7, y_cs=40, y_co=33),
    IOU: dict(r=18, classes=80),
    PASTE: dict(r=6, s=28, h=40, w=300),
    PACK: dict(n=3, k=7, s=14),
    PACK_KP: dict(n=3, k=7, s=14, kp=1),
    PREP: dict(u8=1, h=37, w=53, hp=64, wp=96),
    KPD: dict(s=7, k=3, cs=12, co=0, ws_short=0, **SMALL),
}

# (entry, feature) cells that cannot be put, with the reason
N_A = {}
for _e in ENTRIES:
    if _e not in (ROI, POOL, IOU, KPD):
        N_A[(_e, "views")] = "the entry point takes dense tensors only: it has no channel stride or offset argument"
    if _e not in (SELECT, PREP, PACK, PACK_KP):
        N_A[(_e, "second_trip")] = "no grid-stride loop: the grid covers the work one to one (cmk_mask_pool_concat's loop never wraps, its grid is not " \
                                   "capped); the loops over C, S*S or the candidates that wrap inside a workgroup are edge rows"
    if _e not in (NMS, ROI, SAM, PREDICT, KPD):
        N_A[(_e, "padded_slots")] = "the entry point has no counts argument that marks slots as padding (cmk_pack_records copies every slot " \
                                    "whatever counts says; cmk_fcos_select writes counts)"
del _e
PRECONDITIONS = {
    NMS: "scores are non-negative (the sort key is the complement of the score's bits): a negative or -0.0 score, or a NaN with the sign bit "
         "set, is outside the documented precondition of cmk_nms_topk and has no row",
    ROI: "box sides stay at or below 4x the padded image and no box coordinate is non-finite: the adaptive sampling grid is ceil(side / out_size) "
         "per axis, an Inf or absurd box makes the kernel loop for hours",
    KPD: "box sides stay at or below 9000 px and no box coordinate of a valid slot is non-finite: the row loop is ceil(height)",
}


def kernels_of(c):
    """The kernels an accepted row launches."""
    return {SELECT: ["sel_count_kernel", "sel_scan_kernel", "sel_write_kernel"], NMS: ["nms_topk_kernel"], ROI: ["roi_align_kernel"],
            SAM: ["spatial_attention_kernel"], PREDICT: ["mask_predict_kernel"], POOL: ["mask_pool_kernel"], IOU: ["mask_iou_score_kernel"],
            PASTE: ["paste_masks_kernel"] if c.get("r") else [], PACK: ["pack_records_kernel"], PACK_KP: ["pack_records_kp_kernel"],
            PREP: ["preprocess_kernel<unsigned char>" if c.get("u8") else "preprocess_kernel<float>"],
            KPD: ["keypoint_band_kernel", "keypoint_finish_kernel"]}[c["entry"]]


def case(entry, feature, why="", data="", answer="accept", null=None, host_only=False, wrapper=False, **kw):
    c = dict(DEFAULTS[entry])
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    c.update(id="", entry=entry, feature=feature, answer="refuse" if feature == "refuse" else answer, why=why, data=data, null=null,
             host_only=host_only, wrapper=wrapper, kernels=[])
    if c["answer"] == "accept":
        c["kernels"] = kernels_of(c)
    return c


def _nulls(entry, **kw):
    return [case(entry, "refuse", "null " + p, null=p, **kw) for p in NULLABLE[entry]]


def _select_rows():
    r = [case(SELECT, "census", "two images, five ragged levels, the threshold on cls" + (" * ctr" if wc else ""), with_ctr=wc) for wc in (0, 1)]
    r += [case(SELECT, "edge", "one level of 1x1 with one class", n=1, c=1, levels=[(1, 1)], bias=0.0, cap=4),
          case(SELECT, "edge", "a level of exactly 4096 elements and one of 4097: its second block holds one element", c=1, levels=[(64, 64), (17, 241)], bias=-2.0),
          case(SELECT, "edge", "C = 3: a wave row straddles locations", c=3, levels=[(5, 7), (3, 4)], bias=-2.0, cap=256),
          case(SELECT, "edge", "8 levels (MAX_LEVELS)", c=5, levels=[(9, 11), (7, 8), (5, 6), (4, 5), (3, 4), (2, 3), (1, 2), (1, 1)], bias=-2.0, cap=2048),
          case(SELECT, "edge", "no candidate at all", bias=-30.0, cap=64),
          case(SELECT, "edge", "overflow: more candidates than cap; counts holds the true number, the first cap are written in flat order", cap=100),
          case(SELECT, "second_trip", "259 blocks: per = 2 in sel_scan, the threads from 130 up are empty", n=1, levels=[(115, 115)], cap=131072),
          case(SELECT, "nonfinite", "+Inf, -Inf and NaN logits, a NaN centre-ness, an Inf regression value", data="nonfinite", c=5, levels=[(5, 7), (3, 4)],
               bias=-1.0, cap=512),
          case(SELECT, "nonfinite", "... with the threshold on cls * ctr: NaN > thr is false", data="nonfinite", c=5, levels=[(5, 7), (3, 4)], bias=-1.0,
               cap=512, with_ctr=1),
          case(SELECT, "determinism", "ballot + scan: no atomics")]
    small = dict(c=3, levels=[(5, 7), (3, 4)], cap=256)
    r += _nulls(SELECT, **small)
    r += [case(SELECT, "refuse", "N = 0", n=0, **small), case(SELECT, "refuse", "C = 0", **dict(small, c=0)), case(SELECT, "refuse", "cap = 0", **dict(small, cap=0)),
          case(SELECT, "refuse", "no level", **dict(small, levels=[])), case(SELECT, "refuse", "nine levels", **dict(small, levels=[(2, 2)] * 9)),
          case(SELECT, "refuse", "a level with H = 0", **dict(small, levels=[(5, 7), (0, 4)])),
          case(SELECT, "refuse", "H*W*C >= 2^31", host_only=True, **dict(small, c=80, levels=[(6000, 6000)])),
          case(SELECT, "refuse", "a workspace one word too short", ws_short=1, **small)]
    return r


def _nms_rows():
    r = [case(NMS, "census", "the heavy-overlap case: stacked same-class boxes, score ties, IoU pairs straddling 0.6", data="heavy", cap=4096),
         case(NMS, "edge", "counts 0", data="grid", counts=[0], cap=64),
         case(NMS, "edge", "counts 1", data="grid", counts=[1], cap=64),
         case(NMS, "edge", "topk 1", data="heavy", topk=1, cap=4096),
         case(NMS, "edge", "topk 1024 (MAXK) with more than 1024 survivors", data="grid", topk=1024, counts=[1500], cap=2048),
         case(NMS, "edge", "cnt = 2 * NEED = 4096: the full sort", data="grid", counts=[4096], cap=4100),
         case(NMS, "edge", "cnt = 2 * NEED + 1 = 4097: the prefix sort", data="grid", counts=[4097], cap=4100),
         case(NMS, "edge", "cnt = 39999: the coordinate trick (the offset of class 79 rounds a pair of boxes onto each other)", data="per_class", counts=[39999], cap=40000),
         case(NMS, "edge", "cnt = 40000: NMS per class, on the same boxes plus one", data="per_class", counts=[40000], cap=40000),
         case(NMS, "edge", "all scores equal: one 12-bit bin, the prefix is everything", data="equal", counts=[5000], cap=5000),
         case(NMS, "edge", "counts above cap is clamped to cap", data="grid", counts=[900], cap=300),
         case(NMS, "edge", "three images on three paths in one launch: empty, full sort, prefix + fall-back to the full sort", data="mixed", n=3,
              counts=[0, 3000, 12000], cap=12288),
         case(NMS, "padded_slots", "counts 0, partial and full: the unused tail of the outputs holds zeros and idx -1; candidates past counts are NaN",
              data="grid", n=3, counts=[0, 20, 64], cap=64),
         case(NMS, "nonfinite", "a NaN score sorts first (as torch.sort puts it), then a +Inf score", data="nonfinite", counts=[200], cap=256),
         case(NMS, "determinism", "the histogram atomics are integer: the order is fixed", data="heavy", cap=4096)]
    small = dict(data="grid", counts=[20], cap=64)
    r += _nulls(NMS, **small)
    r += [case(NMS, "refuse", "N = 0", n=0, **small), case(NMS, "refuse", "cap = 0", **dict(small, cap=0)), case(NMS, "refuse", "topk 0", topk=0, **small),
          case(NMS, "refuse", "topk 1025 > MAXK", topk=1025, **small)]
    return r


def _roi_rows():
    r = []
    for by_area in (0, 1):
        for aligned in (1, 0):
            for sr in (0, 2):
                r.append(case(ROI, "census", "R = 14 is no multiple of 8: the padded XCD slots return early; {} rule, {}, sampling_ratio {}".format(
                    "area" if by_area else "ratio", "aligned" if aligned else "v1", sr), by_area=by_area, aligned=aligned, sr=sr))
    r.append(case(ROI, "census", "cmk_roi_align_ratio: equal to the _pool call bit for bit", wrapper=True))
    r += [case(ROI, "views", "y_cs > C: the channels past C of the output stay untouched", y_pad=16),
          case(ROI, "edge", "out_size 1", out=1), case(ROI, "edge", "out_size 7: 13 workgroups per RoI, the last holds one bin", out=7),
          case(ROI, "edge", "out_size 28", out=28, n=1, topk=3, counts=[3]),
          case(ROI, "edge", "four levels (MAXL)", levels=ROI3 + [(2, 3)]), case(ROI, "edge", "one level", levels=ROI3[:1]),
          case(ROI, "edge", "C = 516: the lanes loop twice with a ragged end", c=516, n=1, topk=5, counts=[5], out=7),
          case(ROI, "edge", "the crafted boxes: sub-pixel, outside the map, zero width", data="crafted", by_area=1, aligned=0),
          case(ROI, "edge", "the crafted boxes, ratio rule", data="crafted"),
          case(ROI, "padded_slots", "counts 0, partial and full: zeros and level -1 past counts, whose boxes are NaN", n=3, counts=[0, 3, 7]),
          case(ROI, "nonfinite", "NaN and Inf in the feature maps only: they reach exactly the bins whose samples touch them", data="nonfinite", sr=2),
          case(ROI, "determinism", "one thread owns each output: nothing to reorder")]
    r += _nulls(ROI)
    r += [case(ROI, "refuse", "null img_area under the ratio rule", null="img_area"), case(ROI, "refuse", "canonical_box_size 0 under the area rule", by_area=1, canonical=0.0),
          case(ROI, "refuse", "no level", levels=[]), case(ROI, "refuse", "five levels", levels=ROI3 + [(2, 3), (1, 2)]), case(ROI, "refuse", "C % 4", c=6),
          case(ROI, "refuse", "y_cs < C", y_pad=-4), case(ROI, "refuse", "y_cs % 4", y_pad=2), case(ROI, "refuse", "N = 0", n=0, counts=[]),
          case(ROI, "refuse", "topk = 0", topk=0), case(ROI, "refuse", "out_size 0", out=0), case(ROI, "refuse", "a level with H = 0", levels=[(16, 20), (0, 10)]),
          case(ROI, "refuse", "the grid: ceil(out^2 / 4) * R above 2^31 - 1 workgroups", host_only=True, n=60000, topk=1024, out=28)]
    return r


def _head_rows():
    r = []
    one = dict(n=1, topk=1, counts=[1])
    for e in (SAM, PREDICT):
        x = dict(classes=1) if e == PREDICT else {}
        r.append(case(e, "census", "3 images x 6 slots, counts 6 / 0 / 4"))
        for s in (1, 7, 14):
            for c in (4, 516):
                r.append(case(e, "edge", "S {} C {}".format(s, c) + ("; class-agnostic" if x and c == 4 else ""), s=s, c=c, **(x if c == 4 else {})))
        r.append(case(e, "edge", "R = 1", **one))
        r.append(case(e, "padded_slots", "slots at or beyond counts hold NaN and " + ("are left bit for bit" if e == SAM else "come out exactly 0"), data="padded"))
        r.append(case(e, "nonfinite", "a NaN in one RoI stays inside that RoI", data="nonfinite", c=8))
        r.append(case(e, "determinism", "wave reductions in a fixed order"))
        r += _nulls(e)
        r += [case(e, "refuse", "C % 4", c=6), case(e, "refuse", "S = 0", s=0), case(e, "refuse", "R = 0", n=0, counts=[]), case(e, "refuse", "topk = 0", topk=0),
              case(e, "refuse", "R % topk", data="ragged_r")]
    r += [case(PREDICT, "edge", "without logits_opt", logits=0), case(PREDICT, "edge", "without logits_opt, C 516, agnostic", logits=0, c=516, classes=1),
          case(PREDICT, "refuse", "R above 65535: gridDim.y", host_only=True, n=10923, topk=6, counts=[]),
          case(SAM, "edge", "S = 28: more pixels than the block has threads", s=28, **one),
          case(SAM, "refuse", "S = 74: 3*S*S*4 = 65712 bytes of LDS, more than a launch may ask for", host_only=True, s=74)]

    r += [case(POOL, "census", "R 18, S 7, channel 33 of 40"), case(POOL, "views", "channel 256 of 272, as the MaskIoU head runs it", s=14, y_cs=272, y_co=256),
          case(POOL, "edge", "S = 1", s=1), case(POOL, "edge", "R = 1", r=1), case(POOL, "edge", "the last channel: no pad channels", y_cs=34, y_co=33),
          case(POOL, "edge", "S = 14: 3528 outputs, the last block is ragged", s=14),
          case(POOL, "nonfinite", "a NaN mask value wins its 2x2 window as in max_pool2d; Inf comes through", data="nonfinite"),
          case(POOL, "determinism")]
    r += _nulls(POOL)
    r += [case(POOL, "refuse", "R = 0", r=0), case(POOL, "refuse", "S = 0", s=0), case(POOL, "refuse", "y_co = y_cs", y_cs=40, y_co=40),
          case(POOL, "refuse", "y_co < 0", y_co=-1)]

    r += [case(IOU, "census", "R 18, 80 classes"), case(IOU, "views", "iou_cs above the class count", data="wide"),
          case(IOU, "edge", "R = 1", r=1), case(IOU, "edge", "R = 257: a second block of one thread", r=257), case(IOU, "edge", "class-agnostic: one column", classes=1),
          case(IOU, "nonfinite", "NaN and Inf scores and IoUs multiply as in torch", data="nonfinite"), case(IOU, "determinism")]
    r += _nulls(IOU)
    r += [case(IOU, "refuse", "R = 0", r=0), case(IOU, "refuse", "R < 0", r=-3), case(IOU, "refuse", "iou_cs = 0", classes=0)]
    return r


def _prepost_rows():
    r = [case(PASTE, "census", "W = 300: a second, ragged x block; boxes inside, partly outside, larger than the image, under one pixel"),
         case(PASTE, "edge", "R = 0 returns OK and touches nothing", r=0), case(PASTE, "edge", "H = 1", h=1), case(PASTE, "edge", "S = 1", s=1),
         case(PASTE, "edge", "S = 13, W = 256: exactly one block", s=13, w=256), case(PASTE, "edge", "W = 1", w=1),
         case(PASTE, "edge", "a zero-width box and a box wholly outside paste nothing", data="degenerate"),
         case(PASTE, "nonfinite", "a NaN mask value: NaN >= threshold is false", data="nonfinite"), case(PASTE, "determinism")]
    r += _nulls(PASTE)
    r += [case(PASTE, "refuse", "R < 0", r=-1), case(PASTE, "refuse", "S = 0", s=0), case(PASTE, "refuse", "H = 0", h=0), case(PASTE, "refuse", "W = 0", w=0),
          case(PASTE, "refuse", "H above 65535: gridDim.y", host_only=True, h=65536), case(PASTE, "refuse", "R above 65535: gridDim.z", host_only=True, r=65536)]

    for e in (PACK, PACK_KP):
        kp = (lambda v: dict(kp=v)) if e == PACK_KP else (lambda v: {})
        r.append(case(e, "census", "3 x 7 slots, 14 x 14 masks: a record of {} floats".format(7 * (9 + 196 + (3 if e == PACK_KP else 0)) + 1)))
        r.append(case(e, "edge", "one image, one slot, a 1 x 1 mask: a record below one block", n=1, k=1, s=1))
        r.append(case(e, "second_trip", "8 x 50 slots, 28 x 28 masks: a block walks its record four times", n=8, k=50, s=28, **kp(17)))
        r.append(case(e, "second_trip", "1 x 100 slots, 28 x 28 masks", n=1, k=100, s=28, **kp(17)))
        r.append(case(e, "nonfinite", "NaN payloads are copied bit for bit", data="nonfinite"))
        r.append(case(e, "determinism"))
        r += _nulls(e)
        r += [case(e, "refuse", "N = 0", n=0), case(e, "refuse", "K = 0", k=0), case(e, "refuse", "mask_hw = 0", s=0),
              case(e, "refuse", "N above 65535: gridDim.y", host_only=True, n=65536),
              case(e, "refuse", "a record wider than an int", host_only=True, k=50000, s=256)]
    r.append(case(PACK_KP, "refuse", "no keypoints", kp=0))

    for u8 in (1, 0):
        t = "u8" if u8 else "fp32"
        r += [case(PREP, "census", t + ": padding on both sides", u8=u8),
              case(PREP, "edge", t + ": H == h and W == w, no padding", u8=u8, hp=37, wp=53),
              case(PREP, "edge", t + ": a 1 x 1 image in a 1 x 1 slot", u8=u8, h=1, w=1, hp=1, wp=1),
              case(PREP, "second_trip", t + ": 3 x 837 x 836 = 2,099,196 > 8192 x 256 elements", u8=u8, h=800, w=801, hp=837, wp=836),
              case(PREP, "determinism", t, u8=u8)]
    r.append(case(PREP, "nonfinite", "a NaN and an Inf in an fp32 image stay where they are", data="nonfinite", u8=0))
    r += _nulls(PREP)
    r += [case(PREP, "refuse", "h = 0", h=0), case(PREP, "refuse", "w = 0", w=0), case(PREP, "refuse", "H < h", hp=36), case(PREP, "refuse", "W < w", wp=52)]
    return r


def _keypoint_rows():
    r = [case(KPD, "census", "S 7, K 3, boxes: under one pixel, fractional, 240 x 240 (eight bands), 1300 x 7 (two bands), 9000 x 2 (three bands for two "
              "rows: one empty band record), zero width", data="randn"),
         case(KPD, "views", "dec_co = 5 of a wider buffer", data="randn", cs=20, co=5),
         case(KPD, "edge", "S = 1, K = 1", data="randn", s=1, k=1, cs=4),
         case(KPD, "edge", "S = 16 (KP_MAX_S: all of the LDS), K = 17", data="randn", s=16, k=17, cs=68),
         case(KPD, "edge", "all-zero maps: every tie goes to the first pixel across the bands", data="zeros"),
         case(KPD, "padded_slots", "counts 6 / 0 / 4: zeros past counts, whose boxes and maps are NaN", data="padded"),
         case(KPD, "nonfinite", "a NaN in one map: the first NaN wins and only that (RoI, keypoint) is affected", data="nonfinite"),
         case(KPD, "determinism", "fixed-order reductions, no atomics", data="randn")]
    r += _nulls(KPD)
    r += [case(KPD, "refuse", "K = 0", k=0), case(KPD, "refuse", "S = 0", s=0), case(KPD, "refuse", "S = 17 > KP_MAX_S", s=17), case(KPD, "refuse", "N = 0", n=0, counts=[]),
          case(KPD, "refuse", "topk = 0", topk=0), case(KPD, "refuse", "dec_co < 0", co=-1), case(KPD, "refuse", "dec_cs < dec_co + 4K", cs=12, co=4),
          case(KPD, "refuse", "a workspace one word too short", ws_short=1),
          case(KPD, "refuse", "more work items than 32 bits hold", host_only=True, n=65536, topk=64, counts=[])]
    return r


# the pointers of each entry point (the names call() takes), in the order of the C signature; those no row may NULL are left out of NULLABLE
POINTERS = {SELECT: ("levels", "logits", "regctr", "cand_box", "cand_score", "cand_cls", "cand_loc", "counts", "block_counts"),
            NMS: ("cand_box", "cand_score", "cand_cls", "cand_loc", "counts", "out_box", "out_score", "out_cls", "out_loc", "out_idx", "out_count", "sort_ws"),
            ROI: ("feats", "feat_h", "feat_w", "scales", "level0", "boxes", "counts", "img_area", "y", "out_level"),
            SAM: ("x", "w", "counts"), PREDICT: ("dec", "pw", "pb", "cls", "counts", "masks", "logits_opt"), POOL: ("masks", "y"),
            IOU: ("iou", "scores", "cls", "out"), PASTE: ("masks", "boxes", "out"),
            PACK: ("box", "score", "mscore", "loc", "cls", "masks", "counts", "rec"),
            PACK_KP: ("box", "score", "mscore", "loc", "cls", "masks", "kps", "counts", "rec"),
            PREP: ("src", "dst", "mean", "std"), KPD: ("dec", "boxes", "counts", "ws", "out")}
PER_LEVEL = ("logits", "regctr", "feats")            # one pointer per level
HOST_ARRAYS = ("levels", "feat_h", "feat_w", "scales", "mean", "std")      # built by call() on the host: a row can only NULL them
OPTIONAL = {ROI: ("img_area",), PREDICT: ("logits_opt",)}      # img_area: required under the ratio rule only (one refuse row)
NULLABLE = {SELECT: ("levels", "logits0", "regctr0", "cand_box", "cand_score", "cand_cls", "cand_loc", "counts", "block_counts"),      # logits0: levels[0].logits
            NMS: POINTERS[NMS], ROI: ("feats", "feat_h", "feat_w", "scales", "level0", "boxes", "counts", "y", "out_level"),              # level0: feats[0]
            SAM: POINTERS[SAM], PREDICT: ("dec", "pw", "pb", "cls", "counts", "masks"), POOL: POINTERS[POOL], IOU: POINTERS[IOU], PASTE: POINTERS[PASTE],
            PACK: POINTERS[PACK], PACK_KP: POINTERS[PACK_KP], PREP: POINTERS[PREP], KPD: POINTERS[KPD]}


def all_cases():
    rows = _select_rows() + _nms_rows() + _roi_rows() + _head_rows() + _prepost_rows() + _keypoint_rows()
    seen = {}
    for c in rows:
        geo = []
        for k, d in DEFAULTS[c["entry"]].items():
            v = c[k]
            if k == "levels":
                geo.append("+".join("{}x{}".format(*lv) for lv in v) or "no level")
            elif k == "counts":
                geo.append("counts" + "/".join(str(x) for x in v))
            elif k in ("n", "c", "r", "s", "k", "h", "w", "topk", "cap", "out") or v != d:
                geo.append("{}{}".format(k, v))
        for k in ("data", "null"):
            if c[k]:
                geo.append(("null-" if k == "null" else "") + c[k])
        if c["wrapper"]:
            geo.append(WRAPPER)
        name = " | ".join([c["entry"], c["feature"], " ".join(geo)])
        seen[name] = seen.get(name, 0) + 1
        c["id"] = name if seen[name] == 1 else "{} #{}".format(name, seen[name])
    return rows


# ---------------------------------------------------------------------------------------------------------------
# the C call of a row
# ---------------------------------------------------------------------------------------------------------------
def rois(c):
    """R of a row of the RoI heads: N * topk, or one more than a multiple of topk for the R % topk refusal."""
    return c["n"] * c["topk"] + (1 if c["data"] == "ragged_r" else 0)


def select_blocks(c):
    """Blocks per image of cmk_fcos_select, restated: ceil(H*W*C / 4096) per level."""
    return sum(-(-(h * w * c["c"]) // 4096) for h, w in c["levels"])


def dummy_pointers(c, ptr):
    """Every pointer of a row's call set to one aligned address (no refusal follows a pointer)."""
    nlev = len(c.get("levels") or [])
    return {k: ([ptr] * nlev if k in PER_LEVEL else ptr) for k in POINTERS[c["entry"]] if k not in HOST_ARRAYS and k != "level0"}


def call(lib, c, p, stream=None):
    """The row's entry point on the pointers p (name -> address, per level a list of addresses); the optional operands a row does without
    and the pointer named by c["null"] go in as NULL.  Returns the entry point's return code."""
    from centermask2_amd._lib import FcosLevel
    e = c["entry"]
    p = dict(p)
    null = c["null"]
    for k in ("logits", "regctr", "feats"):
        if k in p:
            p[k] = list(p[k])
    if null in ("logits0", "regctr0"):
        p[null[:-1]][0] = None
    elif null == "level0":
        p["feats"][0] = None
    elif null and null not in HOST_ARRAYS:
        assert null in p, (c["id"], null)
        p[null] = None

    def arr(ctype, values, name):
        values = list(values or [])
        return None if null == name else (ctype * max(1, len(values)))(*values)

    if e == SELECT:
        lv = c["levels"]
        levels = None
        if null != "levels":
            levels = (FcosLevel * max(1, len(lv)))()
            for i, (h, w) in enumerate(lv):
                j = min(i, len(p["logits"]) - 1)                # (a refused ninth level has no buffer of its own)
                levels[i] = FcosLevel(p["logits"][j], p["regctr"][j], h, w, 8 << i)
        ws_len = select_blocks(c) * c["n"] - c["ws_short"]
        return lib.cmk_fcos_select(levels, len(lv), c["n"], c["c"], 0.05, c["with_ctr"], p["cand_box"], p["cand_score"], p["cand_cls"], p["cand_loc"],
                                   p["counts"], p["block_counts"], ws_len, c["cap"], stream)
    if e == NMS:
        return lib.cmk_nms_topk(p["cand_box"], p["cand_score"], p["cand_cls"], p["cand_loc"], p["counts"], c["n"], c["cap"], 0.6, c["topk"], p["out_box"],
                                p["out_score"], p["out_cls"], p["out_loc"], p["out_idx"], p["out_count"], p["sort_ws"], stream)
    if e == ROI:
        lv = c["levels"]
        feats = arr(ctypes.c_void_p, p["feats"], "feats")
        fh, fw = arr(ctypes.c_int, [h for h, _ in lv], "feat_h"), arr(ctypes.c_int, [w for _, w in lv], "feat_w")
        scales = arr(ctypes.c_float, [1.0 / (8 << i) for i in range(len(lv))], "scales")
        y_cs = c["c"] + c["y_pad"]
        if c["wrapper"]:
            return lib.cmk_roi_align_ratio(feats, fh, fw, scales, len(lv), 3, c["c"], p["boxes"], p["counts"], p["img_area"], c["n"], c["topk"], c["out"], c["sr"],
                                           p["y"], y_cs, p["out_level"], stream)
        return lib.cmk_roi_align_pool(feats, fh, fw, scales, len(lv), 3, c["c"], p["boxes"], p["counts"], p["img_area"], c["n"], c["topk"], c["out"], c["sr"],
                                      c["aligned"], c["by_area"], c["canonical"], 4, p["y"], y_cs, p["out_level"], stream)
    if e == SAM:
        return lib.cmk_spatial_attention(p["x"], p["w"], p["counts"], c["topk"], rois(c), c["s"], c["c"], stream)
    if e == PREDICT:
        return lib.cmk_mask_predict(p["dec"], p["pw"], p["pb"], p["cls"], p["counts"], c["topk"], rois(c), c["s"], c["c"], p["masks"],
                                    p["logits_opt"] if c["logits"] else None, stream)
    if e == POOL:
        return lib.cmk_mask_pool_concat(p["masks"], p["y"], c["y_cs"], c["y_co"], c["r"], c["s"], stream)
    if e == IOU:
        return lib.cmk_mask_iou_score(p["iou"], c["classes"] + (16 if c["data"] == "wide" else 0), p["scores"], p["cls"], p["out"], c["r"], stream)
    if e == PASTE:
        return lib.cmk_paste_masks(p["masks"], p["boxes"], c["r"], c["s"], c["h"], c["w"], 0.5, p["out"], stream)
    if e == PACK:
        return lib.cmk_pack_records(p["box"], p["score"], p["mscore"], p["loc"], p["cls"], p["masks"], p["counts"], c["n"], c["k"], c["s"], p["rec"], stream)
    if e == PACK_KP:
        return lib.cmk_pack_records_kp(p["box"], p["score"], p["mscore"], p["loc"], p["cls"], p["masks"], p["kps"], p["counts"], c["n"], c["k"], c["s"], c["kp"],
                                       p["rec"], stream)
    if e == PREP:
        return lib.cmk_preprocess_chw(p["src"], c["u8"], p["dst"], c["h"], c["w"], c["hp"], c["wp"], arr(ctypes.c_float, PREP_MEAN, "mean"),
                                      arr(ctypes.c_float, PREP_STD, "std"), stream)
    if e == KPD:
        ws_len = max(0, c["n"] * c["topk"] * c["k"]) * KP_WS_WORDS - c["ws_short"]
        return lib.cmk_keypoint_decode(p["dec"], c["cs"], c["co"], c["s"], c["k"], p["boxes"], p["counts"], c["n"], c["topk"], p["ws"], ws_len, p["out"], stream)
    raise KeyError(e)


PREP_MEAN, PREP_STD = (103.53, 116.28, 123.675), (1.0, 57.0, 2.0)      # test_preprocess_matches_reference_padding
