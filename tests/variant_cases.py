"""The conformance table of the conv kernels of the non-default backbones (csrc/conv_deform.hip, csrc/dwconv_bn_act.hip, csrc/conv_group3.hip,
csrc/stem7_pool.hip): the deformable 3x3 of the DCN stages, the fused and the plain depth-wise 3x3, the grouped 3x3 of ResNeXt and the fused
7x7 stem + max pool of ResNet.  One row per case: the C entry point, the kernel it launches (its cmk:: name as `nm -C` prints it), the
geometry, the feature cell and the answer the library is declared to give, accept or refuse.  Plain data plus call(), which turns a row and
a dict of pointers into the C call.  No tests here: tests/test_cpu_variant_conformance.py checks the census, the cells, the limits and every
refusal on dummy pointers, tests/test_gpu_variant_conformance.py launches every row on real buffers against float64.

A row is a dict (case() below gives the defaults, DEFAULTS the geometry per entry point):
  entry, feature, answer "accept" | "refuse", kernels [names], why (the edge the row puts),
  n, h, w (the input map), c (channels; deform and stem: Cout), cin / dg / modulated / offsets / mask / off_cs (deform), groups (grouped),
  stride, relu, clamps (in_max, out_min, out_max of the fused depth-wise entry),
  x_view / y_view = (channel stride, channel offset) or None for a dense tensor, same_buffer (x and y are slices of ONE tensor: y's pointer
  is x's), poison (one +Inf, one -Inf and one NaN in three different images), null (the pointer handed in as NULL), misalign (the pointer
  handed in 4 bytes off), host_only (a refusal whose buffers no test allocates: the row runs on dummy pointers only)."""
INF = float("inf")
CMK_EINVAL = -1                      # include/cmk.h: a refused argument (CMK_ELAUNCH = -2: a launch that failed)

ENTRIES = ["cmk_deform_conv3x3_nhwc", "cmk_dwconv3x3_bn_act_nhwc", "cmk_dwconv3x3_nhwc", "cmk_group_conv3x3_nhwc", "cmk_stem7x7_bn_relu_maxpool_nchw3"]
DEFORM, DWACT, DW, GROUP, STEM7 = ENTRIES

FEATURES = [
    "census",          # one plain accepted case per kernel instantiation, and the shapes that put the edges of its tiling
    "x_view",          # the input is a channel slice at a non-zero offset of a wider tensor
    "y_view",          # the output is a channel slice whose offset is a multiple of 4 but not of 16
    "same_buffer",     # x and y are disjoint channel slices of one tensor (stride 1)
    "no_act",          # relu 0, or the clamps off
    "one_pixel",       # a 1x1 map
    "one_row",
    "one_col",
    "n1",
    "odd_n",
    "offsets_edge",    # deform: samples exactly at -1 and just inside H-1 / W-1
    "offsets_far",     # deform: a third of the samples far outside the map, and one pixel whose nine taps all lie outside
    "offsets_int",     # deform: integer offsets, every sample on a pixel: three of its four corners are in-map corners of weight 0
    "mask_saturated",  # deform: mask logits of +-60
    "poison",          # one +Inf, one -Inf, one NaN
    "second_trip",     # the grid-stride loop takes a second iteration
    "refuse",          # CMK_EINVAL with an error text, nothing launched
]

# the geometry defaults per entry point.  (2, 7, 11) is 154 pixels: the image boundary sits inside the deformable kernel's first 128-pixel
# workgroup and the second workgroup is ragged.  (2, 21, 41) spans several tiles of every grouped kernel both ways and is ragged in both
# (tests/test_gpu_resnext.py); 19 x 27 pools to 5 x 7, ragged against the stem's 4 x 6 pooled tile both ways.
DEFAULTS = {
    DEFORM: dict(n=2, h=7, w=11, c=64, cin=32, dg=1, modulated=0, relu=1),
    DWACT: dict(n=2, h=9, w=13, c=24, stride=1, clamps=(6.0, 0.0, 6.0)),
    DW: dict(n=2, h=9, w=13, c=24, stride=1),
    GROUP: dict(n=2, h=21, w=41, c=32, groups=2, stride=1, relu=1),
    STEM7: dict(n=2, h=19, w=27, c=64),
}

POINTERS = {DEFORM: ("x", "offsets", "w", "scale", "shift", "y"), DWACT: ("x", "w", "scale", "shift", "y"), DW: ("x", "w", "y"),
            GROUP: ("x", "w", "scale", "shift", "y"), STEM7: ("x", "w", "scale", "shift", "y")}
NULLABLE = dict(POINTERS)            # every pointer is required: each has its NULL row
# the pointers read or written as 16-byte vectors (the others as single floats): each has its row 4 bytes off
ALIGN16 = {DEFORM: ("x", "w"), DWACT: POINTERS[DWACT], DW: POINTERS[DW], GROUP: POINTERS[GROUP], STEM7: ("y",)}

PRECONDITIONS = {
    DEFORM: "offsets and mask logits are finite: a NaN or Inf offset has no defined sample position (the float64 restatement has none either); "
            "the buffers hold what the shape says (cmk_conv_packed_floats(Cout, Cin, 3) floats of w, Cout of scale and shift)",
    DWACT: "w holds 9*C floats, scale and shift C each",
    DW: "w holds 9*C floats",
    GROUP: "w holds 9*Cg*C floats in the packing of csrc/conv_group3.hip, scale and shift C each",
    STEM7: "x is a dense (N,3,H,W) image, w holds 147*64 floats",
}

N_A = {}
for _f in ("offsets_edge", "offsets_far", "offsets_int", "mask_saturated"):
    for _e in (DWACT, DW, GROUP, STEM7):
        N_A[(_e, _f)] = "the entry point samples no offsets and takes no mask"
N_A[(STEM7, "x_view")] = "the input is a dense NCHW image: no channel stride or offset argument"
N_A[(STEM7, "same_buffer")] = "an NCHW image in, an NHWC map of another size out"
N_A[(STEM7, "no_act")] = "the ReLU before the pool is part of the entry point"
N_A[(DW, "no_act")] = "the plain depth-wise conv has no activation or clamp to switch off"
N_A[(DEFORM, "second_trip")] = "no grid-stride loop: one workgroup per 128 pixels and cout tile"
del _e, _f


# ---------------------------------------------------------------------------------------------------------------
# the host-side choices, restated
# ---------------------------------------------------------------------------------------------------------------
def out_hw(c):
    """The output map of a row."""
    if c["entry"] == STEM7:
        hc, wc = (c["h"] - 1) // 2 + 1, (c["w"] - 1) // 2 + 1
        return (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    s = c["stride"]
    return (c["h"] - 1) // s + 1, (c["w"] - 1) // s + 1


def deform_tiles(cout):
    """(cout tiles, WN): tiles of at most 7 blocks of 32 couts, as even as possible."""
    c32 = -(-cout // 32)
    ntiles = (c32 + 6) // 7
    return ntiles, -(-c32 // ntiles)


def dw_threads(c, t, r):
    """Threads of the depth-wise kernel at T = t columns x R = r rows per thread."""
    ho, wo = out_hw(c)
    return c["n"] * -(-ho // r) * -(-wo // t) * (c["c"] // 4)


def dw_blocks(c, t, r):
    return (dw_threads(c, t, r) + 255) // 256


DW_LADDER = {1: [(2, 4), (4, 1), (2, 1), (1, 1)], 2: [(2, 2), (2, 1), (1, 1)]}      # stride -> (T, R), largest first; the last rung takes what is left
DW_PLAIN = {1: (4, 1), 2: (2, 1)}
DW_GRID_CAP = {DWACT: 8192, DW: 4096}
GROUP_VALU_TILE = {1: (2, 2), 2: (4, 2)}                                              # stride -> (T, R)
GROUP_VALU_CAP = 16384
DW_MAX_GRID_STRIDE = 8192 * 256


def dw_tile(c):
    """(T, R) of the depth-wise kernel a row runs: the largest tile that still leaves 1024 workgroups; the plain entry has one per stride."""
    if c["entry"] == DW:
        return DW_PLAIN[c["stride"]]
    ladder = DW_LADDER[c["stride"]]
    for t, r in ladder[:-1]:
        if dw_blocks(c, t, r) >= 1024:
            return t, r
    return ladder[-1]


def group_valu_blocks(c):
    t, r = GROUP_VALU_TILE[c["stride"]]
    ho, wo = out_hw(c)
    return -(-(c["n"] * -(-ho // r) * -(-wo // t)) // 16) * -(-(c["c"] // 4) // 16)


def kernels_of(c):
    """The kernel an accepted row launches."""
    e = c["entry"]
    if e == DEFORM:
        return ["conv_deform_kernel<{}>".format(deform_tiles(c["c"])[1])]
    if e in (DWACT, DW):
        t, r = dw_tile(c)
        return ["dwconv3_bn_act_kernel<{}, {}, {}, {}>".format(c["stride"], t, r, "true" if e == DW else "false")]
    if e == GROUP:
        cg = c["c"] // c["groups"]
        if cg < 16:
            t, r = GROUP_VALU_TILE[c["stride"]]
            return ["group3_valu_kernel<{}, {}, {}, {}>".format(cg, c["stride"], t, r)]
        return ["group3_mfma_kernel<{}, {}>".format(cg, c["stride"])]
    return ["stem7_pool_kernel"]


def second_trip_threads(c):
    """(threads or workgroups of work, what one launch covers before the loop's second trip) of a second_trip row."""
    e = c["entry"]
    if e in (DWACT, DW):
        return dw_threads(c, *dw_tile(c)), DW_GRID_CAP[e] * 256
    if e == GROUP:
        return group_valu_blocks(c), GROUP_VALU_CAP
    ho, wo = out_hw(c)
    return c["n"] * -(-ho // 4) * -(-wo // 6), 2048


def second_trip_image(c):
    """The image that holds the first work item of the loop's second trip (the work index runs image-slowest)."""
    e, n = c["entry"], c["n"]
    ho, wo = out_hw(c)
    if e in (DWACT, DW):
        first, per_image = DW_GRID_CAP[e] * 256, dw_threads(c, *dw_tile(c)) // n
    elif e == GROUP:
        t, r = GROUP_VALU_TILE[c["stride"]]
        assert c["c"] // 4 <= 16                       # one 16-quad chunk: a workgroup is 16 pixel tiles
        first, per_image = GROUP_VALU_CAP * 16, -(-ho // r) * -(-wo // t)
    else:
        first, per_image = 2048, -(-ho // 4) * -(-wo // 6)
    return min(first // per_image, n - 1)


def need_off_cs(c):
    return (27 if c["modulated"] else 18) * c["dg"]


def cout_pad(cout):
    c32 = -(-cout // 32)
    return c32 * 32 if c32 <= 7 else -(-c32 // 4) * 128


def buffers(c):
    """name -> floats of every buffer the accepted row's call touches (views at their full width)."""
    n, h, w, ch = c["n"], c["h"], c["w"], c["c"]
    ho, wo = out_hw(c)
    xc = c["cin"] if c["entry"] == DEFORM else ch
    b = {"y": n * ho * wo * (c["y_view"] or (ch, 0))[0]}
    b["x"] = n * 3 * h * w if c["entry"] == STEM7 else n * h * w * (c["x_view"] or (xc, 0))[0]
    if c["entry"] == DEFORM:
        b["offsets"] = n * h * w * (c["off_cs"] or need_off_cs(c))
        b["w"] = 9 * (xc // 16) * cout_pad(ch) * 16
    elif c["entry"] == GROUP:
        b["w"] = 9 * (ch // c["groups"]) * ch
    elif c["entry"] == STEM7:
        b["w"] = 147 * 64
    else:
        b["w"] = 9 * ch
    return b


# ---------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------
def case(entry, feature, why="", answer="accept", **kw):
    c = dict(id="", entry=entry, feature=feature, answer=answer, kernels=[], why=why, n=2, h=5, w=7, c=8, cin=0, dg=1, modulated=0, offsets="frac",
             mask="randn", off_cs=None, groups=0, stride=1, relu=1, clamps=None, x_view=None, y_view=None, same_buffer=False, poison=False,
             null=None, misalign=None, host_only=False)
    c.update(DEFAULTS[entry])
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    if feature == "refuse":
        c["answer"] = "refuse"
    if c["answer"] == "accept":
        c["kernels"] = kernels_of(c)
    return c


def _common_rows(e, ch, xc, stride1_only_views=True, **kw):
    """The feature rows every entry point has: views, tiny maps, batch sizes.  ch: output channels, xc: input channels."""
    r = []
    if (e, "x_view") not in N_A:
        r.append(case(e, "x_view", "x is channels [12, 12 + C) of a wider pixel", x_view=(xc + 28, 12), **kw))
    r.append(case(e, "y_view", "y's offset 20 is a multiple of 4 and not of 16", y_view=(ch + 36, 20), **kw))
    if (e, "x_view") not in N_A:
        r.append(case(e, "y_view", "... with x a slice as well, of another stride", x_view=(xc + 8, 4), y_view=(ch + 36, 20), **kw))
    if (e, "same_buffer") not in N_A:
        r.append(case(e, "same_buffer", "x = channels [0, Cin), y = channels [Cin + 4, ...) of one tensor", x_view=(xc + ch + 8, 0),
                      y_view=(xc + ch + 8, xc + 4), same_buffer=True, **kw))
        r.append(case(e, "same_buffer", "... y before x", x_view=(xc + ch + 8, ch + 4), y_view=(xc + ch + 8, 0), same_buffer=True, **kw))
    for f, why, geo in (("one_pixel", "a 1x1 map: every tap but the centre is padding", dict(n=3, h=1, w=1)),
                        ("one_row", "H = 1: no row above or below", dict(n=2, h=1, w=13)), ("one_col", "W = 1", dict(n=2, h=13, w=1)),
                        ("n1", "one image", dict(n=1)), ("odd_n", "five images", dict(n=5))):
        r.append(case(e, f, why, **dict(kw, **geo)))
    return r


def _nulls(e, **kw):
    return [case(e, "refuse", "null " + k, null=k, **kw) for k in NULLABLE[e]]


def _misaligned(e, **kw):
    return [case(e, "refuse", k + " 4 bytes off a 16-byte boundary", misalign=k, **kw) for k in ALIGN16[e]]


def _deform_rows():
    e = DEFORM
    r = []
    for cout, cin, dg, mod, why in (
            (20, 16, 1, 0, "WN 1; Cout 20 is no multiple of 16 (12 dead columns); Cin 16 is a single chunk"),
            (64, 48, 2, 1, "WN 2; Cin 48: an odd chunk count, 24 channels per group"),
            (80, 32, 4, 1, "WN 3 with 16 dead columns in the last block; Cin/dg = 8: every 16-chunk straddles two deformable groups"),
            (128, 32, 1, 0, "WN 4"),
            (160, 16, 2, 1, "WN 5; one chunk that straddles two groups"),
            (192, 32, 2, 0, "WN 6: the stage-4 width of V-39 / V-99"),
            (224, 16, 1, 1, "WN 7: the widest single cout tile"),
            (232, 32, 4, 0, "two cout tiles of WN 4: the last block of the second holds 8 live columns"),
            (288, 48, 1, 1, "two cout tiles of WN 5: 5 and 4 blocks of 32, the second tile's last block is past cout_pad")):
        r.append(case(e, "census", why, c=cout, cin=cin, dg=dg, modulated=mod))
    kw = dict(c=20, cin=16, dg=2, modulated=1)
    r += _common_rows(e, 20, 16, **kw)
    r.append(case(e, "y_view", "an odd pixel stride and offset: y is written float by float", c=20, cin=16, y_view=(27, 5)))
    r.append(case(e, "x_view", "an offset tensor wider than 27*dg channels", off_cs=61, **kw))
    r.append(case(e, "no_act", "relu 0", relu=0, **kw))
    r.append(case(e, "one_pixel", "... two cout tiles", n=3, h=1, w=1, c=232, cin=32, dg=4, modulated=1))
    for kind in ("edge", "far", "int"):
        r.append(case(e, "offsets_" + kind, c=80, cin=32, dg=4, modulated=1, offsets=kind))
        r.append(case(e, "offsets_" + kind, "unmodulated, one group", c=20, cin=16, dg=1, modulated=0, offsets=kind))
    r.append(case(e, "mask_saturated", "logits of +-60: masks of exactly 1 and of 9e-27", c=64, cin=32, dg=2, modulated=1, mask="saturated"))
    for relu in (0, 1):
        tail = "" if not relu else "; with the ReLU, whose fmaxf gives relu(NaN) = 0 as in the other conv epilogues"
        r.append(case(e, "poison", "zero offsets: every border pixel has taps outside the map; +Inf at pixel (0,0) of image 0 (the stand-in address of an unread "
                      "corner), -Inf in the last row of image 1 (a zero-weight in-map corner of the row above), NaN in image 2" + tail,
                      n=3, h=5, w=6, c=20, cin=16, dg=2, modulated=1, offsets="zero", poison=True, relu=relu))
    r.append(case(e, "poison", "fractional offsets", n=3, h=5, w=6, c=64, cin=32, dg=4, modulated=0, offsets="frac", poison=True, relu=0))
    r.append(case(e, "poison", "far offsets: whole samples outside the map", n=3, h=5, w=6, c=20, cin=16, dg=1, modulated=1, offsets="far", poison=True, relu=0))

    r += _nulls(e, **kw) + _misaligned(e, **kw)
    r += [case(e, "refuse", "dg 3", c=20, cin=48, dg=3), case(e, "refuse", "dg 8", c=20, cin=64, dg=8), case(e, "refuse", "dg 0", c=20, cin=16, dg=0),
          case(e, "refuse", "Cin 24 is no multiple of 16", c=20, cin=24, dg=1), case(e, "refuse", "Cin/dg = 4", c=20, cin=16, dg=4),
          case(e, "refuse", "off_cs = 18*dg - 1", c=20, cin=16, dg=2, modulated=0, off_cs=35),
          case(e, "refuse", "off_cs = 27*dg - 1", c=20, cin=16, dg=2, modulated=1, off_cs=53),
          case(e, "refuse", "x_co + Cin = x_cs + 4", x_view=(16, 4), **kw), case(e, "refuse", "x_co = -4", x_view=(32, -4), **kw),
          case(e, "refuse", "x_cs = 2 mod 4", x_view=(18, 0), **kw), case(e, "refuse", "x_co = 2 mod 4", x_view=(24, 2), **kw),
          case(e, "refuse", "y_co + Cout = y_cs + 1", y_view=(20, 1), **kw), case(e, "refuse", "y_co = -1", y_view=(32, -1), **kw),
          case(e, "refuse", "x and y slices of one buffer that share four channels", x_view=(40, 0), y_view=(40, 12), same_buffer=True, **kw),
          case(e, "refuse", "x and y the same slice", c=16, cin=16, x_view=(16, 0), y_view=(16, 0), same_buffer=True)]
    for k in ("n", "h", "w", "cin", "c"):
        r.append(case(e, "refuse", k + " = 0", **dict(kw, **{k: 0})))
    r += [case(e, "refuse", "N*H*W*x_cs = 2^31", n=1, h=32768, w=4096, c=16, cin=16, host_only=True),
          case(e, "refuse", "N*H*W*y_cs = 2^31", n=1, h=32768, w=2048, c=32, cin=16, host_only=True),
          case(e, "refuse", "N*H*W*off_cs >= 2^31", n=1, h=32768, w=2048, c=16, cin=16, off_cs=32, host_only=True)]
    return r


def _dw_census(e):
    """Per rung of the ladder the smallest C that reaches it on a small odd map ('above': exactly 1024 workgroups), and C - 4, which falls to
    the next rung ('below': 1023)."""
    r = []
    if e == DW:
        return [case(e, "census", "stride 1, four columns per thread: Wo = 13 leaves one live column in the last thread", stride=1),
                case(e, "census", "stride 2, two columns per thread: Wo = 7", h=9, w=14, stride=2)]
    # stride 2 reads 4 pixels per output: a flat map (Ho = 3 of 5 rows, Wo = 3 of 6 columns) keeps the input below the size limit
    maps = {1: dict(n=2, h=13, w=11), 2: dict(n=16, h=5, w=6)}
    for stride, ladder in DW_LADDER.items():
        geo = dict(maps[stride], stride=stride)
        for t, rr in ladder[:-1]:
            probe = case(e, "census", c=4, **geo)
            per_quad = dw_threads(probe, t, rr)                       # threads per channel quad
            c4 = -(-(1023 * 256 + 1) // per_quad)
            for ch, side in ((4 * c4, "above: 1024"), (4 * c4 - 4, "below: 1023")):
                r.append(case(e, "census", "stride {} rung T {} x R {}, {} workgroups at that tile; Ho and Wo ragged against it".format(stride, t, rr, side),
                              c=ch, **geo))
        r.append(case(e, "census", "stride {}: the last rung, one output per thread".format(stride), **dict(geo, n=2)))
    return r


def _dw_rows(e):
    kw = dict(c=24)
    r = _dw_census(e)
    r += _common_rows(e, 24, 24, **kw)
    for f, why, geo in (("one_pixel", "stride 2", dict(n=3, h=1, w=1)), ("one_row", "stride 2, an even W", dict(n=2, h=1, w=14)),
                        ("one_col", "stride 2, an even H", dict(n=2, h=14, w=1)), ("x_view", "stride 2", dict(x_view=(52, 12), y_view=(60, 20), h=9, w=14))):
        r.append(case(e, f, why, stride=2, **dict(kw, **geo)))
    if e == DWACT:
        r.append(case(e, "no_act", "all three clamps off", clamps=(INF, -INF, INF), **kw))
        r.append(case(e, "no_act", "only the output clamp", clamps=(INF, 0.0, 6.0), **kw))
        r.append(case(e, "poison", "clamps on: min(+Inf, in_max) = in_max, -Inf and NaN pass", n=3, h=5, w=6, poison=True, **kw))
        r.append(case(e, "poison", "clamps off", n=3, h=5, w=6, poison=True, clamps=(INF, -INF, INF), **kw))
        r.append(case(e, "poison", "stride 2, clamps on", n=3, h=5, w=6, poison=True, stride=2, **kw))
        r.append(case(e, "second_trip", "32769 images of 5 x 7 x 32 at T 2 x R 4: 2,097,216 threads > 8192 workgroups x 256", n=32769, h=5, w=7, c=32))
    else:
        r.append(case(e, "poison", n=3, h=5, w=6, poison=True, **kw))
        r.append(case(e, "poison", "stride 2", n=3, h=5, w=6, poison=True, stride=2, **kw))
        r.append(case(e, "second_trip", "13108 images of 5 x 7 x 32 at T 4: 1,048,640 threads > 4096 workgroups x 256", n=13108, h=5, w=7, c=32))

    r += _nulls(e, **kw) + _misaligned(e, **kw)
    r += [case(e, "refuse", "C = 6", c=6), case(e, "refuse", "stride 3", stride=3, **kw), case(e, "refuse", "stride 0", stride=0, **kw),
          case(e, "refuse", "x_co + C = x_cs + 4", x_view=(24, 4), **kw), case(e, "refuse", "y_co + C = y_cs + 4", y_view=(24, 4), **kw),
          case(e, "refuse", "x_co = -4", x_view=(32, -4), **kw), case(e, "refuse", "y_co = -4", y_view=(32, -4), **kw),
          case(e, "refuse", "x_cs = 2 mod 4", x_view=(26, 0), **kw), case(e, "refuse", "y_cs = 2 mod 4", y_view=(26, 0), **kw),
          case(e, "refuse", "x_co = 2 mod 4", x_view=(32, 2), **kw), case(e, "refuse", "y_co = 2 mod 4", y_view=(32, 2), **kw),
          case(e, "refuse", "x and y slices of one buffer that share four channels", x_view=(56, 0), y_view=(56, 20), same_buffer=True, **kw),
          case(e, "refuse", "y = x in place: a thread would read what its neighbour wrote", same_buffer=True, **kw)]
    for k in ("n", "h", "w", "c"):
        r.append(case(e, "refuse", k + " = 0", **{k: 0}))
    if e == DWACT:
        r += [case(e, "refuse", "in_max NaN", clamps=(float("nan"), 0.0, 6.0), **kw), case(e, "refuse", "out_min NaN", clamps=(6.0, float("nan"), 6.0), **kw),
              case(e, "refuse", "out_max NaN", clamps=(6.0, 0.0, float("nan")), **kw), case(e, "refuse", "out_min > out_max", clamps=(6.0, 6.0, 0.0), **kw)]
    r += [case(e, "refuse", "N*Ho*Wo*C/4 = 46341^2 >= 2^31", n=1, h=46341, w=46341, c=4, host_only=True),
          case(e, "refuse", "N*Ho*Wo*C/4 = 46340^2 = 2^31 - 88,048: within one grid stride of 2^31, the loop index would wrap", n=1, h=46340, w=46340, c=4,
               host_only=True),
          case(e, "refuse", "... at stride 2", n=1, h=92679, w=92679, c=4, stride=2, host_only=True)]
    return r


def _group_rows():
    e = GROUP
    r = []
    for cg in (4, 8, 16, 32, 64):
        for stride in (1, 2):
            r.append(case(e, "census", "Cg {} stride {}: several tiles both ways, ragged in both".format(cg, stride), c=2 * cg, groups=2, stride=stride))
    r += [case(e, "census", "3 groups of 16: a group count that is no power of two on the MFMA kernel", c=48, groups=3),
          case(e, "census", "5 groups of 4: C/4 = 5 is a partial 16-quad chunk", c=20, groups=5),
          case(e, "census", "... at stride 2", c=20, groups=5, stride=2),
          case(e, "census", "6 groups of 8", c=48, groups=6),
          case(e, "census", "18 groups of 4: C/4 = 18 is one full and one partial 16-quad chunk", c=72, groups=18, n=1, h=9, w=13)]
    small = dict(h=9, w=13)
    for kw in (dict(c=20, groups=5, **small), dict(c=32, groups=2, **small)):
        r += _common_rows(e, kw["c"], kw["c"], **kw)
        r.append(case(e, "no_act", "relu 0", relu=0, **kw))
        r.append(case(e, "x_view", "stride 2", stride=2, x_view=(kw["c"] + 28, 12), y_view=(kw["c"] + 36, 20), **kw))
        r.append(case(e, "one_pixel", "stride 2", stride=2, **dict(kw, n=3, h=1, w=1)))
        for stride in (1, 2):
            r.append(case(e, "poison", "a NaN or Inf stays inside its group; a NaN passes the ReLU (stride {})".format(stride), poison=True, stride=stride,
                          **dict(kw, n=3, h=5, w=6)))
    r.append(case(e, "second_trip", "21846 images of 5 x 7 x 64 in 16 groups of 4: 16385 workgroups > 16384", n=21846, h=5, w=7, c=64, groups=16))

    kw = dict(c=32, groups=2, **small)
    r += _nulls(e, **kw) + _misaligned(e, **kw)
    r += [case(e, "refuse", "Cg = 12", c=24, groups=2), case(e, "refuse", "Cg = 128", c=256, groups=2), case(e, "refuse", "Cg = 2", c=8, groups=4),
          case(e, "refuse", "groups = 1", c=16, groups=1), case(e, "refuse", "groups = 0", c=16, groups=0), case(e, "refuse", "C % groups", c=32, groups=3),
          case(e, "refuse", "stride 3", stride=3, **kw), case(e, "refuse", "stride 0", stride=0, **kw),
          case(e, "refuse", "x_co + C = x_cs + 4", x_view=(32, 4), **kw), case(e, "refuse", "y_co + C = y_cs + 4", y_view=(32, 4), **kw),
          case(e, "refuse", "x_co = -4", x_view=(40, -4), **kw), case(e, "refuse", "y_co = -4", y_view=(40, -4), **kw),
          case(e, "refuse", "x_cs = 2 mod 4", x_view=(34, 0), **kw), case(e, "refuse", "y_cs = 2 mod 4", y_view=(34, 0), **kw),
          case(e, "refuse", "x_co = 2 mod 4", x_view=(40, 2), **kw), case(e, "refuse", "y_co = 2 mod 4", y_view=(40, 2), **kw),
          case(e, "refuse", "x and y slices of one buffer that share four channels", x_view=(72, 0), y_view=(72, 28), same_buffer=True, **kw),
          case(e, "refuse", "y = x in place", same_buffer=True, **kw)]
    for k in ("n", "h", "w", "c"):
        r.append(case(e, "refuse", k + " = 0", **dict(kw, **{k: 0})))
    r.append(case(e, "refuse", "N*Ho*Wo*C/4 = 2 * 32768^2 >= 2^31", n=1, h=32768, w=32768, c=8, groups=2, host_only=True))
    return r


def _stem_rows():
    e = STEM7
    r = [case(e, "census", "19 x 27 pools to 5 x 7: ragged against the 4 x 6 pooled tile both ways, odd H and W")]
    for h, w in ((18, 26), (18, 27), (19, 26), (20, 28), (21, 29)):
        r.append(case(e, "census", "H {} W {}: every parity of the image and of the conv map".format(h, w), h=h, w=w))
    r += _common_rows(e, 64, 3)
    r.append(case(e, "one_pixel", "2 x 2: one conv pixel", n=2, h=2, w=2))
    r.append(case(e, "poison", "a NaN wins every pooling window that holds its conv pixels, relu keeps it", n=3, h=19, w=27, poison=True))
    r.append(case(e, "second_trip", "2049 images of one 4 x 6 pooled tile each > 2048 workgroups", n=2049, h=5, w=9))
    r += _nulls(e) + _misaligned(e)
    r += [case(e, "refuse", "Cout 63", c=63), case(e, "refuse", "Cout 128", c=128), case(e, "refuse", "Cout 0", c=0),
          case(e, "refuse", "y_co + 64 = y_cs + 4", y_view=(64, 4)), case(e, "refuse", "y_co = -4", y_view=(72, -4)),
          case(e, "refuse", "y_cs = 2 mod 4", y_view=(66, 0)), case(e, "refuse", "y_co = 2 mod 4", y_view=(72, 2)),
          case(e, "refuse", "x one byte off", misalign="x1")]
    for k in ("n", "h", "w"):
        r.append(case(e, "refuse", k + " = 0", **{k: 0}))
    r.append(case(e, "refuse", "3*H*W >= 2^31", n=1, h=26755, w=26755, host_only=True))
    return r


def all_cases():
    rows = _deform_rows() + _dw_rows(DWACT) + _dw_rows(DW) + _group_rows() + _stem_rows()
    seen = {}
    for c in rows:
        e = c["entry"]
        geo = "n{} {}x{} c{}".format(c["n"], c["h"], c["w"], c["c"])
        extra = []
        if e == DEFORM:
            extra += ["cin{}".format(c["cin"]), "dg{}".format(c["dg"]), "mod{}".format(c["modulated"]), c["offsets"]]
            if c["mask"] != "randn":
                extra.append(c["mask"])
            if c["off_cs"] is not None:
                extra.append("offcs{}".format(c["off_cs"]))
        if e == GROUP:
            extra.append("g{}".format(c["groups"]))
        if e != STEM7:
            extra.append("s{}".format(c["stride"]))
        if e in (DEFORM, GROUP):
            extra.append("relu{}".format(c["relu"]))
        if e == DWACT:
            extra.append("clamps{}/{}/{}".format(*c["clamps"]))
        for k in ("x_view", "y_view"):
            if c[k]:
                extra.append("{}{}".format(k[0], "/".join(str(v) for v in c[k])))
        for k in ("same_buffer", "poison"):
            if c[k]:
                extra.append(k)
        if c["null"]:
            extra.append("null-" + c["null"])
        if c["misalign"]:
            extra.append("misaligned-" + c["misalign"])
        name = " | ".join([e, c["feature"], " ".join([geo] + extra)])
        seen[name] = seen.get(name, 0) + 1
        c["id"] = name if seen[name] == 1 else "{} #{}".format(name, seen[name])
    return rows


# ---------------------------------------------------------------------------------------------------------------
# the C call of a row
# ---------------------------------------------------------------------------------------------------------------
def dummy_pointers(c, ptr):
    """Every pointer of a row's call at its own 16-byte-aligned address inside a small buffer (no refusal follows a pointer); a same_buffer
    row gets y = x."""
    p = {k: ptr + 64 * i for i, k in enumerate(POINTERS[c["entry"]])}
    if c["same_buffer"]:
        p["y"] = p["x"]
    return p


def call(lib, c, p, stream=None):
    """The row's entry point on the pointers p (name -> address); the pointer named by c["null"] goes in as NULL, the one named by
    c["misalign"] 4 bytes further (x1: x one byte further).  Returns the entry point's return code."""
    e = c["entry"]
    p = dict(p)
    if c["null"]:
        assert c["null"] in p, (c["id"], c["null"])
        p[c["null"]] = None
    if c["misalign"] == "x1":
        p["x"] += 1
    elif c["misalign"]:
        p[c["misalign"]] += 4
    n, h, w, ch, stride = c["n"], c["h"], c["w"], c["c"], c["stride"]
    xc = c["cin"] if e == DEFORM else ch
    x_cs, x_co = c["x_view"] or (xc, 0)
    y_cs, y_co = c["y_view"] or (ch, 0)
    if e == DEFORM:
        off_cs = c["off_cs"] if c["off_cs"] is not None else need_off_cs(c)
        return lib.cmk_deform_conv3x3_nhwc(p["x"], x_cs, x_co, p["offsets"], off_cs, p["w"], p["scale"], p["shift"], p["y"], y_cs, y_co, n, h, w, xc, ch,
                                           c["dg"], c["modulated"], c["relu"], stream)
    if e == DWACT:
        in_max, out_min, out_max = c["clamps"]
        return lib.cmk_dwconv3x3_bn_act_nhwc(p["x"], x_cs, x_co, p["w"], p["scale"], p["shift"], in_max, out_min, out_max, p["y"], y_cs, y_co, n, h, w, ch,
                                             stride, stream)
    if e == DW:
        return lib.cmk_dwconv3x3_nhwc(p["x"], x_cs, x_co, p["w"], p["y"], y_cs, y_co, n, h, w, ch, stride, stream)
    if e == GROUP:
        return lib.cmk_group_conv3x3_nhwc(p["x"], x_cs, x_co, p["w"], p["scale"], p["shift"], p["y"], y_cs, y_co, n, h, w, ch, c["groups"], stride,
                                          c["relu"], stream)
    if e == STEM7:
        return lib.cmk_stem7x7_bn_relu_maxpool_nchw3(p["x"], p["w"], p["scale"], p["shift"], p["y"], y_cs, y_co, n, h, w, ch, stream)
    raise KeyError(e)

