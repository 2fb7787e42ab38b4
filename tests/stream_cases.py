"""The conformance table of the kernels that run between the convs (csrc/elementwise.hip, csrc/groupnorm.hip): the raw-image stem conv,
the max pools, the eSE gate and scale, the FPN's upsample + add and the GroupNorm entry points.  One row per case: the C entry point, the
kernels it launches (their cmk:: names as `nm -C` prints them), the geometry, the feature cell and the answer the library is declared to
give, accept or refuse.  Plain data plus call(), which turns a row and a dict of pointers into the C call.  No tests here:
tests/test_cpu_stream_conformance.py checks the census, the cells and every refusal on dummy pointers, tests/test_gpu_stream_conformance.py
launches every row on real buffers against float64.

A row is a dict (case() below gives the defaults):
  entry, feature, answer "accept" | "refuse", kernels [names], why (what the row is there for),
  n, h, w (the map an entry point's H, W or HW = h * w come from), c (channels; the stem: cout),
  x_view / y_view / id_view = (channel stride, channel offset) or None for a dense tensor, gate / identity (the optional operands),
  same_buffer (y is x), chunks (ws_chunks), rows (pixels per pooled block), groups, hc / wc (the coarse map),
  levels [(h, w)] (cmk_groupnorm_affine_multi) or [(h, w, records per image)] (cmk_groupnorm_affine_tiles),
  fill "randn" | "negative", poison (one +Inf in image 0, a -Inf in image 1, one NaN in image 2), null (the pointer handed in as NULL),
  host_only (a refusal whose buffers no test allocates: the row runs on dummy pointers only)."""
import ctypes

ENTRIES = ["cmk_stem_conv_nchw3", "cmk_maxpool3x3s2_ceil_nhwc", "cmk_maxpool1x1s2_nhwc", "cmk_ese_gate", "cmk_ese_gate_pooled", "cmk_ese_scale",
           "cmk_upsample2x_add_nhwc", "cmk_groupnorm_relu_nhwc", "cmk_groupnorm_nhwc", "cmk_groupnorm_affine", "cmk_groupnorm_affine_multi",
           "cmk_groupnorm_affine_tiles"]

FEATURES = [
    "census",        # one plain accepted case per kernel instantiation
    "views",         # input, output and identity are channel slices at non-zero offsets of wider tensors with three different strides
    "same_buffer",   # y = x
    "edge",          # the smallest geometries at which the index arithmetic branches
    "second_trip",   # the grid-stride loop takes a second iteration
    "nonfinite",     # one +Inf, one -Inf, one NaN
    "determinism",   # the same call again gives the same bits (the GPU module repeats EVERY accepted row; this cell is the plain one)
    "refuse",        # a non-zero return with an error text, nothing launched
]

STEM, POOL3, POOL1, GATE, POOLED, SCALE, UPADD, GN_RELU, GN, AFFINE, MULTI, TILES = ENTRIES
GN_INPLACE = (GN_RELU, GN)

# (entry, feature) cells that cannot be put, with the reason
N_A = {}
for _e in (STEM, POOLED, UPADD, GN_RELU, GN, AFFINE, MULTI, TILES):
    N_A[(_e, "views")] = "the entry point takes dense tensors only: it has no channel stride or offset argument"
for _e in ENTRIES:
    if _e != SCALE:
        N_A[(_e, "same_buffer")] = "the output has another shape than the input, or the call is in place by definition"
N_A[(STEM, "same_buffer")] = "an NCHW image in, an NHWC map of another size out"
N_A[(UPADD, "same_buffer")] = "y is updated in place already and the coarse map has another size"
for _e in (GATE, POOLED, AFFINE, MULTI, TILES):
    N_A[(_e, "second_trip")] = "no grid-stride loop: one workgroup per (chunk | 16 outputs | level, image); the loops over C that wrap are edge rows (C 1280, C 2048)"
del _e


def kernels_of(c):
    """The kernels an accepted row launches."""
    e = c["entry"]
    return {STEM: ["stem_conv_kernel<{}>".format(c["c"] // 32)], POOL3: ["maxpool3_kernel"], POOL1: ["subsample2_kernel"],
            GATE: ["ese_partial_kernel", "ese_fc_kernel"], POOLED: ["ese_fc_pooled_kernel"], SCALE: ["ese_scale_kernel"], UPADD: ["upsample2x_add_kernel"],
            GN_RELU: ["gn_stats_kernel", "gn_apply_kernel<true>"], GN: ["gn_stats_kernel", "gn_apply_kernel<false>"],
            AFFINE: ["gn_stats_kernel", "gn_finalize_kernel"], MULTI: ["gn_stats_multi_kernel", "gn_finalize_multi_kernel"],
            TILES: ["gn_finalize_tiles_kernel"]}[e]


def case(entry, feature, why="", answer="accept", **kw):
    c = dict(id="", entry=entry, feature=feature, answer=answer, kernels=[], why=why, n=2, h=5, w=7, c=32, x_view=None, y_view=None, id_view=None,
             gate=False, identity=False, same_buffer=False, chunks=3, rows=8, groups=8, hc=0, wc=0, levels=None, fill="randn", poison=False,
             null=None, host_only=False)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    if feature == "refuse":
        c["answer"] = "refuse"
    if c["answer"] == "accept":
        c["kernels"] = kernels_of(c)
    if entry == UPADD and not c["hc"]:
        c["hc"], c["wc"] = (c["h"] + 1) // 2, (c["w"] + 1) // 2
    return c


def gn_shape_ok(c, groups, chunks):
    """groupnorm.hip's gn_shape_ok, restated: what the statistics kernel's thread mapping and the 64-entry tables take."""
    return not (c % 4 or c < 4 or c > 1024 or groups < 1 or groups > 64 or c % groups or (c // groups) % 4 or 256 % (c // 4) or chunks < 1)


def _stem_rows():
    r = [case(STEM, "census", "Cout {}: stem_conv_kernel<{}>, several workgroups".format(co, co // 32), n=2, h=21, w=37, c=co) for co in (32, 64, 128)]
    for co in (32, 64, 128):
        for h, w in ((1, 1), (1, 2), (2, 2), (2, 3)):
            r.append(case(STEM, "edge", "a map below one 32-pixel tile: a single partial tile", n=1, h=h, w=w, c=co))
        r.append(case(STEM, "edge", "odd H and W", n=2, h=17, w=23, c=co))
        r.append(case(STEM, "edge", "even H and W", n=2, h=16, w=24, c=co))
        r.append(case(STEM, "edge", "Ho*Wo = 35: 32-pixel tiles straddle the three images, the last tile is ragged", n=3, h=9, w=13, c=co))
    r.append(case(STEM, "second_trip", "N*Ho*Wo = 525,625 > 4096 workgroups x 4 tiles x 32 pixels", n=1, h=1449, w=1449, c=32))
    r.append(case(STEM, "nonfinite", "relu(NaN) = 0 is the conv family's documented choice (groupnorm.hip); an Inf stays an Inf", n=3, h=9, w=13, c=64, poison=True))
    r.append(case(STEM, "determinism", n=2, h=21, w=37, c=64))
    r.append(case(STEM, "refuse", "Cout 48", c=48))
    r.append(case(STEM, "refuse", "Cout 256", c=256))
    r.append(case(STEM, "refuse", "3*H*W >= 2^31: the tap offsets are ints", n=1, h=26755, w=26755, c=64, host_only=True))
    r.append(case(STEM, "refuse", "null output", c=64, null="y"))
    return r


def _pool_rows():
    r = [case(POOL3, "census", n=2, h=9, w=13, c=32),
         case(POOL3, "views", "as forward_views runs it: into a channel slice of the next stage's concat buffer", n=2, h=9, w=13, c=36,
              x_view=(64, 12), y_view=(56, 8), gate=True)]
    for h in range(3, 9):
        for w in range(3, 9):
            r.append(case(POOL3, "edge", "ceil-mode windows over the right / bottom edge or an exact fit; C4 = 1", n=3, h=h, w=w, c=4))
            r.append(case(POOL3, "edge", "... C = 36, gated per image", n=3, h=h, w=w, c=36, gate=True))
    r.append(case(POOL3, "edge", "C4 = 1 gated", n=3, h=5, w=6, c=4, gate=True))
    r.append(case(POOL3, "edge", "C = 36 without a gate", n=3, h=6, w=5, c=36))
    for gate in (False, True):
        r.append(case(POOL3, "edge", "all-negative input: the -inf initial value must not leak", n=3, h=6, w=7, c=36, fill="negative", gate=gate))
        r.append(case(POOL3, "nonfinite", "a NaN wins its windows, an all -inf window comes out -inf", n=3, h=7, w=8, c=8, poison=True, gate=gate))
    r.append(case(POOL3, "second_trip", "N*Ho*Wo*C/4 = 1,065,024 float4 items > 4096 x 256", n=1, h=259, w=259, c=256))
    r.append(case(POOL3, "determinism", n=2, h=9, w=13, c=32, gate=True))
    r += [case(POOL3, "refuse", "H = 2 < the window", h=2), case(POOL3, "refuse", "W = 2 < the window", w=2), case(POOL3, "refuse", "C % 4", c=6),
          case(POOL3, "refuse", "x_cs % 4", x_view=(34, 0)), case(POOL3, "refuse", "y_co % 4", y_view=(40, 2)), case(POOL3, "refuse", "null input", null="x")]

    r += [case(POOL1, "census", n=2, h=9, w=13, c=32), case(POOL1, "views", n=2, h=9, w=13, c=36, x_view=(64, 12), y_view=(56, 8))]
    for h, w in ((1, 1), (1, 2), (2, 1), (7, 9), (6, 8)):
        r.append(case(POOL1, "edge", "1x1, 1x2, odd and even maps; C4 = 1", n=3, h=h, w=w, c=4))
    r.append(case(POOL1, "second_trip", "N*Ho*Wo*C/4 = 1,048,600 > 4096 x 256 (one row: the input is only twice the output)", n=1, h=1, w=2097199, c=4))
    r.append(case(POOL1, "nonfinite", "a copy: every bit pattern comes through", n=3, h=7, w=8, c=8, poison=True))
    r.append(case(POOL1, "determinism", n=2, h=9, w=13, c=32))
    r += [case(POOL1, "refuse", "C % 4", c=6), case(POOL1, "refuse", "N = 0", n=0), case(POOL1, "refuse", "H = 0", h=0),
          case(POOL1, "refuse", "x_co % 4", x_view=(40, 2)), case(POOL1, "refuse", "null output", null="y")]

    r += [case(UPADD, "census", n=2, h=9, w=13, c=32)]
    for h, w, hc, wc in ((1, 1, 1, 1), (1, 2, 1, 1), (7, 9, 4, 5), (6, 8, 3, 4), (5, 5, 4, 4)):
        r.append(case(UPADD, "edge", "1x1 and 1x2 maps, odd sizes over a ceil-halved coarse map, a coarse map larger than needed; C4 = 1", n=3, h=h, w=w, hc=hc, wc=wc, c=4))
    r.append(case(UPADD, "second_trip", "N*H*W*C/4 = 1,081,600 > 4096 x 256", n=1, h=65, w=65, c=1024))
    r.append(case(UPADD, "nonfinite", n=3, h=7, w=8, c=8, poison=True))
    r.append(case(UPADD, "determinism", n=2, h=9, w=13, c=32))
    r += [case(UPADD, "refuse", "coarse map too low", h=9, w=13, hc=4, wc=7), case(UPADD, "refuse", "coarse map too narrow", h=9, w=13, hc=5, wc=6),
          case(UPADD, "refuse", "C % 4", c=6), case(UPADD, "refuse", "N = 0", n=0), case(UPADD, "refuse", "null coarse map", null="coarse")]
    return r


GATE_C = {4: "C/4 = 1: 256 pixel lanes", 24: "C/4 = 6: 42 pixel lanes, 4 threads idle", 40: "the last 16-output workgroup holds 8",
          112: "C/4 = 28: 9 pixel lanes (V-19-slim)", 256: "the production size", 1024: "C/4 = 256: one pixel lane", 1280: "C/4 > 256: the loops over C take a second pass"}
GATE_CHUNKS = {1: "one chunk", 3: "259 = 87 + 87 + 85: a ragged last chunk", 300: "more chunks than pixels: the trailing ones are empty and must hold exact zeros",
               256: "256 chunks of 2 pixels: 130 used, 126 empty"}


def _ese_rows():
    r = [case(GATE, "census", n=2, h=7, w=37, c=256, chunks=4),
         case(GATE, "views", "x is a channel slice (the gate and the workspace are dense by the ABI)", n=2, h=7, w=37, c=112, x_view=(144, 16), chunks=3)]
    for c, why in GATE_C.items():
        for chunks, why2 in GATE_CHUNKS.items():
            r.append(case(GATE, "edge", why + "; " + why2, n=2, h=7, w=37, c=c, chunks=chunks))
    r += [case(GATE, "edge", "H*W = 1", n=2, h=1, w=1, c=112, chunks=1), case(GATE, "edge", "H*W = 1 and four chunks", n=2, h=1, w=1, c=112, chunks=4),
          case(GATE, "edge", "H*W = 1, C 1280", n=2, h=1, w=1, c=1280, chunks=1)]
    r.append(case(GATE, "nonfinite", "a NaN in the map makes that image's gates NaN, as relu6 does in torch", n=3, h=7, w=37, c=112, chunks=3, poison=True))
    r.append(case(GATE, "determinism", "the partial sums are fixed-order", n=2, h=7, w=37, c=256, chunks=256))
    r += [case(GATE, "refuse", "C % 4", c=6), case(GATE, "refuse", "no chunks", chunks=0), case(GATE, "refuse", "N = 0", n=0),
          case(GATE, "refuse", "H*W = 0: the mean would divide by zero", h=0), case(GATE, "refuse", "x_cs % 4", c=112, x_view=(114, 0)),
          case(GATE, "refuse", "null workspace", null="ws")]

    r += [case(POOLED, "census", "blocks of 128 rows straddle the two images", n=2, h=7, w=37, c=256, rows=128)]
    r += [case(POOLED, "edge", "H*W a multiple of rows: no block straddles, every odd record is NaN", n=3, h=4, w=6, c=112, rows=8),
          case(POOLED, "edge", "H*W = 35, rows 8: blocks straddle images", n=3, h=5, w=7, c=112, rows=8),
          case(POOLED, "edge", "H*W = rows", n=3, h=5, w=7, c=40, rows=35),
          case(POOLED, "edge", "300 blocks per image over 256 parts: the record loop wraps", n=2, h=10, w=30, c=4, rows=1),
          case(POOLED, "edge", "C 1280", n=3, h=5, w=7, c=1280, rows=8),
          case(POOLED, "edge", "C 24", n=3, h=5, w=7, c=24, rows=8)]
    r.append(case(POOLED, "nonfinite", n=3, h=5, w=7, c=112, rows=8, poison=True))
    r.append(case(POOLED, "determinism", n=3, h=5, w=7, c=112, rows=8))
    r += [case(POOLED, "refuse", "H*W < rows", h=5, w=7, rows=36), case(POOLED, "refuse", "rows = 0", rows=0), case(POOLED, "refuse", "C % 4", c=6),
          case(POOLED, "refuse", "N = 0", n=0), case(POOLED, "refuse", "null gate", null="gate")]

    r += [case(SCALE, "census", n=2, h=5, w=7, c=32, identity=True),
          case(SCALE, "views", n=2, h=5, w=7, c=36, x_view=(64, 12), y_view=(56, 8), id_view=(48, 4), identity=True),
          case(SCALE, "same_buffer", "element i reads then writes element i", n=2, h=5, w=7, c=32, identity=True, same_buffer=True),
          case(SCALE, "same_buffer", "... without an identity", n=2, h=5, w=7, c=32, same_buffer=True)]
    for c in (4, 1280):
        for identity in (False, True):
            r.append(case(SCALE, "edge", "C {} {} an identity".format(c, "with" if identity else "without"), n=3, h=5, w=7, c=c, identity=identity))
    r.append(case(SCALE, "edge", "H*W = 1", n=3, h=1, w=1, c=8, identity=True))
    r.append(case(SCALE, "second_trip", "N*H*W*C/4 = 1,081,600 > 4096 x 256", n=1, h=65, w=65, c=1024))
    r.append(case(SCALE, "nonfinite", n=3, h=7, w=8, c=8, identity=True, poison=True))
    r.append(case(SCALE, "determinism", n=2, h=5, w=7, c=32, identity=True))
    r += [case(SCALE, "refuse", "C % 4", c=6), case(SCALE, "refuse", "id_cs % 4", identity=True, id_view=(34, 0)), case(SCALE, "refuse", "N = 0", n=0),
          case(SCALE, "refuse", "H*W = 0", h=0), case(SCALE, "refuse", "null gate", null="gate")]
    return r


GN_HW_CHUNKS = [(1, 1, 1), (1, 1, 3), (1, 2, 3), (5, 7, 1), (5, 7, 3), (5, 7, 40)]     # (h, w, chunks): chunks > HW, chunks that do not divide HW


def _gn_rows():
    r = []
    for e in (GN_RELU, GN, AFFINE):
        r.append(case(e, "census", n=2, h=5, w=7, c=64, groups=16, chunks=3))
        for c in (4, 16, 64, 256, 1024):
            for groups in sorted({1, c // 4, 64}):
                for h, w, chunks in GN_HW_CHUNKS:
                    ok = gn_shape_ok(c, groups, chunks)
                    if not ok and (h, w, chunks) != GN_HW_CHUNKS[0]:
                        continue                           # one row per refused (C, groups)
                    r.append(case(e, "edge" if ok else "refuse", "C {} in {} groups, H*W {}, {} chunks".format(c, groups, h * w, chunks), n=2, h=h, w=w, c=c,
                                  groups=groups, chunks=chunks))
        if e in GN_INPLACE:
            r.append(case(e, "second_trip", "H*W*C/4 = 262,400 > 1024 workgroups per image x 256", n=1, h=25, w=41, c=1024, groups=32, chunks=8))
        r.append(case(e, "nonfinite", "+Inf, -Inf and NaN each make their (image, group) NaN in float64" +
                      ("; relu(NaN) = 0 is the conv family's documented choice (groupnorm.hip)" if e == GN_RELU else ""),
                      n=3, h=5, w=7, c=64, groups=4, chunks=3, poison=True))
        r.append(case(e, "determinism", "the records are summed in index order", n=2, h=5, w=7, c=64, groups=16, chunks=3))
        r += [case(e, "refuse", "C % 4", c=6, groups=1), case(e, "refuse", "C 2048 > 1024", c=2048, groups=32), case(e, "refuse", "C % groups", c=64, groups=5),
              case(e, "refuse", "2 channels per group", c=16, groups=8), case(e, "refuse", "256 % (C/4)", c=48, groups=1),
              case(e, "refuse", "no chunks", c=64, groups=16, chunks=0), case(e, "refuse", "N = 0", c=64, groups=16, n=0),
              case(e, "refuse", "H*W = 0", c=64, groups=16, h=0), case(e, "refuse", "null workspace", c=64, groups=16, null="ws")]

    five = [(20, 36), (9, 17), (5, 3), (3, 2), (1, 1)]
    r += [case(MULTI, "census", n=2, c=64, groups=16, chunks=3, levels=[(5, 7), (3, 4)]),
          case(MULTI, "edge", "one level", n=2, c=64, groups=16, chunks=3, levels=[(5, 7)]),
          case(MULTI, "edge", "five levels of different H*W", n=2, c=256, groups=32, chunks=4, levels=five),
          case(MULTI, "edge", "five levels, 64 groups of C 1024, chunks beyond the small levels' H*W", n=2, c=1024, groups=64, chunks=40, levels=five),
          case(MULTI, "nonfinite", n=3, c=64, groups=4, chunks=3, levels=[(5, 7), (3, 4)], poison=True),
          case(MULTI, "determinism", n=2, c=64, groups=16, chunks=3, levels=[(5, 7), (3, 4)]),
          case(MULTI, "refuse", "no level", c=64, groups=16, levels=[]), case(MULTI, "refuse", "six levels", c=64, groups=16, levels=five + [(1, 2)]),
          case(MULTI, "refuse", "a level of no pixels", c=64, groups=16, levels=[(5, 7), (0, 4)]), case(MULTI, "refuse", "256 % (C/4)", c=48, groups=1, levels=[(5, 7)]),
          case(MULTI, "refuse", "N = 0", n=0, c=64, groups=16, levels=[(5, 7)]), case(MULTI, "refuse", "null workspace", c=64, groups=16, levels=[(5, 7)], null="ws")]

    r.append(case(TILES, "census", n=2, c=64, groups=32, levels=[(5, 7, 3)]))
    for c, groups in ((6, 3), (64, 32), (2048, 32), (256, 64)):
        parts = 256 // groups
        why = "C {} in {} groups, {} parts".format(c, groups, parts) + ("; no multiple-of-4 rule here" if c == 6 else "") + ("; a second pass over c" if c == 2048 else "")
        r.append(case(TILES, "edge", why + ": 1 and parts - 1 records, the second level at a non-zero tile_begin", n=2, c=c, groups=groups,
                      levels=[(5, 7, 1), (9, 11, parts - 1)]))
        r.append(case(TILES, "edge", why + ": 4 * parts + 3 records run the four-chain loop and the remainder loop", n=2, c=c, groups=groups,
                      levels=[(9, 11, 4 * parts + 3), (5, 7, parts - 1)]))
    r.append(case(TILES, "nonfinite", n=3, c=64, groups=4, levels=[(5, 7, 3), (3, 4, 2)], poison=True))
    r.append(case(TILES, "determinism", "the four chains and the parts are summed in a fixed order", n=2, c=64, groups=32, levels=[(9, 11, 35), (5, 7, 3)]))
    r += [case(TILES, "refuse", "65 groups", c=130, groups=65, levels=[(5, 7, 3)]), case(TILES, "refuse", "C % groups", c=64, groups=3, levels=[(5, 7, 3)]),
          case(TILES, "refuse", "C 8192 > 4096", c=8192, groups=32, levels=[(5, 7, 3)]), case(TILES, "refuse", "no level", c=64, groups=32, levels=[]),
          case(TILES, "refuse", "six levels", c=64, groups=32, levels=[(5, 7, 3)] * 6), case(TILES, "refuse", "N = 0", n=0, c=64, groups=32, levels=[(5, 7, 3)]),
          case(TILES, "refuse", "a level without records", c=64, groups=32, levels=[(5, 7, 0)]),
          case(TILES, "refuse", "null records", c=64, groups=32, levels=[(5, 7, 3)], null="ws")]
    return r


def all_cases():
    rows = _stem_rows() + _pool_rows() + _ese_rows() + _gn_rows()
    seen = {}
    for c in rows:
        geo = "n{} {}x{} c{}".format(c["n"], c["h"], c["w"], c["c"]) if c["levels"] is None else "n{} c{} {}".format(
            c["n"], c["c"], "+".join("x".join(str(v) for v in lv) for lv in c["levels"]) or "no level")
        extra = []
        for k in ("x_view", "y_view", "id_view"):
            if c[k]:
                extra.append("{}{}".format(k[0], "/".join(str(v) for v in c[k])))
        for k in ("gate", "identity", "same_buffer", "poison"):
            if c[k]:
                extra.append(k)
        if c["entry"] in (GATE, GN_RELU, GN, AFFINE, MULTI):
            extra.append("chunks{}".format(c["chunks"]))
        if c["entry"] == POOLED:
            extra.append("rows{}".format(c["rows"]))
        if c["entry"] in (GN_RELU, GN, AFFINE, MULTI, TILES):
            extra.append("g{}".format(c["groups"]))
        if c["entry"] == UPADD:
            extra.append("coarse{}x{}".format(c["hc"], c["wc"]))
        if c["fill"] != "randn":
            extra.append(c["fill"])
        if c["null"]:
            extra.append("null-" + c["null"])
        name = " | ".join([c["entry"], c["feature"], " ".join([geo] + extra)])
        seen[name] = seen.get(name, 0) + 1
        c["id"] = name if seen[name] == 1 else "{} #{}".format(name, seen[name])
    return rows


# ---------------------------------------------------------------------------------------------------------------
# the C call of a row
# ---------------------------------------------------------------------------------------------------------------
POINTERS = {STEM: ("x", "w", "scale", "shift", "y"), POOL3: ("x", "y", "gate"), POOL1: ("x", "y"), GATE: ("x", "fc_w", "fc_b", "gate", "ws"),
            POOLED: ("pool_ws", "fc_w", "fc_b", "gate"), SCALE: ("x", "gate", "identity", "y"), UPADD: ("y", "coarse"),
            GN_RELU: ("x", "gamma", "beta", "ws"), GN: ("x", "gamma", "beta", "ws"), AFFINE: ("x", "gamma", "beta", "ws", "out_scale", "out_shift"),
            MULTI: ("xs", "gamma", "beta", "ws", "out_scale", "out_shift"), TILES: ("ws", "gamma", "beta", "out_scale", "out_shift")}
PER_LEVEL = ("xs", "out_scale", "out_shift")       # of MULTI and TILES: one pointer per level


def dummy_pointers(c, ptr):
    """Every pointer of a row's call set to one aligned address (no refusal follows a pointer)."""
    nlev = len(c["levels"] or [])
    per_level = PER_LEVEL if c["entry"] in (MULTI, TILES) else ()
    return {k: ([ptr] * nlev if k in per_level else ptr) for k in POINTERS[c["entry"]]}


def call(lib, c, p, stream=None):
    """The row's entry point on the pointers p (name -> address, per level a list of addresses); the optional operands a row does without
    and the pointer named by c["null"] go in as NULL.  Returns the entry point's return code."""
    e = c["entry"]
    p = dict(p)
    if e == POOL3 and not c["gate"]:
        p["gate"] = None
    if e == SCALE and not c["identity"]:
        p["identity"] = None
    if c["null"]:
        assert c["null"] in p, (c["id"], c["null"])
        p[c["null"]] = None
    n, h, w, ch, hw = c["n"], c["h"], c["w"], c["c"], c["h"] * c["w"]
    x_cs, x_co = c["x_view"] or (ch, 0)
    y_cs, y_co = c["y_view"] or (ch, 0)
    id_cs, id_co = (c["id_view"] or (ch, 0)) if c["identity"] else (0, 0)
    eps = 1e-5

    def arr(ctype, values):
        values = list(values) if values is not None else None
        return None if values is None else (ctype * max(1, len(values)))(*values)

    if e == STEM:
        return lib.cmk_stem_conv_nchw3(p["x"], p["w"], p["scale"], p["shift"], p["y"], n, h, w, ch, stream)
    if e == POOL3:
        return lib.cmk_maxpool3x3s2_ceil_nhwc(p["x"], x_cs, x_co, p["y"], y_cs, y_co, n, h, w, ch, p["gate"], stream)
    if e == POOL1:
        return lib.cmk_maxpool1x1s2_nhwc(p["x"], x_cs, x_co, p["y"], y_cs, y_co, n, h, w, ch, stream)
    if e == GATE:
        return lib.cmk_ese_gate(p["x"], x_cs, x_co, p["fc_w"], p["fc_b"], p["gate"], p["ws"], c["chunks"], n, hw, ch, stream)
    if e == POOLED:
        return lib.cmk_ese_gate_pooled(p["pool_ws"], c["rows"], p["fc_w"], p["fc_b"], p["gate"], n, hw, ch, stream)
    if e == SCALE:
        return lib.cmk_ese_scale(p["x"], x_cs, x_co, p["gate"], p["identity"], id_cs, id_co, p["y"], y_cs, y_co, n, hw, ch, stream)
    if e == UPADD:
        return lib.cmk_upsample2x_add_nhwc(p["y"], p["coarse"], n, h, w, c["hc"], c["wc"], ch, stream)
    if e in GN_INPLACE:
        fn = lib.cmk_groupnorm_relu_nhwc if e == GN_RELU else lib.cmk_groupnorm_nhwc
        return fn(p["x"], p["gamma"], p["beta"], p["ws"], c["chunks"], n, hw, ch, c["groups"], eps, stream)
    if e == AFFINE:
        return lib.cmk_groupnorm_affine(p["x"], p["gamma"], p["beta"], p["ws"], c["chunks"], n, hw, ch, c["groups"], eps, p["out_scale"], p["out_shift"], stream)
    levels = c["levels"]
    if e == MULTI:
        return lib.cmk_groupnorm_affine_multi(arr(ctypes.c_void_p, p["xs"]), arr(ctypes.c_int, [lh * lw for lh, lw in levels]), len(levels), p["gamma"], p["beta"],
                                              p["ws"], c["chunks"], n, ch, c["groups"], eps, arr(ctypes.c_void_p, p["out_scale"]),
                                              arr(ctypes.c_void_p, p["out_shift"]), stream)
    if e == TILES:
        return lib.cmk_groupnorm_affine_tiles(p["ws"], arr(ctypes.c_int, [lv[0] for lv in levels]), arr(ctypes.c_int, [lv[1] for lv in levels]),
                                              arr(ctypes.c_int, [lv[2] for lv in levels]), len(levels), p["gamma"], p["beta"], n, ch, c["groups"], eps,
                                              arr(ctypes.c_void_p, p["out_scale"]), arr(ctypes.c_void_p, p["out_shift"]), stream)
    raise KeyError(e)
