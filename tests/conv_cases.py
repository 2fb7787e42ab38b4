"""The conv conformance table: every kernel instantiation of the conv library (census rows) and every (family, feature) cell of the
support matrix (feature rows), each with the answer the library is declared to give: accept or refuse.  Plain data plus the helpers that
turn a case into descriptors (dummy pointers for cmk_conv_plan, or real tensors for a launch) and into its float64 reference.  No tests
here: tests/test_cpu_conv_conformance.py plans every case, tests/test_gpu_conv_conformance.py launches them.

A case is a dict (case() below gives the defaults):
  k, stride, shapes [(N, H, W)], cin, cout, tv = (wm, sc, wn[, splitk[, tail ways]]), tail_tiles (cmk.h splitk_tail_tiles, as ops.TAIL_TILES),
  x_view / y_view = (channel stride, channel offset) or None for a dense tensor, same_buffer (x and y are disjoint channel slices of one
  tensor), relu_upto (None = Cout), in_relu, in_affine, res_mode 0 | 1 | 2 with res_view, per_problem (every problem its own scale and shift),
  weight_sets (2: the second half of the problems runs other weights), gn_groups, pool, zero_shift (the bar of tune_wm 11 is relative to the
  image's own magnitude, which a bias would hide), regime (None, or the value feature whose data tests/conv_values.py puts into the row's
  tensors: the rows of VALUE_FEATURES), answer "accept" | "refuse".

Shapes are the smallest at which a tiling can still go wrong: two images, more than one spatial tile and ragged in both directions, a Cout
that leaves masked columns in the last cout tile, an odd number of K chunks (Cin 48) or chunk pairs (Cin 96) where the family takes it."""
import ctypes

FAMILIES = {   # name -> the plain problem its feature rows start from
    "igemm 1x1":            dict(k=1, stride=1, shapes=[(2, 13, 19)], cin=48, cout=80, tv=(1, 32, 3)),
    "igemm 3x3 stride 1":   dict(k=3, stride=1, shapes=[(2, 19, 37)], cin=48, cout=80, tv=(1, 16, 3)),
    "igemm 3x3 stride 2":   dict(k=3, stride=2, shapes=[(2, 21, 35)], cin=48, cout=80, tv=(1, 16, 3)),
    "gather (wm 7)":        dict(k=3, stride=1, shapes=[(2, 13, 19)], cin=48, cout=80, tv=(7, 32, 1)),
    "pw (wm 8)":            dict(k=1, stride=1, shapes=[(2, 13, 19)], cin=96, cout=225, tv=(8, 32, 2)),
    "pw gather (wm 9)":     dict(k=3, stride=1, shapes=[(2, 13, 19)], cin=96, cout=225, tv=(9, 32, 2)),
    "pw split bf16 (wm 10)": dict(k=1, stride=1, shapes=[(2, 13, 19)], cin=96, cout=225, tv=(10, 32, 4)),
    "pw split fp16 (wm 12)": dict(k=1, stride=1, shapes=[(2, 13, 19)], cin=96, cout=225, tv=(12, 32, 4)),
    "wino4r (wm 5)":        dict(k=3, stride=1, shapes=[(2, 13, 41)], cin=48, cout=80, tv=(5, 16, 2)),
    "wino6 map tiles":      dict(k=3, stride=1, shapes=[(2, 13, 41)], cin=48, cout=80, tv=(6, 16, 1)),
    "wino6 RoI pairs":      dict(k=3, stride=1, shapes=[(4, 14, 14)], cin=48, cout=80, tv=(6, 16, 2)),
    "wino6p map tiles":     dict(k=3, stride=1, shapes=[(2, 13, 41)], cin=48, cout=80, tv=(6, 32, 1)),
    "wino6p RoI pairs":     dict(k=3, stride=1, shapes=[(4, 14, 14)], cin=48, cout=80, tv=(6, 32, 2)),
    "wino6s map tiles":     dict(k=3, stride=1, shapes=[(2, 13, 41)], cin=48, cout=80, tv=(6, 64, 1)),
    "wino6s RoI pairs":     dict(k=3, stride=1, shapes=[(4, 14, 14)], cin=48, cout=80, tv=(6, 64, 2)),
    "sp3 (sc 2)":           dict(k=3, stride=1, shapes=[(2, 19, 37)], cin=48, cout=80, tv=(11, 2, 1), zero_shift=True),
    "sp3 (sc 21)":          dict(k=3, stride=1, shapes=[(2, 19, 37)], cin=48, cout=80, tv=(11, 21, 0), zero_shift=True),
}

FEATURES = [
    "x_view",               # input: a channel slice of a wider tensor
    "y_view",               # output: a channel slice at an offset that is no multiple of 16
    "same_buffer",          # x and y are disjoint channel slices of ONE tensor (x_cs == y_cs: how every OSA block runs)
    "relu_partial",         # relu_upto that is no multiple of 32
    "relu_zero",            # relu_upto 0
    "in_relu",
    "in_affine",            # x' = relu(x * in_scale + in_shift) while staging; the padding stays zero
    "res_same",             # same-size residual through a view (res_co > 0, res_cs > Cout)
    "res_up_odd_h",         # nearest-2x upsampled residual cropped to an odd H (even W)
    "res_up_odd_w",         # ... to an odd H and an odd W
    "splitk2", "splitk4", "splitk8",
    "splitk_view_relu",     # split-K with an output view and a partial ReLU
    "splitk_res",           # split-K with a same-size residual
    "splitk_in_affine",
    "tail_splitk",          # cmk.h splitk_tail: the last tile of a RoI-pair launch split 2 ways
    "multi5",               # five problems, per-problem scale and shift, the last one 1x1 pixels
    "multi10_two_weights",  # ten problems, the second five on other weights
    "gn",                   # fused GroupNorm {sum, sumsq} records
    "gn_in_affine",
    "pool",                 # pooled sums of the eSE gate
    "odd_n",                # an odd image count (on the RoI-pair geometry: a last pair with one image)
    "n1",                   # one image
    # value features (tests/conv_values.py has the regimes, the emulations and the bars): the family's plain problem, a dense output
    "ints",                 # small integers: the output EQUALS float64, whatever the summation order (F(4x4): HELD_TO_BAR)
    "pow2_channels",        # x[..., c] * 2^e, w[:, c] * 2^-e: the bits of the plain launch (the fp16-split forms: HELD_TO_BAR)
    "cancel",               # x = 1 + 2^-9 r against zero-sum filters: the signal lives in the low bits of x
    "sparse",               # x = relu(r), every fifth channel and the last image zero, the fused ReLU on
    "nonfinite",            # one Inf, one NaN: every output outside the pixel's reach keeps the bits of the clean launch
    "f16_domain",           # the edges of the fp16 window cmk.h promises: max|x| = 1e6; a weight channel 2^-16 of the largest
]

# The support table: one letter per feature, in the order of FEATURES.  A = the family takes the feature and honours it, R = its front door
# refuses it (a non-zero return with an error text, nothing launched), - = the cell cannot be put (N_A below says why).
#                           x y s rp rz ir ia rs uh uw k2 k4 k8 kv kr ka tl m5 m10 gn ga pl on n1 in p2 ca sp nf fd
MATRIX = {
    "igemm 1x1":             "A A A A  A  A  A  A  A  A  A  A  A  A  A  A  R  A  R   R  R  R  A  A  A  A  A  A  A  -",
    "igemm 3x3 stride 1":    "A A A A  A  A  A  A  A  A  A  A  A  A  A  A  R  A  R   R  R  R  A  A  A  A  A  A  A  -",
    "igemm 3x3 stride 2":    "A A - A  A  A  A  A  A  A  A  A  A  A  A  A  R  A  R   R  R  R  A  A  A  A  A  A  A  -",
    "gather (wm 7)":         "A A A A  A  A  R  A  R  R  A  A  A  A  A  R  R  R  R   R  R  R  A  A  A  A  A  A  A  -",
    "pw (wm 8)":             "A A A A  A  R  R  A  A  R  A  A  A  A  A  R  R  R  R   R  R  A  A  A  A  A  A  A  A  -",
    "pw gather (wm 9)":      "A A A A  A  R  R  A  R  R  A  A  A  A  A  R  R  R  R   R  R  R  A  A  A  A  A  A  A  -",
    "pw split bf16 (wm 10)": "A A A A  A  R  R  R  A  R  R  R  R  R  R  R  R  R  R   R  R  A  A  A  A  A  A  A  A  -",
    "pw split fp16 (wm 12)": "A A A A  A  R  R  R  A  R  R  R  R  R  R  R  R  R  R   R  R  A  A  A  A  A  A  A  A  A",
    "wino4r (wm 5)":         "A A A A  A  R  A  R  R  R  R  R  R  R  R  R  R  A  R   A  A  R  A  A  A  A  A  A  A  -",
    "wino6 map tiles":       "A A A A  A  R  A  R  R  R  A  A  A  A  R  A  R  A  A   A  A  R  A  A  A  A  A  A  A  -",
    "wino6 RoI pairs":       "A A A A  A  R  A  R  R  R  A  A  A  A  R  A  A  R  R   R  R  R  A  A  A  A  A  A  A  -",
    "wino6p map tiles":      "A A A A  A  R  A  R  R  R  A  A  A  A  R  A  R  A  A   A  A  R  A  A  A  A  A  A  A  -",
    "wino6p RoI pairs":      "A A A A  A  R  A  R  R  R  A  A  A  A  R  A  A  R  R   R  R  R  A  A  A  A  A  A  A  -",
    "wino6s map tiles":      "A A A A  A  R  A  R  R  R  R  R  R  R  R  R  R  A  A   A  A  R  A  A  A  A  A  A  A  -",
    "wino6s RoI pairs":      "A A A A  A  R  A  R  R  R  R  R  R  R  R  R  R  R  R   R  R  R  A  A  A  A  A  A  A  -",
    "sp3 (sc 2)":            "A A A A  A  R  A  R  R  R  R  R  R  R  R  R  R  A  A   A  A  R  A  A  A  A  A  A  A  A",
    "sp3 (sc 21)":           "A A A A  A  R  A  R  R  R  R  R  R  R  R  R  R  A  A   A  A  R  A  A  A  A  A  A  A  A",
}
N_A = {("igemm 3x3 stride 2", "same_buffer"): "a stride-2 output has another height and width than its input: the two cannot be slices of one tensor"}
N_A.update({(f, "f16_domain"): "fp32 operands and bf16 pieces carry fp32's exponent: there is no window to leave" for f in FAMILIES if MATRIX[f].split()[-1] == "-"})
# value cells whose exact claim cannot hold, held to the emulation's bar instead (tests/conv_values.py), with the reason
HELD_TO_BAR = {(f, "ints"): "F(4x4) has thirds in G: U = G g G^T is rounded and the output cannot be exact" for f in FAMILIES if f.startswith("wino6")}
HELD_TO_BAR.update({(f, "pow2_channels"): "an fp16 piece of a scaled channel can go subnormal and lose bits: e_c in [-6, 6], and the output is near the plain launch's, not equal to it"
                    for f in ("pw split fp16 (wm 12)", "sp3 (sc 2)", "sp3 (sc 21)")})
VALUE_FEATURES = ("ints", "pow2_channels", "cancel", "sparse", "nonfinite", "f16_domain")

MULTI5 = [(2, 20, 36), (2, 9, 17), (2, 5, 3), (2, 3, 2), (2, 1, 1)]
GN3 = [(2, 20, 36), (2, 9, 17), (2, 5, 3)]       # the levels at which the Winograd forms' records hold their 1e-4 bar (one pixel per image has no variance to speak of)
GN_GROUPS = 10                                   # Cout 80: 8 channels per group


def declared(family, feature):
    """"accept" | "refuse" | None (a cell of N_A) from the MATRIX literal."""
    letters = MATRIX[family].split()
    assert len(letters) == len(FEATURES), (family, len(letters))
    return {"A": "accept", "R": "refuse", "-": None}[letters[FEATURES.index(feature)]]


def case(**kw):
    c = dict(id="", family="", feature="census", k=3, stride=1, shapes=[(2, 19, 37)], cin=48, cout=80, tv=(1, 16, 3), tail_tiles=0,
             x_view=None, y_view=None, same_buffer=False, relu_upto=None, in_relu=False, in_affine=False, res_mode=0, res_view=None,
             per_problem=False, weight_sets=1, gn_groups=0, pool=False, zero_shift=False, regime=None, answer="accept")
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    c["shapes"] = [tuple(s) for s in c["shapes"]]
    return c


def out_hw(c, h, w):
    return (h, w) if c["stride"] == 1 else ((h - 1) // 2 + 1, (w - 1) // 2 + 1)


def family_of(c):
    """The family of the matrix a case's variant and problem belong to (census rows are filed by it too)."""
    wm, sc, wn = c["tv"][:3]
    if wm in (1, 2):
        return "igemm 1x1" if c["k"] == 1 else "igemm 3x3 stride {}".format(c["stride"])
    if wm == 6:
        return "wino6{} {}".format({16: "", 32: "p", 64: "s"}[sc], "map tiles" if wn == 1 else "RoI pairs")
    if wm == 11:
        return "sp3 (sc {})".format(sc)
    return {7: "gather (wm 7)", 8: "pw (wm 8)", 9: "pw gather (wm 9)", 10: "pw split bf16 (wm 10)", 12: "pw split fp16 (wm 12)", 5: "wino4r (wm 5)"}[wm]


def _feature_row(family, feature):
    """The case of one cell: the family's plain problem with the one feature put on.  Feature rows write into a channel slice of a wider
    tensor (census rows write a dense one)."""
    base = dict(FAMILIES[family])
    cout, cin = base["cout"], base["cin"]
    roi = "RoI" in family
    one_by_one = base["k"] == 1
    c = dict(base, family=family, feature=feature, y_view=(cout + 24, 16))
    tv = tuple(base["tv"])
    aff_shapes = [(2, 16, 16)] if one_by_one else base["shapes"]       # the fused affine of a 1x1 conv needs H*W % 256 == 0
    if feature == "x_view":
        c.update(x_view=(cin + 32, 16))
    elif feature == "y_view":
        c.update(y_view=(cout + 20, 8))
    elif feature == "same_buffer":
        c.update(same_buffer=True, y_view=None)
    elif feature == "relu_partial":
        c.update(relu_upto=cout - 37)                                  # 43 | 188: inside a 32-cout tile, and not its first
    elif feature == "relu_zero":
        c.update(relu_upto=0)
    elif feature == "in_relu":
        c.update(in_relu=True)
    elif feature == "in_affine":
        c.update(in_affine=True, shapes=aff_shapes)
    elif feature == "res_same":
        c.update(res_mode=1, res_view=(cout + 16, 8))
    elif feature in ("res_up_odd_h", "res_up_odd_w"):
        n, h, w = base["shapes"][0]
        if roi:
            h, w = 13, 14
        h |= 1                                                         # the upsampled residual is cropped: (H + 1) / 2 rows cover an odd H
        w = (w | 1) if feature == "res_up_odd_w" else (w + (w & 1))
        if base["stride"] == 2:                                        # the residual has the OUTPUT's size: make that odd / even
            h, w = 2 * h - 1, 2 * w - 1
        c.update(res_mode=2, res_view=(cout + 16, 8), shapes=[(n, h, w)])
    elif feature in ("splitk2", "splitk4", "splitk8", "splitk_view_relu", "splitk_res", "splitk_in_affine"):
        sk = {"splitk2": 2, "splitk4": 4, "splitk8": 8}.get(feature, 2)
        c.update(tv=tv + (sk,), cin=32 * sk)                           # K chunks % (2 * splitk) == 0 in every family that splits K
        if feature == "splitk_view_relu":
            c.update(y_view=(cout + 20, 8), relu_upto=cout - 37)
        elif feature == "splitk_res":
            c.update(res_mode=1, res_view=(cout + 16, 8))
        elif feature == "splitk_in_affine":
            c.update(in_affine=True, shapes=aff_shapes)
    elif feature == "tail_splitk":
        c.update(tv=tv + (1, 2), tail_tiles=1)
    elif feature == "multi5":
        c.update(shapes=MULTI5, per_problem=True)
    elif feature == "multi10_two_weights":
        c.update(shapes=MULTI5 + MULTI5, per_problem=True, weight_sets=2)
    elif feature in ("gn", "gn_in_affine"):
        shapes = MULTI5 if family.startswith("sp3") else GN3
        if roi:
            shapes = base["shapes"]
        elif one_by_one:
            shapes = [(2, 16, 16)]
        elif base["stride"] == 2 or family in ("gather (wm 7)", "pw gather (wm 9)"):
            shapes = base["shapes"]                                    # (they refuse either way; one problem keeps the refusal about the records)
        c.update(gn_groups=GN_GROUPS if cout == 80 else 15, relu_upto=0, shapes=shapes, per_problem=len(shapes) > 1, in_affine=feature == "gn_in_affine")
    elif feature == "pool":
        c.update(pool=True)
    elif feature == "odd_n":
        n, h, w = base["shapes"][0]
        c.update(shapes=[(3, h, w)])
    elif feature == "n1":
        n, h, w = base["shapes"][0]
        c.update(shapes=[(1, h, w)])
    elif feature in VALUE_FEATURES:
        c.update(regime=feature, y_view=None, relu_upto=None if feature == "sparse" else 0)
        if feature == "nonfinite":
            c.update(pool=declared(family, "pool") == "accept")                # the pair of launches with the records on
    else:
        raise KeyError(feature)
    return case(answer=declared(family, feature), **c)


def _census_rows():
    """At least one accepted case per kernel instantiation, with the plainest features that reach it: scale and shift set (tune_wm 11: a
    zero shift, see zero_shift), relu_upto = Cout, dense views."""
    rows = []
    wn_cout = {1: 20, 2: 40, 3: 80, 4: 100, 5: 150, 6: 170, 7: 200}      # Cout <= 224: the padded Cout is a multiple of 32 * wn, the last tile masked
    for wn, cout in wn_cout.items():
        rows.append(case(k=1, shapes=[(2, 13, 19)], cout=cout, tv=(1, 32, wn)))
        rows.append(case(k=3, stride=2, shapes=[(2, 21, 35)], cout=cout, tv=(1, 16, wn)))
        for sc in (16, 32):
            rows.append(case(k=3, shapes=[(2, 19, 37)], cout=cout, tv=(1, sc, wn)))
            if wn <= 4:
                rows.append(case(k=3, shapes=[(2, 19, 37)], cout=cout, tv=(2, sc, wn)))
        if wn <= 4:
            rows.append(case(k=1, shapes=[(2, 13, 19)], cout=cout, tv=(2, 32, wn)))
    for wn, cout in ((1, 80), (2, 40), (4, 100)):                        # the gather form: Cout tiles % wn == 0
        rows.append(case(k=3, shapes=[(2, 13, 19)], cout=cout, tv=(7, 32, wn)))
    rows.append(case(k=3, stride=2, shapes=[(2, 21, 35)], cout=225, tv=(7, 32, 4)))      # ... at stride 2, the 128-cout padding
    for mt in (4, 2):                                                    # conv_pw_kernel<MT, POOL, GA, UPRES, SPLITK, SPLIT>
        pw = dict(k=1, shapes=[(2, 13, 19)], cin=96, cout=225)
        rows.append(case(tv=(8, 32, mt), **pw))
        rows.append(case(tv=(8, 32, mt), pool=True, **pw))
        rows.append(case(tv=(8, 32, mt), res_mode=2, **dict(pw, shapes=[(2, 13, 20)])))
        rows.append(case(tv=(8, 32, mt, 2), **dict(pw, cin=64, cout=288)))
        rows.append(case(tv=(9, 32, mt), **dict(pw, k=3)))
        rows.append(case(tv=(9, 32, mt), **dict(pw, k=3, stride=2, shapes=[(2, 21, 35)], cout=100)))
        rows.append(case(tv=(9, 32, mt, 2), **dict(pw, k=3, cin=64)))
    for form in (10, 12):
        pw = dict(k=1, shapes=[(2, 13, 19)], cin=96, cout=225, tv=(form, 32, 4))
        rows.append(case(**pw))
        rows.append(case(pool=True, **pw))
        rows.append(case(res_mode=2, **dict(pw, shapes=[(2, 13, 20)])))
        rows.append(case(**dict(pw, k=3)))
        rows.append(case(**dict(pw, k=3, stride=2, shapes=[(2, 21, 35)], cout=100)))
    for aff in (False, True):
        rows.append(case(shapes=[(2, 13, 41)], tv=(5, 16, 2), in_affine=aff))
        for sc in (16, 32, 64):
            rows.append(case(shapes=[(2, 13, 41)], tv=(6, sc, 1), in_affine=aff))
            rows.append(case(shapes=[(3, 14, 14)], tv=(6, sc, 2), in_affine=aff))
            rows.append(case(shapes=[(2, 7, 7)], cout=170, tv=(6, sc, 2), in_affine=aff))
        for geo in range(4):
            rows.append(case(tv=(11, 2, geo), cout=150, in_affine=aff, zero_shift=True))           # two cout tiles per wave
            rows.append(case(tv=(11, 21, geo), cout=150, in_affine=aff, zero_shift=True))          # one
        rows.append(case(tv=(11, 2, 0), cout=40, in_affine=aff, zero_shift=True))                  # geometry 0 up to 64 couts: one tile per wave by itself
    for i, c in enumerate(rows):
        c["family"] = family_of(c)
        if c["in_affine"] and c["k"] == 1:
            c["shapes"] = [(2, 16, 16)]
        if c["res_mode"]:
            c["res_view"] = (c["cout"], 0)
    return rows


def _extra_rows():
    """Feature rows beyond the one per cell: the five-level launch on direct tilings other than the cell's (the FCOS predictors run on
    whichever the tuner picked)."""
    rows = []
    for k, stride, tv, cout in ((3, 1, (2, 32, 2), 40), (3, 1, (1, 32, 5), 150), (3, 1, (2, 16, 4), 100), (3, 1, (1, 16, 1), 20),
                                (3, 2, (1, 16, 2), 40), (3, 2, (1, 16, 7), 200), (1, 1, (2, 32, 4), 100), (1, 1, (1, 32, 1), 20)):
        c = case(k=k, stride=stride, tv=tv, cout=cout, shapes=MULTI5, per_problem=True, feature="multi5", y_view=(cout + 24, 16), relu_upto=cout - 13)
        rows.append(dict(c, family=family_of(c)))
    return rows


def _value_rows():
    """The cells of the value features (after every other row: a row's index seeds its tensors, and those of the older rows stay), then
    nonfinite once more per family on a launch whose images share something."""
    rows = [_feature_row(family, feature) for family in FAMILIES for feature in VALUE_FEATURES if declared(family, feature) is not None]
    # nonfinite on the launches that share something between images or problems: the GroupNorm records where the family takes them (those
    # rows are multi-problem launches already), else the five-level launch where it takes that
    for family in FAMILIES:
        with_records = "gn" if declared(family, "gn") == "accept" else "multi5" if declared(family, "multi5") == "accept" else None
        if with_records:
            rows.append(dict(_feature_row(family, with_records), feature="nonfinite", regime="nonfinite", y_view=None, relu_upto=0))
    return rows


def all_cases():
    rows = _census_rows()
    for family in FAMILIES:
        for feature in FEATURES:
            if declared(family, feature) is not None and feature not in VALUE_FEATURES:
                rows.append(_feature_row(family, feature))
    rows += _extra_rows() + _value_rows()
    seen = {}
    for c in rows:
        name = "{} | {} | k{}s{} {} cin{} cout{} tv{}".format(c["family"], c["feature"], c["k"], c["stride"], "+".join("{}x{}x{}".format(*s) for s in c["shapes"][:1]) +
                                                            ("(x{})".format(len(c["shapes"])) if len(c["shapes"]) > 1 else ""), c["cin"], c["cout"], "-".join(str(v) for v in c["tv"]))
        if c["in_affine"] and c["feature"] == "census":
            name += " aff"
        if c["pool"] and c["feature"] == "census":
            name += " pool"
        if c["res_mode"] and c["feature"] == "census":
            name += " res{}".format(c["res_mode"])
        seen[name] = seen.get(name, 0) + 1
        c["id"] = name if seen[name] == 1 else "{} #{}".format(name, seen[name])
    return rows


# ---------------------------------------------------------------------------------------------------------------
# descriptors
# ---------------------------------------------------------------------------------------------------------------
def views_of(c):
    """((x_cs, x_co), (y_cs, y_co)) of a case; same_buffer: [x | 16 spare | y | 4 spare] in one tensor."""
    if c["same_buffer"]:
        cs = c["cin"] + 16 + c["cout"] + 4
        cs += -cs % 4
        return (cs, 0), (cs, c["cin"] + 16)
    return c["x_view"] or (c["cin"], 0), c["y_view"] or (c["cout"], 0)


def res_shape(c, n, h, w):
    """(N, Hr, Wr, res_cs) of the residual of a problem: the output's size (res_mode 1) or half of it, rounded up (res_mode 2)."""
    ho, wo = out_hw(c, h, w)
    cs = (c["res_view"] or (c["cout"], 0))[0]
    return (n, ho, wo, cs) if c["res_mode"] == 1 else (n, (ho + 1) // 2, (wo + 1) // 2, cs)


def fill_descs(c, _lib, ptr=None, bufs=None, ops=None):
    """The ConvDesc array of a case.  With ptr: every pointer is that dummy aligned address (cmk_conv_plan never follows one), every packing
    on offer, as tests/test_cpu_conv_plan.py::_descs fills them.  With bufs (device_buffers below) and ops: the real tensors through
    ops._fill_desc and ops._set_variant, as the wrappers of ops.py do; returns (descs, keep) with keep the workspaces to hold until the launch
    (keep["ws"]: split-K or tail slabs, keep["pool"], keep["gn"]: the NaN-filled workspace of a case whose records are refused)."""
    n = len(c["shapes"])
    descs = (_lib.ConvDesc * n)()
    relu_upto = c["cout"] if c["relu_upto"] is None else c["relu_upto"]
    if bufs is None:
        (x_cs, x_co), (y_cs, y_co) = views_of(c)
        for i, (d, (N, H, W)) in enumerate(zip(descs, c["shapes"])):
            d.x = d.scale = d.shift = d.y = ptr
            d.w = d.w_wino = d.w_wino6 = d.w_split = d.w_splith = ptr + 64 * weight_set(c, i)       # another weight set: another address
            d.w_splith_scale = 1.0
            d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = N, H, W, c["cin"], c["cout"], c["k"], c["stride"]
            d.x_cs, d.x_co, d.y_cs, d.y_co = x_cs, x_co, y_cs, y_co
            d.relu_upto, d.in_relu = relu_upto, int(c["in_relu"])
            d.res_mode = c["res_mode"]
            if c["res_mode"]:
                _, d.Hr, d.Wr, d.res_cs = res_shape(c, N, H, W)
                d.res, d.res_co = ptr, (c["res_view"] or (0, 0))[1]
            if c["in_affine"]:
                d.in_scale = d.in_shift = ptr
            d.tune_wm, d.tune_sc, d.tune_wn = c["tv"][:3]
            d.gn_groups, d.gn_ws = c["gn_groups"], (ptr if c["gn_groups"] else None)
        from centermask2_amd.ops import Variant
        d = descs[0]
        v = Variant.of(c["tv"])
        if v.splitk > 1:
            d.splitk, d.splitk_ws = v.splitk, ptr
        if v.tail:
            d.splitk_tail, d.splitk_ws, d.splitk_tail_tiles = v.tail, ptr, c["tail_tiles"]
        if c["pool"]:
            d.pool_ws = ptr
        return descs
    import torch
    View = ops.View
    for i in range(n):
        res = View(bufs["res"][i], c["res_view"][1] if c["res_view"] else 0, c["cout"]) if c["res_mode"] else None
        ops._fill_desc(descs[i], bufs["xv"][i], bufs["pcs"][i], bufs["yv"][i], False, relu_upto, res, c["res_mode"] == 2, c["in_relu"],
                       bufs["aff"][i] if c["in_affine"] else None)
    ws = ops._set_variant(descs, n, c["tv"], c["tail_tiles"])
    keep = {"ws": ws, "pool": None, "gn": None, "affine": None}
    if ws is not None:
        ws.fill_(float("nan"))            # a slab the kernel leaves unwritten and the reduce reads shows in the output; a refusal leaves all of it
    d = descs[0]
    dev = bufs["yv"][0].t.device
    if c["pool"]:
        rows = _lib.load().cmk_conv_pool_rows(ctypes.byref(d)) or 128
        N, H, W = c["shapes"][0]
        keep["rows"] = rows
        keep["pool"] = torch.full((2 * (-(-(N * H * W) // rows)), c["cout"]), float("nan"), device=dev)
        d.pool_ws = keep["pool"].data_ptr()
    if c["gn_groups"]:
        if c["answer"] == "accept":
            keep["affine"] = ops._gn_records(descs, bufs["yv"], c["gn_groups"])
        if keep["affine"] is None:        # a kernel without records (or a refusal ahead): hand in a workspace all the same
            keep["gn"] = torch.full((4096,), float("nan"), dtype=torch.float64, device=dev)
            for i in range(n):
                descs[i].gn_groups, descs[i].gn_ws = c["gn_groups"], keep["gn"].data_ptr()
    return descs, keep


# ---------------------------------------------------------------------------------------------------------------
# tensors and the float64 reference
# ---------------------------------------------------------------------------------------------------------------
def host_tensors(c, seed=0):
    """Seeded finite fp32 inputs of a case on the CPU: per problem x (N, H, W, x_cs), scale, shift, the input affine (N, Cin) x 2 and the
    residual (N, Hr, Wr, res_cs); per weight set the filter bank (Cout, Cin, k, k) and the GroupNorm (gamma, beta) that would follow."""
    import torch
    g = torch.Generator().manual_seed(1000 + seed)
    cin, cout, k = c["cin"], c["cout"], c["k"]
    (x_cs, _), _ = views_of(c)
    rnd = lambda *s: torch.randn(s, generator=g)
    t = {"x": [], "scale": [], "shift": [], "aff": [], "res": [], "w": [], "gn": []}
    for _ in range(c["weight_sets"]):
        t["w"].append(rnd(cout, cin, k, k) * (2.0 / (cin * k * k)) ** 0.5)
        t["gn"].append((torch.rand((cout,), generator=g) + 0.5, rnd(cout) * 0.1))
    scale, shift = torch.rand((cout,), generator=g) + 0.5, rnd(cout) * 0.1
    for i, (n, h, w) in enumerate(c["shapes"]):
        t["x"].append(rnd(n, h, w, x_cs))
        if c["per_problem"] and i > 0:
            scale, shift = torch.rand((cout,), generator=g) + 0.5, rnd(cout) * 0.1
        t["scale"].append(scale)
        t["shift"].append(torch.zeros(cout) if c["zero_shift"] else shift)
        t["aff"].append((torch.rand((n, cin), generator=g) + 0.5, rnd(n, cin) * 0.2) if c["in_affine"] else None)
        t["res"].append(rnd(*res_shape(c, n, h, w)) if c["res_mode"] else None)
    return t


def weight_set(c, i):
    return 0 if c["weight_sets"] == 1 or i < len(c["shapes"]) // 2 else 1


def reference(c, t, eps=1e-5):
    """Float64 answers of a case from host_tensors: per problem the output (N, Ho, Wo, Cout) — F.conv2d on double inputs with the input
    affine and ReLU, scale and shift, the residual (nearest-2x upsampled and cropped for res_mode 2) and the partial ReLU all in double —
    and, for cases with records, the GroupNorm {scale, shift} (N, Cout) of that output and its pooled means (N, Cout)."""
    import torch
    import torch.nn.functional as F
    (_, x_co), _ = views_of(c)
    cin, cout = c["cin"], c["cout"]
    relu_upto = cout if c["relu_upto"] is None else c["relu_upto"]
    out = {"y": [], "gn": [], "pool": []}
    for i, (n, h, w) in enumerate(c["shapes"]):
        x = t["x"][i][..., x_co:x_co + cin].double().permute(0, 3, 1, 2)
        if c["in_affine"]:
            a_sc, a_sh = t["aff"][i]
            x = (x * a_sc.double()[:, :, None, None] + a_sh.double()[:, :, None, None]).relu()
        if c["in_relu"]:
            x = x.relu()
        y = F.conv2d(x, t["w"][weight_set(c, i)].double(), None, stride=c["stride"], padding=c["k"] // 2)
        y = y * t["scale"][i].double()[None, :, None, None] + t["shift"][i].double()[None, :, None, None]
        if c["res_mode"]:
            r_co = c["res_view"][1] if c["res_view"] else 0
            r = t["res"][i][..., r_co:r_co + cout].double().permute(0, 3, 1, 2)
            if c["res_mode"] == 2:
                r = F.interpolate(r, scale_factor=2, mode="nearest")[:, :, :y.shape[2], :y.shape[3]]
            y = y + r
        y[:, :relu_upto] = y[:, :relu_upto].relu()
        out["y"].append(y.permute(0, 2, 3, 1).contiguous())
        if c["gn_groups"]:
            groups = c["gn_groups"]
            gamma, beta = (v.double() for v in t["gn"][weight_set(c, i)])
            r = y.reshape(n, groups, -1)
            mean, var = r.mean(2), r.var(2, unbiased=False)
            sc = (1.0 / torch.sqrt(var + eps)).repeat_interleave(cout // groups, 1) * gamma[None]
            out["gn"].append((sc, beta[None] - mean.repeat_interleave(cout // groups, 1) * sc))
        if c["pool"]:
            out["pool"].append(y.mean(dim=(2, 3)))
    return out
