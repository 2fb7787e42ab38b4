"""The visualizer conformance table (tests/vis_cases.py) without a GPU: nothing is launched.  The kernels that the accepted rows name must
be exactly the __global__ kernels of csrc/visualize.hip as the built library holds them, every (entry, feature) cell must have a row or a
reason, the geometry a row exists for must be what the restated launch code makes of its arguments, no accepted row may grow into a
workload, the three size functions must be their restatements, and every refused row must be refused with CMK_EINVAL on dummy aligned
pointers: every argument check of these entries sits before its launch.  And the references the GPU module leans on, against each other:
the built checkerboard expectation against the edge follower, the record restatement against the renderer's own label and plate."""
import numpy as np
import pytest

from tests import conformance as C
from tests import contour_ref as CR
from tests import vis_cases as vc
from tests import visualize_ref as VR

CASES = vc.all_cases()
ACCEPTED = [c for c in CASES if c["answer"] == "accept"]
ROW_KEYS = {"id", "entry", "feature", "answer", "why", "data", "null", "host_only", "wrapper", "expect", "kernels"}


def test_census_equals_the_kernels_of_visualize_hip(cmk_lib):
    """No count is written down: a kernel added to visualize.hip without a row, or a row naming a kernel that is gone, fails by name."""
    C.assert_census(CASES, ("visualize.hip",))
    assert C.TABLES["tests/vis_cases.py"] == (vc, ("visualize.hip",))
    for e in vc.ENTRIES:
        assert all(hasattr(cmk_lib, name) for name in e.split("+")), e
    wrappers = [c for c in CASES if c["wrapper"]]
    assert hasattr(cmk_lib, vc.WRAPPER) and len(wrappers) == 1 and wrappers[0]["feature"] == "census" and wrappers[0]["entry"] == vc.PREP and not wrappers[0]["ids"]


def test_every_cell_has_a_row_or_a_reason():
    C.assert_cells(CASES, vc, nullable=vc.NULLABLE)
    assert all(isinstance(v, str) and v.strip() for v in vc.NO_ROW.values())
    for c in CASES:
        assert c["why"].strip(), c["id"]
        if c["answer"] == "accept" and not c["kernels"]:                 # accepted and launching nothing: a count of zero
            assert min(c.get(k, 1) for k in ("r", "n", "rows")) == 0 and "touches nothing" in c["why"], c["id"]
        assert c["null"] is None or c["null"] in vc.POINTERS[c["entry"]], c["id"]
        assert set(c) - ROW_KEYS == set(vc.DEFAULTS[c["entry"]]), c["id"]
    for e in vc.ENTRIES:
        assert set(vc.NULLABLE[e]) <= set(vc.POINTERS[e])
    both = {c["null"] for c in CASES if c["entry"] == vc.CONT and c["null"] and c["phase"] == "count"}
    assert both == set(vc.COUNT_PHASE)                                   # the pair: each phase refuses its own pointers
    # every out-of-place pair overlaps identically and partially
    for e, pairs in ((vc.ASSIGN, [("out_" + a, "old_" + a) for a in vc.TABLE_ARRAYS]),
                     (vc.GATHER, [("out_words", "old_words"), ("out_words", "new_words"), ("out_areas", "old_areas")])):
        for o, i in pairs:
            shifts = {c["overlap"][2] for c in CASES if c["entry"] == e and c["overlap"] and c["overlap"][:2] == (o, i)}
            assert 0 in shifts and shifts - {0}, (e, o, i, shifts)
    assert {c["overlap"] for c in CASES if c["entry"] == vc.COMP and c["overlap"]} == {-1, 1}
    cont = {(c["phase"],) + c["overlap"] for c in CASES if c["entry"] == vc.CONT and c["overlap"]}
    pairs = {v[:3] for v in cont}
    assert all(p + (0,) in cont and p + (1,) in cont for p in pairs)
    assert len(pairs) == 3 + 3 * 2 + 3                                   # count: its three buffers pairwise; trace: three outputs x two inputs, and pairwise
    for c in CASES:                                                      # a partial overlap is one: the shifted pointer lies inside the other buffer
        if c["entry"] == vc.CONT and c["overlap"]:
            t = sum(vc.host_corners(c))
            size = {"words": 8 * c["r"] * vc.nwords(c["h"], c["w"]), "ws": vc.contour_ws_bytes(c["r"], c["h"], c["w"]), "xy": 8 * t, "head": 4 * t}[c["overlap"][1]]
            assert 0 <= 16 * c["overlap"][2] < size, c["id"]
        if c["entry"] in (vc.ASSIGN, vc.GATHER) and c["overlap"]:
            assert -c["cap"] < c["overlap"][2] < (c["n"] if c["overlap"][1].startswith("new") else c["cap"]), c["id"]
    # a refusal behind T > 0 needs a non-zero even host array
    row = next(c for c in CASES if c["entry"] == vc.CONT and c["null"] == "scratch")
    assert sum(vc.host_corners(row)) > 0 and all(v % 2 == 0 for v in vc.host_corners(row))


def test_the_restated_geometry_is_what_the_rows_say():
    """A row exists for a branch; `expect` names the restated quantity that takes it.  The words of `why` and the numbers must agree."""
    for c in ACCEPTED:
        g = vc.geometry(c)
        for k, v in c["expect"].items():
            assert k in g and g[k] == v, (c["id"], k, "the row says", v, "the restated launch code says", g.get(k))
    say = {"the scalar path": ("vec", 0), "the vector path": ("vec", 1), "17 link trips": ("link_trips", 17), "nb = 1027": ("nb", 1027),
           "21 jump rounds": ("jump_rounds", 21), "R * NB = 1025": ("offsets_trips", 2), "R * NB = 1026": ("offsets_trips", 2), "a third round": ("rounds", 3),
           "the second round": ("rounds", 2), "one full round": ("rounds", 1), "65568 words": ("nw", 65568), "nw = 257": ("nw", 257)}
    said = set()
    for c in ACCEPTED:
        g = vc.geometry(c)
        for words, (k, v) in say.items():
            if words in c["why"] and k in g:
                assert g[k] == v, (c["id"], "says '{}' but the restated {} is {}".format(words, k, g[k]))
                said.add(words)
        if c["feature"] == "second_trip":
            assert max(g.get(k, 0) for k in ("trips", "rounds", "offsets_trips", "blocks_trips")) >= 2, (c["id"], g)
        elif "trips" in g:
            assert g["trips"] == 1, c["id"]
    assert said == set(say), sorted(set(say) - said)
    by = lambda e: [(c, vc.geometry(c)) for c in ACCEPTED if c["entry"] == e]
    assert {c["n"] for c, _ in by(vc.PREP)} >= {0, 1, 63, 64, 65, 130}
    comp = by(vc.COMP)
    assert {c["h"] * c["w"] for c, _ in comp} >= {15, 64, 65, 37 * 70, 16 * 64, 40 * 129} and {c["n"] for c, _ in comp} >= {0, 1, 64, 65, 129}
    assert {(c["in_off"], c["out_off"]) for c, _ in comp} >= {(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (4, 4)}
    assert {c["alpha256"] for c, _ in comp} == {0, 128, 256} and {c["line_width"] for c, _ in comp} >= {1, 16} and {c["font_scale"] for c, _ in comp} >= {1, 16}
    assert {(c["k"], c["s"]) for c, _ in by(vc.KP)} >= {(1, 0), (3, 4), (17, 19)}
    assert {g["pairs"] for _, g in by(vc.IOU)} >= {1, 255, 256, 257}
    assert {(c["n"], c["rows"], c["cap"]) for c, _ in by(vc.ASSIGN)} >= set(vc.ASSIGN_SHAPES)
    assert max(g["row_trips"] for _, g in by(vc.ASSIGN)) == 64 and max(g["lane_trips"] for _, g in by(vc.ASSIGN)) == 16
    assert {g["nw"] for _, g in by(vc.GATHER)} >= {1, 256, 257, 65568} and max(g["trips"] for _, g in by(vc.GATHER)) == 2
    cont = by(vc.CONT)
    assert {(c["h"], c["w"]) for c, _ in cont} >= set(vc.AWKWARD) and {c["h"] for c, _ in cont if c["data"] == "columns"} == {63, 64, 65, 128, 129}
    assert {c["r"] * g["NB"] for c, g in cont} >= {1025, 1026}
    # 725 is the smallest side of a checkerboard with T > 2^20; 724 stays at nb = 1024
    assert all(vc.checker_corners(725, p) > 1 << 20 for p in (0, 1)) and {vc.checker_corners(725, p) for p in (0, 1)} == {1051252, 1051248}
    assert all(vc.checker_corners(724, p) <= 1 << 20 for p in (0, 1)) and vc.cdiv(vc.checker_corners(724, 0), 1024) == 1024


def test_no_row_grows_into_a_workload():
    big = []
    for c in ACCEPTED:
        b = vc.largest_buffer(c)
        assert b <= vc.MAX_BYTES, (c["id"], b)
        if b > vc.BIG_BYTES:
            big.append(c["id"])
    assert len(big) == 1 and "checker" in big[0], big
    for c in ACCEPTED:
        if c["entry"] in (vc.ASSIGN, vc.GATHER):                     # an accepted row is inside the header's bounds: the tables hold cap rows
            assert 1 <= c["cap"] <= 1024 and 0 <= c["n"] <= c["cap"] and 0 <= c["rows"] <= c["cap"], c["id"]
        if c["entry"] == vc.IOU:
            assert 0 <= c["n"] <= 1024 and 0 <= c["rows"] <= 1024, c["id"]
        if c["entry"] == vc.KP:
            assert c["n"] * (c["s"] + c["k"]) <= 200, (c["id"], "the reference paints every primitive")


def test_the_size_functions(cmk_lib):
    assert cmk_lib.cmk_vis_record_ints() == vc.REC_INTS == VR.REC_INTS and VR.REC_INTS % 4 == 0
    for r, h, w in [(1, 1, 1), (5, 13, 67), (1, 1024, 1), (513, 1024, 1), (1025, 1, 1), (1, 725, 725), (0, 5, 3), (65535, 63, 64), (3, 64, 63), (2, 1023, 62)]:
        assert cmk_lib.cmk_vis_contour_ws_bytes(r, h, w) == vc.contour_ws_bytes(r, h, w), (r, h, w)
    for r, h, w in [(-1, 5, 3), (65536, 5, 3), (1, 0, 3), (1, 3, 0), (1, -1, 3), (1, vc.TOO_BIG, vc.TOO_BIG)]:
        assert cmk_lib.cmk_vis_contour_ws_bytes(r, h, w) == 0, (r, h, w)
    for t in (1, 2, 1023, 1024, 1025, 1 << 20, 1051252, vc.INT32_MAX):
        assert cmk_lib.cmk_vis_contour_trace_ws_bytes(t) == vc.trace_ws_bytes(t), t
    assert vc.trace_ws_bytes(1051252) == 50464204
    for t in (0, -1, vc.INT32_MIN):
        assert cmk_lib.cmk_vis_contour_trace_ws_bytes(t) == 0, t


@pytest.mark.parametrize("entry", vc.ENTRIES)
def test_refused_rows_are_refused_before_any_launch(cmk_lib, entry):
    C.assert_refused_before_launch(cmk_lib, vc, entry, einval=vc.CMK_EINVAL)


def test_overlapping_pairs_are_refused_when_every_other_pointer_is_apart(cmk_lib):
    """On dummy pointers every pair of a call is one address, so the refusal of an overlap row may be another pair's.  Here every pointer
    has a host buffer of its own (nothing is read through them before the launch) and only the row's pair overlaps: CMK_EINVAL must
    come from that pair.  A pointer comparison in place of a range test lets the shifted rows through to the launch."""
    import ctypes
    rows = [c for c in CASES if c.get("overlap") and not c["host_only"]]
    assert {c["entry"] for c in rows} == {vc.COMP, vc.ASSIGN, vc.GATHER, vc.CONT}
    for c in rows:
        bufs = {k: (ctypes.c_char * 8192)() for k in vc.POINTERS[c["entry"]] if k not in vc.HOST_ARRAYS}
        p = {k: (ctypes.addressof(b) + 2048 + 63) // 64 * 64 for k, b in bufs.items()}
        rc = vc.call(cmk_lib, c, p)
        assert rc == vc.CMK_EINVAL and cmk_lib.cmk_last_error().decode().strip(), (c["id"], rc, cmk_lib.cmk_last_error().decode())
        assert "overlap" in cmk_lib.cmk_last_error().decode(), (c["id"], cmk_lib.cmk_last_error().decode())


# ---------------------------------------------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [5, 6])
@pytest.mark.parametrize("parity", [0, 1])
def test_the_built_checkerboard_is_what_the_edge_follower_traces(side, parity):
    """The expectation of the 725 x 725 row is built (contour_ref.unit_squares), not traced: here it is held to the edge follower."""
    mask = CR.checkerboard(side, parity)
    want = CR.contours(mask)
    assert CR.as_lists(CR.unit_squares(mask)) == want and 4 * len(want) == vc.checker_corners(side, parity)
    assert mask[0, 0] == (parity == 0)


def test_records_against_the_renderer_and_by_hand():
    """records() and render() state the label, the plate and the colours independently; on well-formed inputs they must agree, and three
    fields are pinned by hand."""
    names = ["cat", "", "a" * 40]
    glyphs = np.zeros((3, 32), dtype=np.uint8)
    for i, s in enumerate(names):
        g = VR.glyph_indices(s.upper())[:32]
        glyphs[i, :len(g)] = g
    lens = np.array([3, 0, 40], dtype=np.int32)
    pal = np.array(VR.PALETTE_RGB, dtype=np.uint8)
    boxes = np.array([[2.5, 3.9, 30, 20], [60, 44, 70, 50], [-5, -7, 10, 10], [np.nan, 0, 5, 5]], dtype=np.float32)
    scores = np.array([0.995, 0.004999, 1e30, 0.5], dtype=np.float32)
    classes = np.array([0, 1, 2, vc.INT64_MIN], dtype=np.int64)
    recs = VR.records(boxes, scores, classes, [0, 1, 2, 3], glyphs, lens, pal, 48, 64, 1)
    r = recs[0]
    assert r[VR.R_BOX:VR.R_BOX + 4].tolist() == [2, 3, 30, 20] and r[VR.R_LEN] == 8 and r[VR.R_PLATE:VR.R_PLATE + 4].tolist() == [2, 3, 49, 9]      # "CAT 100%"
    assert r[VR.R_GLYPH:VR.R_GLYPH + 8].tobytes()[:8] == bytes(VR.glyph_indices("CAT 100%")) and r[VR.R_HIT:VR.R_HIT + 4].tolist() == [2, 3, 50, 20]
    assert recs[1][VR.R_LEN] == 3 and recs[1][VR.R_PLATE:VR.R_PLATE + 4].tolist() == [64 - 19, 48 - 9, 19, 9]                                        # " 0%"
    assert recs[2][VR.R_LEN] == 32 and recs[2][VR.R_PLATE:VR.R_PLATE + 2].tolist() == [0, 0]
    assert recs[3][VR.R_FLAGS] == 0 and recs[3][VR.R_GLYPH:VR.R_GLYPH + 8].tobytes()[:24] == bytes(VR.glyph_indices("C-9223372036854775808 50%"))[:24]
    assert recs[3][VR.R_LEN] == 25 and recs[3][VR.R_BOX:VR.R_BOX + 4].tolist() == [0, 0, -1, -1] == recs[3][VR.R_HIT:VR.R_HIT + 4].tolist()
    col = VR.colours(2, "RGB")
    assert recs[2][VR.R_COL] == col[0][0] | col[0][1] << 8 | col[0][2] << 16 and recs[2][VR.R_EDGE] == col[1][0] | col[1][1] << 8 | col[1][2] << 16
    assert recs[2][VR.R_TEXT] == col[2][0] | col[2][1] << 8 | col[2][2] << 16 and recs[2][18] == 0 and recs[2][19] == 0
    ids = VR.records(boxes, scores, classes, [7, -1, 2, 1 << 40], glyphs, lens, pal, 48, 64, 1, color_ids=[-1, vc.INT32_MIN, 65, 3])
    assert ids[:, VR.R_SRC].tolist() == [0, 1, 2, 3] and ids[0][VR.R_COL] == recs[0][VR.R_COL] * 0 + (int(pal[63][0]) | int(pal[63][1]) << 8 | int(pal[63][2]) << 16)
    assert ids[1][VR.R_COL] == recs[0][VR.R_COL] and ids[2][VR.R_COL] == recs[1][VR.R_COL]
