"""The variant-conv conformance table (tests/variant_cases.py) without a GPU: nothing is launched.  The kernels that the accepted rows name
must be exactly the __global__ kernels of csrc/conv_deform.hip, csrc/dwconv_bn_act.hip, csrc/conv_group3.hip and csrc/stem7_pool.hip as the
built library instantiates them, every (entry point, feature) cell must have a row or a reason, no accepted row may be out of proportion,
and every refused row must be refused with CMK_EINVAL on dummy aligned pointers: every argument check of these entry points sits before its
launch.  And the per-corner float64 restatement of the deformable conv (tests/deform_ref.py) equals the grid_sample one where both apply."""
import pytest
import torch

from tests import conformance as C
from tests import variant_cases as vc
from tests.deform_ref import deform_conv3x3_ref, deform_conv3x3_ref_corners, make_offsets

CASES = vc.all_cases()
MB = 1 << 20


def test_census_equals_the_kernels_of_the_four_files(cmk_lib):
    """No count is written down: a new kernel or instantiation without a row, or a row naming a kernel that is gone, fails here by name."""
    C.assert_census(CASES, C.TABLES["tests/variant_cases.py"][1])
    assert all(hasattr(cmk_lib, e) for e in vc.ENTRIES)


def test_every_cell_has_a_row_or_a_reason():
    C.assert_cells(CASES, vc, nullable=vc.POINTERS)
    assert set(vc.DEFAULTS) == set(vc.POINTERS) == set(vc.NULLABLE) == set(vc.ENTRIES)
    for c in CASES:
        assert bool(c["kernels"]) == (c["answer"] == "accept"), c["id"]
        assert c["null"] is None or c["null"] in vc.NULLABLE[c["entry"]], c["id"]
        assert c["why"].strip() or c["feature"] in ("n1", "odd_n", "offsets_edge", "offsets_far", "offsets_int", "poison"), (c["id"], "a row says which edge it puts")
        if c["same_buffer"] and c["answer"] == "accept":
            (x_cs, x_co), (y_cs, y_co) = c["x_view"], c["y_view"]
            xc = c["cin"] if c["entry"] == vc.DEFORM else c["c"]
            assert c["stride"] == 1 and x_cs == y_cs and (x_co + xc <= y_co or y_co + c["c"] <= x_co), (c["id"], "an accepted same_buffer row has disjoint slices")
    for e in vc.ENTRIES:                                                 # every pointer has its NULL row, every vector pointer its misaligned row
        nulled = {c["null"] for c in CASES if c["entry"] == e and c["null"]}
        assert nulled == set(vc.POINTERS[e]), (e, sorted(set(vc.POINTERS[e]) - nulled))
        off = {c["misalign"] for c in CASES if c["entry"] == e and c["misalign"]}
        assert off >= set(vc.ALIGN16[e]), (e, sorted(set(vc.ALIGN16[e]) - off))
    # the refusals of overlapping slices and of a count within one grid stride of 2^31
    for e in (vc.DWACT, vc.DW, vc.GROUP, vc.DEFORM):
        assert sum(c["same_buffer"] and c["answer"] == "refuse" for c in CASES if c["entry"] == e) >= 2, e
    for e in (vc.DWACT, vc.DW):
        quads = [c["n"] * vc.out_hw(c)[0] * vc.out_hw(c)[1] * (c["c"] // 4) for c in CASES if c["entry"] == e and c["host_only"]]
        assert any((1 << 31) - vc.DW_MAX_GRID_STRIDE < q < (1 << 31) for q in quads) and any(q >= (1 << 31) for q in quads), e


def test_kernels_of_names_every_rung_of_the_ladders_from_both_sides():
    """The restated choice of instantiation is pinned at its thresholds: per rung of the depth-wise ladder one accepted row of exactly 1024
    workgroups at that rung's tile, which runs that rung, and one of 1023, which runs a later rung; the deformable rows reach WN 1..7 and
    both ragged two-tile widths."""
    for stride, ladder in vc.DW_LADDER.items():
        rows = [c for c in CASES if c["entry"] == vc.DWACT and c["answer"] == "accept" and c["stride"] == stride]
        for i, (t, r) in enumerate(ladder[:-1]):
            name = "dwconv3_bn_act_kernel<{}, {}, {}, false>".format(stride, t, r)
            higher = ladder[:i]
            at = [c for c in rows if all(vc.dw_blocks(c, *hr) < 1024 for hr in higher)]
            above = [c for c in at if vc.dw_blocks(c, t, r) == 1024]
            below = [c for c in at if vc.dw_blocks(c, t, r) == 1023]
            assert above and all(c["kernels"] == [name] for c in above), (stride, t, r, "no row just above the threshold")
            assert below and all(c["kernels"] != [name] for c in below), (stride, t, r, "no row just below the threshold")
            for c in above + below:
                ho, wo = vc.out_hw(c)
                assert (r == 1 or ho % r) and (t == 1 or wo % t) and c["h"] % 2 == 1 and c["w"] % 2 == (1 if stride == 1 else 0), (c["id"], "ragged against the tile")
    deform = {c["c"]: c["kernels"][0] for c in CASES if c["entry"] == vc.DEFORM and c["answer"] == "accept"}
    assert {vc.deform_tiles(co) for co in deform} >= {(1, wn) for wn in range(1, 8)} | {(2, 4), (2, 5)}
    assert vc.deform_tiles(232) == (2, 4) and vc.deform_tiles(288) == (2, 5) and vc.deform_tiles(192) == (1, 6) and vc.deform_tiles(20) == (1, 1)
    assert vc.cout_pad(288) == 384 and vc.cout_pad(232) == 256 and vc.cout_pad(20) == 32


def test_the_rows_keep_the_limits_that_protect_the_machine():
    """No accepted row but the second_trip rows holds a buffer above 40 MB; a second_trip row stays below 300 MB and is the smallest count
    of whole images above what one launch covers.  Restated geometry only."""
    trips = []
    for c in CASES:
        if c["answer"] != "accept":
            continue
        largest = max(vc.buffers(c).values()) * 4
        ho, wo = vc.out_hw(c)
        assert c["n"] >= 1 and ho >= 1 and wo >= 1, c["id"]
        if c["feature"] != "second_trip":
            assert largest <= 40 * MB, (c["id"], largest)
            continue
        trips.append((c["entry"], c["kernels"][0]))
        assert largest <= 300 * MB, (c["id"], largest)
        work, covered = vc.second_trip_threads(c)
        one_less, _ = vc.second_trip_threads(dict(c, n=c["n"] - 1))
        assert work > covered >= one_less, (c["id"], work, covered, "the smallest batch whose loop takes a second trip")
        assert c["h"] * c["w"] <= 64 and not c["x_view"] and not c["y_view"], (c["id"], "many images of a small dense map")
    assert sorted(trips) == sorted([(vc.DWACT, "dwconv3_bn_act_kernel<1, 2, 4, false>"), (vc.DW, "dwconv3_bn_act_kernel<1, 4, 1, true>"),
                                    (vc.GROUP, "group3_valu_kernel<4, 1, 2, 2>"), (vc.STEM7, "stem7_pool_kernel")])


@pytest.mark.parametrize("entry", vc.ENTRIES)
def test_refused_rows_are_refused_before_any_launch(cmk_lib, entry):
    C.assert_refused_before_launch(cmk_lib, vc, entry, einval=vc.CMK_EINVAL)


# ---------------------------------------------------------------------------------------------------------------
# the two float64 restatements of the deformable conv
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["frac", "int", "far", "edge", "zero"])
@pytest.mark.parametrize("dg,modulated", [(1, 0), (2, 1), (4, 1)])
def test_per_corner_restatement_equals_the_grid_sample_one(kind, dg, modulated):
    """For finite inputs on maps of H, W >= 2 the per-corner restatement (the arbiter of the table's poison rows, valid for H or W = 1 too)
    equals the grid_sample one of the direct tests to 1e-12 of max(1, max|ref|)."""
    for n, h, w in ((2, 7, 11), (1, 2, 2), (3, 5, 6)):
        g = torch.Generator().manual_seed(31 * dg + h)
        x = torch.randn((n, 16, h, w), generator=g)
        weight = torch.randn((12, 16, 3, 3), generator=g) / 12.0
        scale, shift = torch.rand((12,), generator=g) + 0.5, torch.randn((12,), generator=g) * 0.1
        off = make_offsets(kind, "randn", n, h, w, dg, modulated, seed=5)
        for relu in (False, True):
            a = deform_conv3x3_ref_corners(x, off, weight, dg, modulated, scale, shift, relu=relu)
            b = deform_conv3x3_ref(x, off, weight, dg, modulated, scale, shift, relu=relu)
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), (kind, dg, n, h, w)


def test_per_corner_restatement_follows_the_rule_of_the_header():
    """A sample outside (-1,H) x (-1,W) reads nothing, an out-of-map corner reads nothing, an in-map corner is read even at weight 0.  A 5x6
    map with an Inf at (0,0) and zero offsets: exactly the four pixels whose window holds (0,0) are non-finite; an Inf in the last row also
    reaches the pixels whose window holds the pixel above it (its corner of weight 0)."""
    x = torch.randn((1, 16, 5, 6), generator=torch.Generator().manual_seed(1))
    weight = torch.ones((4, 16, 3, 3))
    off = torch.zeros((1, 18, 5, 6))
    x[0, 3, 0, 0] = float("inf")
    bad = ~torch.isfinite(deform_conv3x3_ref_corners(x, off, weight, 1, 0))[0, 0]
    want = torch.zeros((5, 6), dtype=torch.bool)
    want[:2, :2] = True
    assert torch.equal(bad, want)
    x[0, 3, 0, 0] = 0.0
    x[0, 3, 4, 3] = float("inf")
    bad = ~torch.isfinite(deform_conv3x3_ref_corners(x, off, weight, 1, 0))[0, 0]
    want.zero_()
    want[2:, 1:5] = True          # the samples at (4,3), (4,2), (3,3) and (3,2) read it, the last three as a corner of weight 0
    assert torch.equal(bad, want)
    one = deform_conv3x3_ref_corners(torch.ones((1, 16, 1, 1)), torch.zeros((1, 18, 1, 1)), weight, 1, 0)       # a 1x1 map: the centre tap alone
    assert torch.equal(one, torch.full((1, 4, 1, 1), 16.0, dtype=torch.float64))
