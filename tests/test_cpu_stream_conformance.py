"""The stream conformance table (tests/stream_cases.py) without a GPU: nothing is launched.  The kernels that the accepted rows name must
be exactly the __global__ kernels of csrc/elementwise.hip and csrc/groupnorm.hip as the built library instantiates them, every (entry point,
feature) cell must have a row or a reason, and every refused row must be refused on dummy aligned pointers: every argument check of these
entry points sits before its launch."""
import pytest

from tests import conformance as C
from tests import stream_cases as sc

CASES = sc.all_cases()


def test_census_equals_the_kernels_of_the_two_files(cmk_lib):
    """No count is written down: a new kernel or instantiation without a row, or a row naming a kernel that is gone, fails here by name."""
    C.assert_census(CASES, C.TABLES["tests/stream_cases.py"][1])


def test_every_cell_has_a_row_or_a_reason():
    C.assert_cells(CASES, sc)
    for c in CASES:
        assert bool(c["kernels"]) == (c["answer"] == "accept"), c["id"]
        assert set(sc.POINTERS[c["entry"]]) >= {c["null"]} - {None}, c["id"]


def test_the_restated_groupnorm_shape_rule_splits_the_grid_both_ways():
    """The C x groups grid of the GroupNorm entry points is sorted into accepted and refused rows by stream_cases.gn_shape_ok; both kinds
    exist, so the refusal test below and the GPU module check that restatement against the library's rule in both directions."""
    for e in (sc.GN_RELU, sc.GN, sc.AFFINE):
        grid = [c for c in CASES if c["entry"] == e and c["why"].startswith("C ") and " groups, H*W " in c["why"]]
        assert {c["answer"] for c in grid} == {"accept", "refuse"}
        assert {(c["c"], c["groups"]) for c in grid if c["answer"] == "accept"} >= {(4, 1), (16, 4), (64, 16), (256, 64), (1024, 64), (1024, 1)}


@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_refused_rows_are_refused_before_any_launch(cmk_lib, entry):
    C.assert_refused_before_launch(cmk_lib, sc, entry)                    # any non-zero code: this table names none
