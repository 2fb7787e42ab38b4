"""The stream conformance table (tests/stream_cases.py) without a GPU: nothing is launched.  The kernels that the accepted rows name must
be exactly the __global__ kernels of csrc/elementwise.hip and csrc/groupnorm.hip as the built library instantiates them, every (entry point,
feature) cell must have a row or a reason, and every refused row must be refused on dummy aligned pointers: every argument check of these
entry points sits before its launch."""
import ctypes
import os
import re
import subprocess

import pytest

from tests import stream_cases as sc

CASES = sc.all_cases()
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centermask2_amd", "csrc")


def source_kernels():
    """The __global__ kernel names of the two files."""
    names = set()
    for f in ("elementwise.hip", "groupnorm.hip"):
        with open(os.path.join(CSRC, f)) as fh:
            names |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", fh.read()))
    return names


def library_kernels(names):
    """Their instantiations in the built library: the kernel handles `nm -C` prints as cmk::name[<args>](...)."""
    from centermask2_amd import _lib
    syms = subprocess.run(["nm", "-C", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    found = set()
    for line in syms.splitlines():
        m = re.search(r" cmk::(\w+(?:<[^>]*>)?)\(", line)
        if m and m.group(1).split("<")[0] in names:
            found.add(m.group(1))
    return found


def test_census_equals_the_kernels_of_the_two_files(cmk_lib):
    """No count is written down: a new kernel or instantiation without a row, or a row naming a kernel that is gone, fails here by name."""
    names = source_kernels()
    assert names, "no __global__ kernel found in the sources"
    kernels = library_kernels(names)
    assert {k.split("<")[0] for k in kernels} == names, "kernels of the sources the library lacks: {}".format(sorted(names - {k.split("<")[0] for k in kernels}))
    named = {k for c in CASES if c["answer"] == "accept" for k in c["kernels"]}
    assert named == kernels, "kernels no accepted row launches: {}; rows naming kernels the library lacks: {}".format(sorted(kernels - named), sorted(named - kernels))
    census = {k for c in CASES if c["feature"] == "census" for k in c["kernels"]}
    assert census == kernels, "kernels without a census row: {}".format(sorted(kernels - census))


def test_every_cell_has_a_row_or_a_reason():
    assert {c["entry"] for c in CASES} == set(sc.ENTRIES) and {c["feature"] for c in CASES} == set(sc.FEATURES)
    cells = {(c["entry"], c["feature"]) for c in CASES}
    for e in sc.ENTRIES:
        for f in sc.FEATURES:
            assert ((e, f) in cells) != ((e, f) in sc.N_A), (e, f, "a cell has a row or a reason, not both and not neither")
    assert all(isinstance(v, str) and v.strip() for v in sc.N_A.values())
    assert len({c["id"] for c in CASES}) == len(CASES)                   # ids name rows
    for c in CASES:
        assert c["answer"] in ("accept", "refuse") and (c["answer"] == "refuse") == (c["feature"] == "refuse"), c["id"]
        assert bool(c["kernels"]) == (c["answer"] == "accept"), c["id"]
        assert not c["host_only"] or c["answer"] == "refuse", c["id"]
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
    buf = (ctypes.c_float * 96)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    rows = [c for c in CASES if c["entry"] == entry and c["answer"] == "refuse"]
    assert rows
    for c in rows:
        rc = sc.call(cmk_lib, c, sc.dummy_pointers(c, ptr))
        assert rc != 0, (c["id"], "declared refuse, accepted")
        assert cmk_lib.cmk_last_error().decode().strip(), (c["id"], "refused without an error text")
