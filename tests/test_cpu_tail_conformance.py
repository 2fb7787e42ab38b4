"""The tail conformance table (tests/tail_cases.py) without a GPU: nothing is launched.  The kernels that the accepted rows name must be
exactly the __global__ kernels of csrc/detect.hip, csrc/roi.hip, csrc/prepost.hip and csrc/keypoint.hip as the built library instantiates
them, every (entry point, feature) cell must have a row or a reason, and every refused row must be refused on dummy aligned pointers: every
argument check of these entry points sits before its launch.  And the library-wide census: every kernel of the built library is claimed by
exactly one of the six conformance tables (conv, stream, tail, image, variant, vis) or by a named direct test module."""
import glob
import os

import pytest

from tests import conformance as C
from tests import image_cases as ic
from tests import tail_cases as tc

CASES = tc.all_cases()
TESTS = os.path.dirname(os.path.abspath(__file__))

# kernels outside the six tables: the source file of csrc/ that defines them -> the direct test module that launches them
DIRECT = {
    "conv.hip": "test_gpu_conv_conformance.py",      # the split-K reduction behind the conv table's splitk rows (no conv_*_kernel<> instantiation)
}


def test_census_equals_the_kernels_of_the_four_files(cmk_lib):
    """No count is written down: a new kernel or instantiation without a row, or a row naming a kernel that is gone, fails here by name."""
    C.assert_census(CASES, C.TABLES["tests/tail_cases.py"][1])
    wrappers = [c for c in CASES if c["wrapper"]]
    assert len(wrappers) == 1 and wrappers[0]["feature"] == "census" and wrappers[0]["entry"] == tc.ROI
    assert hasattr(cmk_lib, tc.WRAPPER) and all(hasattr(cmk_lib, e) for e in tc.ENTRIES)


def test_every_cell_has_a_row_or_a_reason():
    C.assert_cells(CASES, tc, nullable=tc.NULLABLE)
    for c in CASES:
        launches = c["answer"] == "accept" and not (c["entry"] == tc.PASTE and c["r"] == 0)        # R = 0 is accepted and launches nothing
        assert bool(c["kernels"]) == launches, c["id"]
        assert c["null"] is None or c["null"] in tc.NULLABLE[c["entry"]] + tc.OPTIONAL.get(c["entry"], ()), c["id"]
        assert set(c) - {"id", "entry", "feature", "answer", "why", "data", "null", "host_only", "wrapper", "kernels"} == set(tc.DEFAULTS[c["entry"]]), c["id"]


def test_the_rows_keep_the_limits_that_protect_the_machine():
    """No accepted row asks for a geometry whose launch is out of proportion: the restated sizes of every accepted row stay small."""
    for c in CASES:
        if c["answer"] != "accept":
            continue
        if c["entry"] == tc.SELECT:
            assert tc.select_blocks(c) <= 300 and c["cap"] <= 131072, c["id"]
        if c["entry"] == tc.NMS:
            assert c["cap"] <= 40000 and max(c["counts"] + [0]) <= 40000 and len(c["counts"]) == c["n"], c["id"]
        if "counts" in c and c["entry"] != tc.NMS:
            assert len(c["counts"]) == c["n"] and all(0 <= v <= c["topk"] for v in c["counts"]), c["id"]


@pytest.mark.parametrize("entry", tc.ENTRIES)
def test_refused_rows_are_refused_before_any_launch(cmk_lib, entry):
    C.assert_refused_before_launch(cmk_lib, tc, entry, einval=tc.CMK_EINVAL)


# ---------------------------------------------------------------------------------------------------------------
# the library-wide census
# ---------------------------------------------------------------------------------------------------------------
def test_every_kernel_of_the_library_is_claimed_exactly_once(cmk_lib):
    """Every __global__ kernel of csrc/ that the built library holds belongs to the conv table (the conv_*_kernel<...> instantiations that
    tests/test_cpu_conv_conformance.py counts), to the stream table, to the tail table, to the image table (rle.hip, mask_iou.hip and resize.hip,
    claimed per instantiation), to the variant table (conv_deform.hip, dwconv_bn_act.hip, conv_group3.hip and stem7_pool.hip, per instantiation),
    to the vis table (visualize.hip) or to a direct test module named in DIRECT.  A new kernel that nobody claims fails here by name; no count is
    written down."""
    from tests import conv_cases, test_cpu_conv_conformance as conv
    sources = sorted(os.path.basename(f) for f in glob.glob(os.path.join(C.CSRC, "*.hip")) + glob.glob(os.path.join(C.CSRC, "*.hpp")))
    names = C.source_kernels(sources)
    kernels = C.library_kernels(names)
    assert {C.base(k) for k in kernels} == names, "kernels of the sources the library lacks: {}".format(sorted(names - {C.base(k) for k in kernels}))
    tables = {path: conv.library_kernels() if table is conv_cases else C.claimed_kernels(table.all_cases()) for path, (table, _) in C.TABLES.items()}
    claims = {k: [path for path, claimed in tables.items() if k in claimed] for k in kernels}
    for k in kernels:
        for f, module in DIRECT.items():
            if C.base(k) in C.source_kernels([f]):
                claims[k].append("tests/" + module)
    unclaimed = sorted(k for k, v in claims.items() if not v)
    twice = sorted((k, v) for k, v in claims.items() if len(v) > 1)
    assert not unclaimed, "kernels that no table and no direct test module claims: {}".format(unclaimed)
    assert not twice, "kernels claimed more than once: {}".format(twice)
    assert all(claimed <= kernels for claimed in tables.values())
    assert set(DIRECT) == {"conv.hip"}
    assert not set(DIRECT) & set(ic.FILES), "a file of the image table is claimed per instantiation, not per file"
    for f, module in DIRECT.items():
        assert C.source_kernels([f]), "DIRECT names a file without kernels: " + f
        path = os.path.join(TESTS, module)
        assert os.path.exists(path), module
        with open(path) as fh:
            assert "pytest.mark.gpu" in fh.read(), module + " launches nothing on a GPU"
