"""The tail conformance table (tests/tail_cases.py) without a GPU: nothing is launched.  The kernels that the accepted rows name must be
exactly the __global__ kernels of csrc/detect.hip, csrc/roi.hip, csrc/prepost.hip and csrc/keypoint.hip as the built library instantiates
them, every (entry point, feature) cell must have a row or a reason, and every refused row must be refused on dummy aligned pointers: every
argument check of these entry points sits before its launch.  And the library-wide census: every kernel of the built library is claimed by
exactly one of the five conformance tables (conv, stream, tail, image, variant) or by a named direct test module."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

from tests import image_cases as ic
from tests import stream_cases as sc
from tests import tail_cases as tc
from tests import variant_cases as vc

CASES = tc.all_cases()
TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "centermask2_amd", "csrc")
TAIL_FILES = ("detect.hip", "roi.hip", "prepost.hip", "keypoint.hip")

# kernels outside the five tables: the source file of csrc/ that defines them -> the direct test module that launches them
DIRECT = {
    "visualize.hip": "test_gpu_visualize.py",
    "conv.hip": "test_gpu_conv_conformance.py",      # the split-K reduction behind the conv table's splitk rows (no conv_*_kernel<> instantiation)
}


def source_kernels(files):
    """The __global__ kernel names of these files of csrc/."""
    names = set()
    for f in files:
        with open(os.path.join(CSRC, f)) as fh:
            names |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", fh.read()))
    return names


def library_kernels(names):
    """Their instantiations in the built library: the kernel handles `nm -C` prints as cmk::name[<args>](...)."""
    from centermask2_amd import _lib
    syms = subprocess.run(["nm", "-C", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    found = set()
    for line in syms.splitlines():
        m = re.search(r" (?:void )?cmk::(?:\(anonymous namespace\)::)?(\w+(?:<[^>]*>)?)\(", line)
        if m and m.group(1).split("<")[0] in names:
            found.add(m.group(1))
    return found


def base(kernel):
    return kernel.split("<")[0]


def test_census_equals_the_kernels_of_the_four_files(cmk_lib):
    """No count is written down: a new kernel or instantiation without a row, or a row naming a kernel that is gone, fails here by name."""
    names = source_kernels(TAIL_FILES)
    assert names, "no __global__ kernel found in the sources"
    kernels = library_kernels(names)
    assert {base(k) for k in kernels} == names, "kernels of the sources the library lacks: {}".format(sorted(names - {base(k) for k in kernels}))
    named = {k for c in CASES if c["answer"] == "accept" for k in c["kernels"]}
    assert named == kernels, "kernels no accepted row launches: {}; rows naming kernels the library lacks: {}".format(sorted(kernels - named), sorted(named - kernels))
    census = {k for c in CASES if c["feature"] == "census" for k in c["kernels"]}
    assert census == kernels, "kernels without a census row: {}".format(sorted(kernels - census))
    wrappers = [c for c in CASES if c["wrapper"]]
    assert len(wrappers) == 1 and wrappers[0]["feature"] == "census" and wrappers[0]["entry"] == tc.ROI
    assert hasattr(cmk_lib, tc.WRAPPER) and all(hasattr(cmk_lib, e) for e in tc.ENTRIES)


def test_every_cell_has_a_row_or_a_reason():
    assert {c["entry"] for c in CASES} == set(tc.ENTRIES) and {c["feature"] for c in CASES} == set(tc.FEATURES)
    cells = {(c["entry"], c["feature"]) for c in CASES}
    for e in tc.ENTRIES:
        for f in tc.FEATURES:
            assert ((e, f) in cells) != ((e, f) in tc.N_A), (e, f, "a cell has a row or a reason, not both and not neither")
    assert all(isinstance(v, str) and v.strip() for v in list(tc.N_A.values()) + list(tc.PRECONDITIONS.values()))
    assert set(tc.PRECONDITIONS) <= set(tc.ENTRIES)
    assert len({c["id"] for c in CASES}) == len(CASES)                   # ids name rows
    for c in CASES:
        assert c["answer"] in ("accept", "refuse") and (c["answer"] == "refuse") == (c["feature"] == "refuse"), c["id"]
        launches = c["answer"] == "accept" and not (c["entry"] == tc.PASTE and c["r"] == 0)        # R = 0 is accepted and launches nothing
        assert bool(c["kernels"]) == launches, c["id"]
        assert not c["host_only"] or c["answer"] == "refuse", c["id"]
        assert c["null"] is None or c["null"] in tc.NULLABLE[c["entry"]] + tc.OPTIONAL.get(c["entry"], ()), c["id"]
        assert set(c) - {"id", "entry", "feature", "answer", "why", "data", "null", "host_only", "wrapper", "kernels"} == set(tc.DEFAULTS[c["entry"]]), c["id"]
    for e in tc.ENTRIES:                                                 # every pointer of every entry point has its NULL row
        nulled = {c["null"] for c in CASES if c["entry"] == e and c["null"]}
        assert nulled >= set(tc.NULLABLE[e]), (e, sorted(set(tc.NULLABLE[e]) - nulled))


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
    buf = (ctypes.c_float * 96)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    rows = [c for c in CASES if c["entry"] == entry and c["answer"] == "refuse"]
    assert rows
    for c in rows:
        rc = tc.call(cmk_lib, c, tc.dummy_pointers(c, ptr))
        err = cmk_lib.cmk_last_error().decode()
        # CMK_EINVAL is the argument checks' code; a call that got as far as its launch returns CMK_ELAUNCH here (there is no device)
        assert rc == tc.CMK_EINVAL, (c["id"], "declared refuse, but the call went on to its launch" if rc else "declared refuse, accepted", rc, err)
        assert err.strip(), (c["id"], "refused without an error text")


# ---------------------------------------------------------------------------------------------------------------
# the library-wide census
# ---------------------------------------------------------------------------------------------------------------
def test_every_kernel_of_the_library_is_claimed_exactly_once(cmk_lib):
    """Every __global__ kernel of csrc/ that the built library holds belongs to the conv table (the conv_*_kernel<...> instantiations that
    tests/test_cpu_conv_conformance.py counts), to the stream table, to the tail table, to the image table (rle.hip, mask_iou.hip and resize.hip,
    claimed per instantiation), to the variant table (conv_deform.hip, dwconv_bn_act.hip, conv_group3.hip and stem7_pool.hip, per instantiation)
    or to a direct test module named in DIRECT.  A new kernel that nobody claims fails here by name; no count is
    written down."""
    from tests import test_cpu_conv_conformance as conv
    sources = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    names = source_kernels(sources)
    kernels = library_kernels(names)
    assert {base(k) for k in kernels} == names, "kernels of the sources the library lacks: {}".format(sorted(names - {base(k) for k in kernels}))
    claims = {k: [] for k in kernels}
    conv_kernels = conv.library_kernels()
    stream = {k for c in sc.all_cases() if c["answer"] == "accept" for k in c["kernels"]}
    tail = {k for c in CASES if c["answer"] == "accept" for k in c["kernels"]}
    image = {k for c in ic.all_cases() if c["answer"] == "accept" for k in c["kernels"]}
    variant = {k for c in vc.all_cases() if c["answer"] == "accept" for k in c["kernels"]}
    for k in kernels:
        if k in conv_kernels:
            claims[k].append("tests/conv_cases.py")
        if k in stream:
            claims[k].append("tests/stream_cases.py")
        if k in tail:
            claims[k].append("tests/tail_cases.py")
        if k in image:
            claims[k].append("tests/image_cases.py")
        if k in variant:
            claims[k].append("tests/variant_cases.py")
        for f, module in DIRECT.items():
            if base(k) in source_kernels([f]):
                claims[k].append("tests/" + module)
    unclaimed = sorted(k for k, v in claims.items() if not v)
    twice = sorted((k, v) for k, v in claims.items() if len(v) > 1)
    assert not unclaimed, "kernels that no table and no direct test module claims: {}".format(unclaimed)
    assert not twice, "kernels claimed more than once: {}".format(twice)
    assert conv_kernels <= kernels and stream <= kernels and tail <= kernels and image <= kernels and variant <= kernels
    assert set(DIRECT) == {"visualize.hip", "conv.hip"}
    assert not set(DIRECT) & set(ic.FILES), "a file of the image table is claimed per instantiation, not per file"
    for f, module in DIRECT.items():
        assert source_kernels([f]), "DIRECT names a file without kernels: " + f
        path = os.path.join(TESTS, module)
        assert os.path.exists(path), module
        with open(path) as fh:
            assert "pytest.mark.gpu" in fh.read(), module + " launches nothing on a GPU"
