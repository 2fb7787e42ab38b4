"""The image-side conformance table (tests/image_cases.py) without a GPU: nothing is launched.  The kernels that the accepted rows name
must be exactly the __global__ kernels of csrc/resize.hip, csrc/rle.hip and csrc/mask_iou.hip as the built library instantiates them, every
(entry, feature) cell must have a row or a reason, the geometry a row exists for must be what the restated launch code makes of its
arguments, no accepted row may grow into a workload, and every refused row must be refused with CMK_EINVAL on dummy aligned pointers:
every argument check of these entries sits before its launch."""
import os

import pytest

from tests import conformance as C
from tests import image_cases as ic

CASES = ic.all_cases()
ACCEPTED = [c for c in CASES if c["answer"] == "accept"]
ROW_KEYS = {"id", "entry", "feature", "answer", "why", "data", "null", "host_only", "expect", "kernels"}


def test_census_equals_the_kernels_of_the_three_files(cmk_lib):
    """No count is written down: a new kernel or instantiation without a row, or a row naming a kernel that is gone, fails here by name."""
    C.assert_census(CASES, ic.FILES)
    for e in ic.ENTRIES:
        assert all(hasattr(cmk_lib, name) for name in e.split("+")), e


def test_every_cell_has_a_row_or_a_reason():
    C.assert_cells(CASES, ic, nullable=ic.NULLABLE)
    assert all(isinstance(v, str) and v.strip() for v in ic.NO_ROW.values())
    for c in CASES:
        assert c["why"].strip(), c["id"]
        if c["answer"] == "accept" and not c["kernels"]:                 # accepted and launching nothing: a count of zero
            assert min(c.get(k, 1) for k in ("r", "m", "n")) == 0 and "touches nothing" in c["why"], c["id"]
        assert c["null"] is None or c["null"] in ic.NULLABLE[c["entry"]], c["id"]
        assert set(c) - ROW_KEYS == set(ic.DEFAULTS[c["entry"]]), c["id"]
    for e in ic.ENTRIES:                                                 # every pointer of every entry has its NULL row
        nulled = {c["null"] for c in CASES if c["entry"] == e and c["null"]}
        assert nulled == set(ic.NULLABLE[e]), (e, sorted(set(ic.NULLABLE[e]) ^ nulled))
        assert set(ic.NULLABLE[e]) <= set(ic.POINTERS[e])
        zero = [c for c in ACCEPTED if c["entry"] == e and not c["kernels"]]
        assert bool(zero) == (e in (ic.RLE, ic.PACK, ic.DEC, ic.INTER, ic.BND, ic.UNPACK)), (e, "a count of 0 is an accepted row that launches nothing")
    both = {c["null"] for c in CASES if c["entry"] == ic.RLE and c["null"] and c["phase"] == "count"}
    assert both == set(ic.COUNT_PHASE)                                   # the pair: each phase refuses its own pointers


def test_the_restated_geometry_is_what_the_rows_say():
    """A row exists for a branch; `expect` names the restated quantity that takes it.  The words of `why` and the numbers must agree."""
    for c in ACCEPTED:
        g = ic.geometry(c)
        for k, v in c["expect"].items():
            assert k in g and g[k] == v, (c["id"], k, "the row says", v, "the restated launch code says", g.get(k))
    say = {"two tiles across": ("nxt", 2), "three tiles across": ("nxt", 3), "two halo words": ("q", 2), "one halo word": ("q", 1),
           "64-pixel step": ("step64", 1), "exactly 64 KiB": ("lds", 65536), "shrunk to 8": ("TW", 8), "no square fits": ("fits", 0),
           "the scalar kernel": ("v", 1), "the vector kernel": ("v", 4), "ksize 17": ("ksize", 17), "ksize 3": ("ksize", 3), "no tail store": ("tail", 0),
           "a second chunk": ("chunks", 2), "the funnel": ("aligned", 0), "aligned": ("aligned", 1)}
    said = set()
    for c in ACCEPTED:
        g = ic.geometry(c)
        for words, (k, v) in say.items():
            if words in c["why"] and k in g and not (words == "aligned" and "not aligned" in c["why"]):
                assert g[k] == v, (c["id"], "says '{}' but the restated {} is {}".format(words, k, g[k]))
                said.add(words)
        if c["feature"] == "second_trip":
            assert max(g.get(k, 0) for k in ("trips", "scan_trips", "offset_trips")) >= 2 or "string kernel" in c["why"], (c["id"], g)
        elif "trips" in g:
            assert g["trips"] == 1, c["id"]
    assert said == set(say), sorted(set(say) - said)
    # the branches of the boundary kernel that the issue names, each on some accepted row
    bnd = [ic.geometry(c) for c in ACCEPTED if c["entry"] == ic.BND and c["kernels"] == ["mask_boundary_kernel"]]
    assert any(g["q"] == 2 for g in bnd) and any(g["step64"] for g in bnd) and any(g["shrunk"] and g["TW"] == 8 for g in bnd)
    assert any(g["nxt"] == 2 for g in bnd) and any(g["nxt"] == 3 for g in bnd) and max(g["lds"] for g in bnd) == 65536
    assert all(g["lds"] <= 65536 and g["TR"] >= 1 and 1 <= g["TW"] <= 32 for g in bnd)
    assert {c["d"] for c in ACCEPTED if c["entry"] == ic.BND and c["kernels"] == ["mask_boundary_kernel"]} >= {1, 64, 65, 127, 128}
    # resize_h: both tail kinds and the second trip; tta_reduce: both kernels on both sides of an alignment and a second trip of each
    rh = [ic.geometry(c) for c in ACCEPTED if c["entry"] == ic.RH]
    assert {g["tail"] == 0 for g in rh} == {True, False} and max(g["trips"] for g in rh) == 2 and max(g["quads"] for g in rh) == 2101050
    tr = [(c, ic.geometry(c)) for c in ACCEPTED if c["entry"] == ic.TRED]
    assert {(g["v"], g["trips"]) for _, g in tr} == {(1, 1), (4, 1), (1, 2), (4, 2)}
    assert any(g["v"] == 1 and c["s"] % 4 == 0 and c["masks_off"] for c, g in tr) and any(g["v"] == 1 and c["s"] % 4 == 0 and c["out_off"] for c, g in tr)
    assert 1081700 in {g["items"] for _, g in tr}                       # K 100, S 208 with scores: 1,081,600 + 100
    # the exact tile multiples
    inter = [ic.geometry(c) for c in ACCEPTED if c["entry"] == ic.INTER and c["kernels"]]
    assert {g["words"] for g in inter} >= {1, 512, 513} and {g["gt_tiles"] for g in inter} >= {1, 2, 3} and {g["nblocks"] for g in inter} == {1, 2}
    for e in (ic.PACK, ic.UNPACK, ic.DEC):
        assert {c["h"] * c["w"] for c in ACCEPTED if c["entry"] == e} >= {1, 64, 65, 512, 513, 2048, 2049}, e
    assert {c["w"] for c in ACCEPTED if c["entry"] == ic.RLE} >= {256, 257, 1024, 1025} and {c["off"] for c in ACCEPTED if c["entry"] == ic.RLE} == {0, 1, 2, 3}


def test_no_row_grows_into_a_workload():
    for c in ACCEPTED:
        assert ic.largest_buffer(c) <= ic.MAX_BYTES, (c["id"], ic.largest_buffer(c))
        for k in ("counts", "flips"):
            assert k not in c or len(c[k]) == c["a"], c["id"]
        if c["entry"] == ic.BND:
            assert c["r"] <= 17 and c["h"] * c["w"] * min(c["d"], min(c["h"], c["w"])) <= 1 << 27, (c["id"], "the literal 3x3 reference iterates d times")
    assert sum(ic.largest_buffer(c) > (4 << 20) for c in ACCEPTED) <= 6


def test_ksize_and_workspace_formulas(cmk_lib):
    for i, o in [(53, 87), (230, 31), (1, 3), (9, 1), (37, 37), (1000, 2001), (480, 800), (1333, 800), (7, 7), (65535, 1)]:
        assert cmk_lib.cmk_resize_ksize(i, o) == ic.ksize_of(i, o), (i, o)
    assert cmk_lib.cmk_resize_ksize(0, 5) == 0 and cmk_lib.cmk_resize_ksize(5, 0) == 0 and cmk_lib.cmk_resize_ksize(-1, -1) == 0
    for r, h, w in [(1, 1, 1), (13, 97, 131), (2, 1100, 1000), (1025, 3, 5), (0, 5, 3), (65535, 64, 1), (3, 65, 4), (3, 64, 4)]:
        assert cmk_lib.cmk_rle_ws_bytes(r, h, w) == ic.rle_ws_bytes(r, h, w), (r, h, w)
    for r, h, w in [(-1, 5, 3), (65536, 5, 3), (1, 0, 3), (1, 3, 0), (1, ic.TOO_BIG, ic.TOO_BIG)]:
        assert cmk_lib.cmk_rle_ws_bytes(r, h, w) == 0, (r, h, w)
    with open(os.path.join(os.path.dirname(os.path.abspath(ic.__file__)), "..", "include", "cmk.h")) as fh:
        assert "#define CMK_BOUNDARY_MAX_D {}\n".format(ic.CMK_BOUNDARY_MAX_D) in fh.read()


@pytest.mark.parametrize("entry", ic.ENTRIES)
def test_refused_rows_are_refused_before_any_launch(cmk_lib, entry):
    C.assert_refused_before_launch(cmk_lib, ic, entry, einval=ic.CMK_EINVAL)
