"""The conv conformance table (tests/conv_cases.py) against the library's own account of a launch, cmk_conv_plan, on dummy aligned
pointers: no GPU, nothing is launched.  The census — the kernels that the accepted cases name — must be exactly the conv kernels of the
built library, every case must be accepted or refused as the table declares, and every cell of the support matrix must have a case."""
import ctypes
import subprocess

import pytest

from tests import conv_cases as cc


@pytest.fixture(scope="module")
def planned(cmk_lib):
    """[(case, kernel name | None, error text)] of every case of the table."""
    from centermask2_amd import _lib
    buf = (ctypes.c_float * 96)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    out = []
    for c in cc.all_cases():
        descs = cc.fill_descs(c, _lib, ptr=ptr)
        name = ctypes.create_string_buffer(96)
        rc = cmk_lib.cmk_conv_plan(descs, len(descs), name, len(name), None, None)
        out.append((c, name.value.decode() if rc == 0 else None, cmk_lib.cmk_last_error().decode() if rc != 0 else ""))
    return out


def library_kernels():
    """The conv kernel instantiations of the built library (the parse of test_plan_names_are_kernels_of_the_library)."""
    from centermask2_amd import _lib
    syms = subprocess.run("nm -C --defined-only '{}'".format(_lib.LIB_PATH), shell=True, check=True, capture_output=True, text=True).stdout
    return {line.split("cmk::", 1)[1].split("(")[0] for line in syms.splitlines() if " cmk::conv_" in line and "_kernel<" in line}


def test_census_equals_the_kernels_of_the_library(planned):
    """No count is written down: a new instantiation without a case, or a case naming a kernel that is gone, fails here by name."""
    kernels = library_kernels()
    named = {k for c, k, _ in planned if c["answer"] == "accept" and k is not None}
    assert kernels, "no conv kernels found in the library"
    assert named == kernels, "kernels no accepted case launches: {}; cases naming kernels the library lacks: {}".format(
        sorted(kernels - named), sorted(named - kernels))
    census = {k for c, k, _ in planned if c["feature"] == "census" and k is not None}
    assert census == kernels, "kernels without a census row: {}".format(sorted(kernels - census))


def test_every_case_is_answered_as_declared(planned):
    wrong = []
    for c, kernel, err in planned:
        assert c["answer"] in ("accept", "refuse"), c["id"]
        if (kernel is not None) != (c["answer"] == "accept"):
            wrong.append((c["id"], c["answer"], kernel or err))
        if kernel is None:
            assert err.strip(), "refused without an error text: " + c["id"]
        else:
            assert cc.family_of(c) == c["family"], c["id"]
    assert not wrong, wrong
    assert len({c["id"] for c, _, _ in planned}) == len(planned)        # ids name cases


def test_matrix_is_complete(planned):
    cells = {(c["family"], c["feature"]): c["answer"] for c, _, _ in planned if c["feature"] != "census"}
    assert set(cc.MATRIX) == set(cc.FAMILIES)
    not_put = set()
    for family in cc.FAMILIES:
        for feature in cc.FEATURES:
            want = cc.declared(family, feature)
            if want is None:
                not_put.add((family, feature))
                continue
            assert cells.get((family, feature)) == want, (family, feature, cells.get((family, feature)), want)
    assert not_put == set(cc.N_A) and all(cc.N_A.values())              # a cell without a case carries its reason, and there is no other
    assert len(cells) == len(cc.FAMILIES) * len(cc.FEATURES) - len(cc.N_A)


def test_untuned_defaults_resolve_to_census_kernels(planned, cmk_lib):
    """Every distinct problem of the table, without forced features: the variant the library picks by itself plans a kernel of the census."""
    from centermask2_amd import _lib
    buf = (ctypes.c_float * 96)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    census = {k for c, k, _ in planned if c["feature"] == "census" and k is not None}
    problems = {(c["k"], c["stride"], tuple(c["shapes"]), c["cin"], c["cout"]) for c, _, _ in planned}
    assert len(problems) > 30
    for k, stride, shapes, cin, cout in sorted(problems):
        if len(shapes) > 5:
            continue                  # ten problems are no launch of the untuned library: they take tune_wm 6 | 11 by name
        c = cc.case(k=k, stride=stride, shapes=list(shapes), cin=cin, cout=cout, tv=(0, 0, 0))
        descs = cc.fill_descs(c, _lib, ptr=ptr)
        v = (ctypes.c_int * 3)()
        assert cmk_lib.cmk_conv_resolve(descs, len(descs), 0, v) == 0, (c, cmk_lib.cmk_last_error())
        assert tuple(v) != (0, 0, 0)
        name = ctypes.create_string_buffer(96)
        explicit = cc.fill_descs(dict(c, tv=tuple(v)), _lib, ptr=ptr)
        assert cmk_lib.cmk_conv_plan(explicit, len(explicit), name, len(name), None, None) == 0, (c, tuple(v), cmk_lib.cmk_last_error())
        assert name.value.decode() in census, (c, tuple(v), name.value)
        untuned = ctypes.create_string_buffer(96)
        assert cmk_lib.cmk_conv_plan(descs, len(descs), untuned, len(untuned), None, None) == 0 and untuned.value == name.value
