"""The value rows of the conv conformance table can fail: without a GPU and without the library, from the float64 reference
(conv_cases.reference) and the fp32 emulations of the families' algorithms (conv_values.emulate) alone.

The exactness the rows claim holds in every emulation said to have it; kernels that lack one of their products, or carry one wrong entry
in A^T, miss a row's bar by at least 4x; the reach of a poisoned pixel is exactly where the reference and the emulations go non-finite."""
import functools

import pytest
import torch

from tests import conformance as C
from tests import conv_cases as cc
from tests import conv_values as cv

ROWS = {}
for _c in cc.all_cases():
    if _c["regime"]:
        ROWS.setdefault((_c["family"], _c["feature"]), _c)       # the cell's own row: the family's plain problem (further nonfinite rows follow it)


def _algorithm(c):
    """Families that share an emulation and a problem share its results here (the three F(4x4) kernels, the two sp3 tilings)."""
    return (c["tv"][0], c["k"], c["stride"], tuple(c["shapes"]), c["cin"], c["cout"], c["regime"], c["zero_shift"], c["relu_upto"])


@functools.lru_cache(maxsize=None)
def _results(key, family, feature):
    """{label: (tensors, float64 reference, emulation)} of a row."""
    c = ROWS[(family, feature)]
    return {label: (t, cc.reference(c, t), cv.emulate(c, t)) for label, t in cv.launch_sets(c, 0).items()}


def results(family, feature):
    c = ROWS[(family, feature)]
    first = next(f for f in cc.FAMILIES if (f, feature) in ROWS and _algorithm(ROWS[(f, feature)]) == _algorithm(c))
    return _results(_algorithm(c), first, feature)


def test_every_value_cell_has_its_row():
    for family in cc.FAMILIES:
        for feature in cc.VALUE_FEATURES:
            assert ((family, feature) in ROWS) != ((family, feature) in cc.N_A), (family, feature)
    assert {f for f, feat in ROWS if feat == "f16_domain"} == {"pw split fp16 (wm 12)", "sp3 (sc 2)", "sp3 (sc 21)"}
    assert all(feat in ("ints", "pow2_channels") and (f, feat) in ROWS and why.strip() for (f, feat), why in cc.HELD_TO_BAR.items())


@pytest.mark.parametrize("family", list(cc.FAMILIES))
def test_exactness_claims_hold_in_the_emulations(family):
    # ints: exact where it is said to be, and every sum of magnitudes below 2^24 (in the fp16 pieces' own units too)
    c = ROWS[(family, "ints")]
    t, ref, emu = results(family, "ints")["row"]
    for i in range(len(c["shapes"])):
        mags = cc.reference(c, dict(t, x=[x.abs() for x in t["x"]], w=[w.abs() for w in t["w"]], shift=[s.abs() for s in t["shift"]]))["y"][i]
        assert float(mags.max()) < 2.0 ** 24
        if cv.f16_split(c):
            pw, s_w = cv.pieces_f16_w(t["w"][0])
            assert float(pw["m"].abs().max()) == 0.0 and float(cv.pieces_f16_x(t["x"][i])["m"].abs().max()) == 0.0       # x * 2^-4 and w * S_w are exact in fp16
            assert float(mags.max()) * s_w / 16.0 < 2.0 ** 24                 # the accumulator holds the sums times S_w * 2^-4
        if cv.exact_ints(c):
            assert torch.equal(emu[i].double(), ref["y"][i]), (family, "ints is not exact in the emulation")
        else:
            assert not torch.equal(emu[i].double(), ref["y"][i])          # the reason on record holds: F(4x4) is not exact
    # pow2_channels: the emulation gives the same bits with and without the per-channel powers of two
    c = ROWS[(family, "pow2_channels")]
    r = results(family, "pow2_channels")
    for a, b in zip(r["plain"][2], r["row"][2]):
        if cv.exact_pow2(c):
            assert C.same_bits(a, b), (family, "pow2_channels changes the emulation's bits")
    for a, b in zip(r["plain"][1]["y"], r["row"][1]["y"]):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))      # (float64 itself only reorders its sums)
    # sparse: the all-zero image is relu(shift) per channel, exactly
    c = ROWS[(family, "sparse")]
    t, ref, emu = results(family, "sparse")["row"]
    want = t["shift"][-1].relu()
    assert torch.equal(emu[-1][-1], want.expand_as(emu[-1][-1])) and torch.equal(ref["y"][-1][-1], want.double().expand_as(ref["y"][-1][-1]))
    assert float(emu[-1][0].abs().max()) > 0.0


def _mutant_ratios(family, **mutant):
    """{feature: (mutant's distance, bar)} over the rows of the family that have one bar for the whole output."""
    out = {}
    for feature in ("cancel", "sparse", "ints", "f16_domain"):
        if (family, feature) not in ROWS:
            continue
        c = ROWS[(family, feature)]
        for label, (t, ref, emu) in results(family, feature).items():
            own = max(float((e.double() - r).abs().max()) for e, r in zip(emu, ref["y"]))
            got = max(float((e.double() - r).abs().max()) for e, r in zip(cv.emulate(c, t, **mutant), ref["y"]))
            out[feature + " " + label] = (got, cv.MARGIN * own)
    return out


MUTANTS = [("pw split bf16 (wm 10)", dict(drop=d)) for d in ("lh", "hl", "mm")] + \
          [(f, dict(drop=d)) for f in ("pw split fp16 (wm 12)", "sp3 (sc 2)") for d in ("mh", "hm")] + \
          [(f, dict(mats="AT4")) for f in ("wino6 map tiles", "wino6 RoI pairs")]


@pytest.mark.parametrize("family,mutant", MUTANTS, ids=["{} {}".format(f, "-".join(str(v) for v in m.values())) for f, m in MUTANTS])
def test_mutants_miss_the_bar(family, mutant):
    """A kernel with one product dropped, or with one entry of A^T off by one, is at least 4x above the bar on a row of its family."""
    if mutant.get("mats") == "AT4":
        bt, g, at = cv.wino_numerics.MATS[4]
        at = at.clone()
        at[1, 3] += 1
        mutant = dict(mats={2: cv.wino_numerics.MATS[2], 4: (bt, g, at)})
    ratios = _mutant_ratios(family, **mutant)
    for row, (got, bar) in ratios.items():
        print("{} | {}: mutant {:.3e}, bar {:.3e}, ratio {:.1f}".format(family, row, got, bar, got / bar if bar else float("inf")))
    assert any(got >= 4.0 * bar and got > 0.0 for got, bar in ratios.values()), ratios
    got, bar = ratios["cancel row"]
    assert got >= 4.0 * bar, ("cancel is the row that separates them", got, bar)


@pytest.mark.parametrize("family", list(cc.FAMILIES))
def test_nonfinite_reach_is_where_the_reference_and_the_emulation_go_nonfinite(family):
    c = ROWS[(family, "nonfinite")]
    r = results(family, "nonfinite")
    direct = dict(c, tv=(1, 16, 1))
    for label in ("inf", "nan"):
        p, j, py, px, _ = cv.poison_site(c, label)
        n, h, w = c["shapes"][p]
        t, ref, emu = r[label]
        for i in range(len(c["shapes"])):
            for img in range(c["shapes"][i][0]):
                bad_ref, bad_emu = ~torch.isfinite(ref["y"][i][img]), ~torch.isfinite(emu[i][img])
                hit = (i, img) == (p, j)
                want_ref = cv.reach(direct, h, w, py, px) if hit else torch.zeros(bad_ref.shape[:2], dtype=torch.bool)
                want_emu = cv.reach(c, h, w, py, px) if hit else want_ref
                assert torch.equal(bad_ref, want_ref[..., None].expand_as(bad_ref)), (family, label, i, img, "float64")
                assert torch.equal(bad_emu, want_emu[..., None].expand_as(bad_emu)), (family, label, i, img, "emulation")
                assert not hit or (bool(want_ref.any()) and bool((want_ref <= want_emu).all()))
                if not hit:                                      # and nothing else moved: the clean launch's bits
                    assert C.same_bits(emu[i][img], r["clean"][2][i][img])
