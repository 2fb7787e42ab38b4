"""The conformance harness (tests/conformance.py) against entry points that misbehave: the protocol the five tables share still bites.
No library and no device: the "entry point" is a Python function on host buffers.  It copies an (n=2, h=3, w=4, c=8) input, which holds
an Inf and a NaN, into the channel slice [4, 12) of a 16-channel output and adds 1 to an in-place operand.  The well-behaved version passes
run_row at distance 0; every other version must make run_row raise an AssertionError that names the row."""
import pytest
import torch

from tests import conformance as C

CPU = torch.device("cpu")
EINVAL = 1
INF_AT, NAN_AT, PLAIN_AT = (0, 1, 2, 3), (1, 2, 0, 5), (1, 0, 3, 7)
X = torch.randn((2, 3, 4, 8), generator=torch.Generator().manual_seed(11))
X[INF_AT], X[NAN_AT] = C.INF, C.NAN
ACC = torch.arange(16, dtype=torch.int32).view(2, 8)


def _row(answer="accept", rid="fake-copy"):
    return dict(id=rid, entry="fake", feature="census" if answer == "accept" else "refuse", answer=answer, kernels=["fake_kernel"] if answer == "accept" else [])


def _bufs():
    B = C.Bufs(CPU)
    B.put("x", X)
    B.out("y", (2, 3, 4, 16), window=(4, 8))
    B.out("acc", (2, 8), torch.int32, init=ACC)
    return B


def _f32(region):
    return region.view(torch.float32)


def _copy(B):
    _f32(B.outs["y"].region()).copy_(_f32(B.ins["x"].region()))
    B.outs["acc"].region().view(torch.int32).add_(1)


def _check(nan_is_zero=False):
    def check(got):
        assert torch.equal(got["acc"], ACC + 1), "fake-copy: the in-place operand"
        ref = torch.relu(X.double()) if nan_is_zero else X.double()         # torch's relu keeps the NaN
        return C.dist(*C.finite_parts(got["y"].double(), ref, "fake-copy", nan_is_zero=nan_is_zero))
    return check


def _run(entry_point, answer="accept", einval=None, nan_is_zero=False):
    """run_row on fresh buffers; entry_point(B, call number) -> (rc, err)."""
    B, calls = _bufs(), []

    def launch(row):
        calls.append(row)
        return entry_point(B, len(calls))
    return C.run_row(_row(answer), B, launch, _check(nan_is_zero), einval=einval)


def _good(B, k):
    _copy(B)
    return 0, ""


def _after(damage):
    """The good entry point, then `damage(B, call number)`."""
    def entry_point(B, k):
        _copy(B)
        damage(B, k)
        return 0, ""
    return entry_point


def _poke(buf, at):
    buf.alloc[at] ^= 1


def _set_y(at, value):
    def damage(B, k):
        _f32(B.outs["y"].region())[at] = value
    return damage


def _other_bits_on_call_two(B, k):
    if k == 2:
        _f32(B.outs["y"].region())[PLAIN_AT] += 1.0


def _leave_the_sentinel(B, k):
    B.outs["y"].region().view(torch.int32)[PLAIN_AT] = -1


def _relu(B, k):
    y = _f32(B.outs["y"].region())
    y.copy_(torch.nan_to_num(torch.relu(y), nan=0.0, posinf=C.INF))


def test_the_well_behaved_entry_point_passes_at_distance_zero():
    assert _run(_good) == 0.0
    assert _run(_after(_relu), nan_is_zero=True) == 0.0                     # NaN -> 0 is accepted where the table says relu(NaN) = 0


MISBEHAVING = {
    "the guard before the output": lambda B, k: _poke(B.outs["y"], B.outs["y"].lo - 4),
    "the guard after the output": lambda B, k: _poke(B.outs["y"], B.outs["y"].lo + B.outs["y"].nbytes),
    "outside the channel slice": lambda B, k: _poke(B.outs["y"], B.outs["y"].lo + 3 * 4),
    "an input element": lambda B, k: _poke(B.ins["x"], B.ins["x"].lo + 40),
    "a byte of an input's guard": lambda B, k: _poke(B.ins["x"], 0),
    "other bits on the second call": _other_bits_on_call_two,
    "an output element left as the sentinel": _leave_the_sentinel,
    "NaN where the reference has Inf": _set_y(INF_AT, C.NAN),
    "Inf where the reference is finite": _set_y(PLAIN_AT, C.INF),
    "NaN -> 0 without nan_is_zero": _set_y(NAN_AT, 0.0),
}


@pytest.mark.parametrize("what", list(MISBEHAVING))
def test_an_accepted_row_that_misbehaves_fails_by_name(what):
    with pytest.raises(AssertionError, match="fake-copy"):
        _run(_after(MISBEHAVING[what]))


def _refuse(rc=EINVAL, err="bad argument", before=None):
    def entry_point(B, k):
        if before:
            before(B)
        return rc, err
    return entry_point


def test_a_well_behaved_refusal_passes_under_both_policies():
    assert _run(_refuse(), "refuse") is None and _run(_refuse(), "refuse", einval=EINVAL) is None
    assert _run(_refuse(rc=-2), "refuse") is None                           # any non-zero code where the table does not name one


REFUSALS = {
    "returns 0": (_refuse(rc=0), None),
    "an empty error text": (_refuse(err=" "), None),
    "writes an output first": (_refuse(before=lambda B: _f32(B.outs["y"].region())[PLAIN_AT].fill_(0.0)), None),
    "-2 under the CMK_EINVAL policy": (_refuse(rc=-2), EINVAL),
    "changes an in-place operand": (_refuse(before=lambda B: B.outs["acc"].region().view(torch.int32)[1, 2].add_(1)), EINVAL),
    "changes an input": (_refuse(before=lambda B: _poke(B.ins["x"], B.ins["x"].lo)), EINVAL),
    "launches after all": (_good, None),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_a_declared_refusal_that_misbehaves_fails_by_name(what):
    entry_point, einval = REFUSALS[what]
    with pytest.raises(AssertionError, match="fake-copy"):
        _run(entry_point, "refuse", einval=einval)


def test_a_misaligned_buffer_and_a_regarded_input():
    """The byte offset of a misalignment row moves the pointer and nothing else; the repeated call sees another byte around a regarded
    input, so an entry point that reads the guard gives other bits."""
    def run(reach, check):
        B = C.Bufs(CPU)
        src = B.put("src", torch.arange(12, dtype=torch.uint8), off=3, guard=256)
        dst = B.out("dst", (12,), torch.uint8, off=5, guard=256)
        assert src.ptr() % 16 == 3 and dst.ptr() % 16 == 5 and torch.equal(src.get(), torch.arange(12, dtype=torch.uint8))
        B.regard = "src"

        def launch(row):
            dst.region().copy_(src.alloc[src.lo - reach:src.lo - reach + 12])
            return 0, ""
        return C.run_row(_row(), B, launch, check)
    assert run(0, lambda got: C.exact(got["dst"], torch.arange(12, dtype=torch.uint8), "fake-copy")) == 0.0
    with pytest.raises(AssertionError, match="a second call gave other bits"):
        run(1, lambda got: None)


def test_a_kept_slice_of_the_output_allocation():
    """An input in the allocation of the output (same_buffer): the call writes its own slice and must keep the other."""
    kept = torch.randn((2, 3, 4, 4), generator=torch.Generator().manual_seed(5))
    for spoil, ok in ((False, True), (True, False)):
        B = C.Bufs(CPU)
        y = B.out("y", (2, 3, 4, 16), window=(8, 4), keep=(0, 4, kept), guard=C.map_guard(_row(), (3, 4, 16)))

        def launch(row):
            whole = _f32(y._slice(y.alloc, 0, 16))
            whole[..., 8:12] = whole[..., 0:4] * 2.0
            if spoil:
                whole[0, 0, 0, 1] = 0.0
            return 0, ""
        if ok:
            assert C.run_row(_row(), B, launch, lambda got: C.exact(got["y"], kept * 2.0, "fake-copy")) == 0.0
        else:
            with pytest.raises(AssertionError, match="fake-copy"):
                C.run_row(_row(), B, launch, lambda got: None)


def test_the_driver_names_every_failing_row_and_counts_against_the_table():
    rows = [_row(rid="row-a"), _row(rid="row-b"), _row("refuse", rid="row-c")]

    def run(c):
        assert c["id"] == "row-b", "broken on purpose\nsecond line"
        return 0.25
    with pytest.raises(AssertionError) as e:
        C.run_entry("fake", rows, run)
    text = str(e.value)
    assert "2 of 3 rows failed" in text and "row-a: broken on purpose" in text and "row-c: broken on purpose" in text and "row-b" not in text and "second line" not in text
    C.run_entry("fake", rows, lambda c: 0.5 if c["answer"] == "accept" else None)
    with pytest.raises(AssertionError):
        C.run_entry("fake", rows[:2], lambda c: 0.5)                        # an entry without a refused row
    with pytest.raises(AssertionError):
        C.run_entry("fake", rows, lambda c: 0.5)                            # a refused row that launched
    nothing = dict(_row(rid="row-d"), kernels=[])                           # accepted, launches nothing: counted by kernels, not by answer
    C.run_entry("fake", rows[:2] + [nothing], lambda c: 0.5 if c["kernels"] else None, count="kernels", report=False)
    with pytest.raises(RuntimeError):                                       # anything but an AssertionError ends the entry at once
        C.run_entry("fake", rows, lambda c: (_ for _ in ()).throw(RuntimeError("device error")))


def test_the_bar_recipe_and_the_comparisons():
    rows = [_row(rid="row-a"), _row(rid="row-b")]
    assert C.fp32_bar("fake", rows, lambda c: 1e-7 if c["id"] == "row-a" else 3e-7) == pytest.approx(1.2e-6)
    assert C.fp32_bar("fake", rows, lambda c: 1e-7, floor=1e-5) == 1e-5
    with pytest.raises(AssertionError):
        C.fp32_bar("fake", rows, lambda c: 0.0)
    nan_a, nan_b = (torch.tensor([v], dtype=torch.int32).view(torch.float32) for v in (0x7FC00000, 0x7FC01234))
    assert C.same_bits(nan_a, nan_a.clone()) and not C.same_bits(nan_a, nan_b)
    for dtype in (torch.uint8, torch.float16, torch.int32, torch.float64):
        t = torch.arange(6).to(dtype)
        assert C.same_bits(t, t.clone()) and not C.same_bits(t, t.flip(0)) and not C.same_bits(t, t[:5])
    assert C.is_filler(C.Buf(CPU, (3, 2), torch.float64).get()) and C.is_filler(C.Buf(CPU, (5,), torch.int64).get())
    assert int(C.Buf(CPU, (1,), torch.int32).get()) == C.SENTINEL[torch.int32] and not C.is_filler(torch.full((2,), C.NAN))
    assert C.dist(torch.tensor([10.0, 21.0]), torch.tensor([10.0, 20.0], dtype=torch.float64)) == 0.05
