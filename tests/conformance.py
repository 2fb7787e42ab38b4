"""The conformance harness: what the six kernel conformance tables (tests/*_cases.py) and their CPU and GPU test modules share.

The protocol of a row, stated once (run_row).  Every buffer handed to the call is the middle of a larger allocation of filler bytes (Buf).
A refused row returns the table's refusal code with an error text and leaves every buffer untouched.  An accepted row writes nothing
outside its outputs, leaves every input and its guards bit-unchanged, meets its reference (the table's check, which gets the outputs on
the host) and gives the same bits when the same call runs again into fresh filler.  run_entry drives the rows of one entry point and
counts them against the table; fp32_bar is the recipe of the bars that come from torch's own fp32 error.  The CPU side: the kernels of the
sources and of the built library, the census, the cell check, the refusal on dummy pointers, and TABLES, the registry the library-wide
census iterates.  Nothing here knows an entry point."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import torch

from tests import conv_cases, image_cases, stream_cases, tail_cases, variant_cases, vis_cases

NAN, INF = float("nan"), float("inf")
SENTINEL = {torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}      # the integer filler, by dtype
PAD = 1024            # elements of filler before and after a second_trip output: whole guard images would triple tens of MB
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centermask2_amd", "csrc")

# cases file -> (its module, the files of csrc/ whose kernels it claims per instantiation).  The conv table claims the conv_*_kernel<>
# instantiations of the library instead (tests/test_cpu_conv_conformance.py counts them); a further table is one more line
TABLES = {
    "tests/conv_cases.py": (conv_cases, ()),
    "tests/stream_cases.py": (stream_cases, ("elementwise.hip", "groupnorm.hip")),
    "tests/tail_cases.py": (tail_cases, ("detect.hip", "roi.hip", "prepost.hip", "keypoint.hip")),
    "tests/image_cases.py": (image_cases, image_cases.FILES),
    "tests/variant_cases.py": (variant_cases, ("conv_deform.hip", "dwconv_bn_act.hip", "conv_group3.hip", "stem7_pool.hip")),
    "tests/vis_cases.py": (vis_cases, ("visualize.hip",)),
}


# ---------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def is_filler(t):
    """Every byte of a host tensor or array is the filler of its dtype: 0xFF in floats (a NaN), 0x5A in everything else (SENTINEL)."""
    a = np.ascontiguousarray(t.numpy() if torch.is_tensor(t) else t)
    return bool((a.reshape(-1).view(np.uint8) == (0xFF if a.dtype.kind == "f" else 0x5A)).all())


def finite_parts(got, ref, what, nan_is_zero=False):
    """NaN and Inf sit where the reference has them (nan_is_zero: a fused ReLU's documented relu(NaN) = 0); returns the finite rest."""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    ref_nan = torch.isnan(ref)
    if nan_is_zero:
        assert not bool(torch.isnan(got).any()), what + ": {} NaN behind the ReLU, the reference has {}".format(int(torch.isnan(got).sum()), int(ref_nan.sum()))
        assert bool((got[ref_nan] == 0).all()), what + ": relu(NaN) must be 0"
    else:
        assert torch.equal(torch.isnan(got), ref_nan), what + ": NaN elsewhere than in the reference ({} vs {})".format(int(torch.isnan(got).sum()), int(ref_nan.sum()))
    for inf in (INF, -INF):
        assert torch.equal(got == inf, ref == inf), what + ": {} elsewhere than in the reference".format(inf)
    ok = torch.isfinite(ref)
    return got[ok], ref[ok]


def exact(got, ref, what):
    g, r = finite_parts(got, ref, what)
    assert torch.equal(g, r), what + ": not equal, max abs err {:.3e}".format(float((g.double() - r.double()).abs().max()) if g.numel() else 0.0)
    return 0.0


def rel(err, ref):
    """An absolute error as a normalised distance: err / max(1, max|ref|)."""
    return err / max(1.0, float(ref.abs().max())) if ref.numel() else 0.0


def dist(a, ref):
    return rel(float((a.double() - ref).abs().max()), ref)


# ---------------------------------------------------------------------------------------------------------------
# the guarded buffer
# ---------------------------------------------------------------------------------------------------------------
def map_guard(c, rest, itemsize=4):
    """The guard bytes of an (N,) + rest map: one image each side, PAD elements for a second_trip row."""
    return (PAD if c["feature"] == "second_trip" else math.prod(rest)) * itemsize


class Buf:
    """A buffer of `shape` and `dtype` in the middle of a byte allocation of filler (0xFF in floats, which reads as NaN; 0x5A elsewhere):
    `guard` bytes before it, plus the byte offset `off` of a misalignment row, and at least `guard` after it (by default 64 elements and
    two leading-dimension units, whichever is more).  window = (co, ch): the call owns only the channel slice [co, co + ch) of the last
    dimension and the rest of the buffer must stay filler.  keep = (co, ch, tensor): that slice holds the tensor and must keep it (an input
    in the allocation of the output).  init: what the region holds before the call (an input, an in-place operand); None: filler."""

    def __init__(self, dev, shape, dtype=torch.float32, init=None, guard=None, off=0, window=None, keep=None):
        self.shape, self.dtype = tuple(shape), dtype
        self.size = torch.empty(0, dtype=dtype).element_size()
        self.nbytes = math.prod(self.shape) * self.size
        self.fill = 0xFF if dtype.is_floating_point else 0x5A
        if guard is None:
            unit = max(1, math.prod(self.shape[1:]))
            guard = max(2, -(-64 // unit)) * unit * self.size
        assert 0 <= off < 16 and not (off and (window or keep))
        self.lo = guard + off
        self.alloc = torch.empty(2 * guard + 16 + self.nbytes, dtype=torch.uint8, device=dev)
        assert self.alloc.data_ptr() % 64 == 0
        self.window = window
        self.keep = keep and keep[:2]
        self.kept = keep and self._bytes(keep[2].to(dev))
        self.init = None if init is None else self._bytes(init.to(dev))
        assert self.init is None or self.init.shape == self.region().shape, (tuple(self.init.shape), tuple(self.region().shape))
        self.reset()

    def _bytes(self, t):
        assert t.dtype == self.dtype, (t.dtype, self.dtype)
        return t.contiguous().reshape(-1).view(torch.uint8).view(tuple(t.shape[:-1]) + (t.shape[-1] * self.size,))

    def _mid(self, alloc):
        return alloc[self.lo:self.lo + self.nbytes]

    def _slice(self, alloc, co, ch):
        """The bytes of the channels [co, co + ch) of the buffer."""
        return self._mid(alloc).view(self.shape[:-1] + (self.shape[-1] * self.size,))[..., co * self.size:(co + ch) * self.size]

    def region(self, alloc=None):
        """The bytes the call may write (a view of the allocation, the last dimension in bytes)."""
        return self._slice(self.alloc if alloc is None else alloc, *(self.window or (0, self.shape[-1])))

    def reset(self, guard_fill=None):
        """Fresh filler everywhere (guard_fill: another byte in the guards), then the kept slice and the initial content."""
        self.guard_fill = self.fill if guard_fill is None else guard_fill
        self.alloc.fill_(self.guard_fill)
        self._mid(self.alloc).fill_(self.fill)
        if self.keep:
            self._slice(self.alloc, *self.keep).copy_(self.kept)
        if self.init is not None:
            self.region().copy_(self.init)

    def ptr(self):
        return self.alloc.data_ptr() + self.lo

    def get(self, region=None):
        """The region (or a clone of it) on the host, in the buffer's dtype."""
        return (self.region() if region is None else region).cpu().contiguous().view(self.dtype)

    def outside_untouched(self):
        """The guards and whatever of the buffer the call does not own: filler byte for byte, the kept slice bit-unchanged."""
        t, hi = self.alloc, self.lo + self.nbytes
        if self.window or self.keep:
            t = self.alloc.clone()
            self.region(t).fill_(self.fill)
            if self.keep:
                if not torch.equal(self._slice(t, *self.keep), self.kept):
                    return False
                self._slice(t, *self.keep).fill_(self.fill)
            if not bool((t[self.lo:hi] == self.fill).all()):
                return False
        return bool((t[:self.lo] == self.guard_fill).all()) and bool((t[hi:] == self.guard_fill).all())

    def untouched(self):
        """As reset() left it."""
        return self.outside_untouched() and (bool((self.region() == self.fill).all()) if self.init is None else torch.equal(self.region(), self.init))


class Bufs:
    """The buffers of one row: p, the pointers by argument name; ins, what the call may only read; outs, what it writes (outputs,
    workspaces, in-place operands).  And the optional hooks of run_row."""

    def __init__(self, dev):
        self.dev, self.p, self.ins, self.outs = dev, {}, {}, {}
        self.steps = None          # the calls of an accepted row when it is more than one (the RLE pair: count, then encode)
        self.between = None        # check(outputs on the host) after the first of them, before the second is allowed to run
        self.again = ()            # further forms of the row, each launched into fresh buffers and held to the first call's bits
        self.regard = None         # name of an input whose guards hold another byte on the repeated call
        self.extra = None          # extra(first): whatever else must give the bits `first` of the outputs (siblings, a dense call)

    def put(self, name, t, key=None, **kw):
        b = self.ins[name] = Buf(self.dev, t.shape, t.dtype, init=t, **kw)
        self.p[key or name] = b.ptr()
        return b

    def out(self, name, shape, dtype=torch.float32, init=None, **kw):
        b = self.outs[name] = Buf(self.dev, shape, dtype, init=init, **kw)
        self.p[name] = b.ptr()
        return b


# ---------------------------------------------------------------------------------------------------------------
# the protocol of a row, the driver of an entry point, the bar recipe
# ---------------------------------------------------------------------------------------------------------------
def run_row(c, B, launch, check, einval=None, launches=True):
    """One row on its buffers B.  launch(row) -> (rc, error text), synchronised.  check(outputs on the host by name) -> the distance on
    record (None counts as 0).  einval: the code a refusal must return (None: any non-zero code).  launches: False for an accepted row
    that must return 0 and touch nothing.  Returns the row's distance, or None for a row that launched nothing."""
    what = c["id"]
    before = {k: b.alloc.clone() for k, b in B.ins.items()}

    def inputs_unchanged(why):
        for k, b in B.ins.items():
            assert torch.equal(b.alloc, before[k]), (what, k, why)

    def run(steps):
        for i, row in enumerate(steps):
            rc, err = launch(row)
            assert rc == 0, (what, "declared accept, refused", rc, err)
            if i == 0 and len(steps) > 1 and B.between:
                B.between({name: b.get() for name, b in B.outs.items()})

    if c["answer"] == "refuse" or not launches:
        rc, err = launch(c)
        if c["answer"] != "refuse":
            assert rc == 0, (what, "a call that has nothing to do is OK", rc, err)
        elif einval is None:
            assert rc != 0 and err.strip(), (what, "declared refuse, launched", rc)
        else:
            assert rc == einval and err.strip(), (what, "declared refuse: the argument checks' code is {}, a launch that failed gives another".format(einval), rc, err)
        for name, b in B.outs.items():
            assert b.untouched(), (what, name, "written by a call that launches nothing")
        inputs_unchanged("changed by a call that launches nothing")
        return None
    steps = B.steps or [c]
    run(steps)
    for name, b in B.outs.items():
        assert b.outside_untouched(), (what, name, "written outside the output view or into a guard")
    inputs_unchanged("an input of the call changed")
    first = {name: b.region().clone() for name, b in B.outs.items()}
    d = check({name: b.get(first[name]) for name, b in B.outs.items()})
    if B.extra:
        B.extra(first)
    for again in [steps] + [[row] for row in B.again]:             # the same call again into fresh buffers
        for b in B.outs.values():
            b.reset()
        if B.regard:                                               # ... with another byte around an input: what the kernel read lay inside it
            B.ins[B.regard].reset(guard_fill=0xC3)
        run(again)
        for name, b in B.outs.items():
            assert torch.equal(b.region(), first[name]) and b.outside_untouched(), (what, name, "a second call gave other bits")
    return 0.0 if d is None else d


def run_rows(rows, run):
    """[run(c) for c in rows], where a row that misses its check does not hide the ones after it: the first line of every AssertionError
    is collected and raised at the end (a device error is no AssertionError and ends the test)."""
    failed, out = [], []
    for c in rows:
        try:
            out.append(run(c))
        except AssertionError as err:
            failed.append("{}: {}".format(c["id"], str(err).splitlines()[0] if str(err) else "assert"))
    assert not failed, "\n".join(["{} of {} rows failed".format(len(failed), len(rows))] + failed)
    return out


def run_entry(entry, rows, run, count="answer", report=True):
    """Every row of one entry point through run(c) -> distance | None, then the counts against the table: a row launches iff its answer is
    accept (count="answer") or iff it names kernels (count="kernels"), and both kinds exist.  report: print each distance and the largest."""
    dists = []

    def one(c):
        dists.append(run(c))
        if report and dists[-1] is not None:
            print("{}: {:.3e}".format(c["id"], dists[-1]))

    try:
        run_rows(rows, one)
    finally:
        if report:
            print("{}: largest distance on record {:.3e}".format(entry, max([0.0] + [d for d in dists if d is not None])))
    launched, quiet = sum(d is not None for d in dists), sum(d is None for d in dists)
    want = sum(c["answer"] == "accept" if count == "answer" else bool(c["kernels"]) for c in rows)
    assert launched == want and launched > 0
    assert quiet == len(rows) - want and quiet > 0


def fp32_bar(name, rows, distance, what="torch fp32", floor=0.0):
    """The project's recipe for a bar that no kernel has a say in: 4x the largest distance of torch's own fp32 CPU result from the float64
    one over `rows` (the table's accepted finite rows), distance(c) computing it from the references alone; never below `floor`."""
    worst = 0.0
    for c in rows:
        d = distance(c)
        print("{}: {} vs float64 {:.3e}".format(c["id"], what, d))
        worst = max(worst, d)
    assert worst > 0.0
    bar = max(floor, 4.0 * worst)
    print("{}: largest fp32 distance {:.3e}, bar {:.3e}".format(name, worst, bar))
    return bar


# ---------------------------------------------------------------------------------------------------------------
# without a GPU: the kernels of the sources and of the library, the census, the cells, the refusals
# ---------------------------------------------------------------------------------------------------------------
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


def claimed_kernels(cases):
    return {k for c in cases if c["answer"] == "accept" for k in c["kernels"]}


def assert_census(cases, files):
    """The kernels the accepted rows name, and those the census rows name, are exactly the kernels of `files` as the built library
    instantiates them.  No count is written down: whatever is missing on either side fails by name."""
    names = source_kernels(files)
    assert names, "no __global__ kernel found in the sources"
    kernels = library_kernels(names)
    assert {base(k) for k in kernels} == names, "kernels of the sources the library lacks: {}".format(sorted(names - {base(k) for k in kernels}))
    named = claimed_kernels(cases)
    assert named == kernels, "kernels no accepted row launches: {}; rows naming kernels the library lacks: {}".format(sorted(kernels - named), sorted(named - kernels))
    census = {k for c in cases if c["feature"] == "census" for k in c["kernels"]}
    assert census == kernels, "kernels without a census row: {}".format(sorted(kernels - census))


def assert_cells(cases, table, nullable=None):
    """The part of the cell check that every table shares: the rows span the table's entries and features, every (entry, feature) cell has
    a row or a reason and not both, ids name rows, a row is refused iff its feature is refuse, only a refused row is host-only, and every
    pointer of nullable[entry] has its NULL row."""
    assert {c["entry"] for c in cases} == set(table.ENTRIES) and {c["feature"] for c in cases} == set(table.FEATURES)
    cells = {(c["entry"], c["feature"]) for c in cases}
    assert set(table.N_A) <= {(e, f) for e in table.ENTRIES for f in table.FEATURES}
    for e in table.ENTRIES:
        for f in table.FEATURES:
            assert ((e, f) in cells) != ((e, f) in table.N_A), (e, f, "a cell has a row or a reason, not both and not neither")
    reasons = list(table.N_A.values()) + list(getattr(table, "PRECONDITIONS", {}).values())
    assert all(isinstance(v, str) and v.strip() for v in reasons)
    assert set(getattr(table, "PRECONDITIONS", {})) <= set(table.ENTRIES)
    assert len({c["id"] for c in cases}) == len(cases)                   # ids name rows
    for c in cases:
        assert c["answer"] in ("accept", "refuse") and (c["answer"] == "refuse") == (c["feature"] == "refuse"), c["id"]
        assert not c["kernels"] or c["answer"] == "accept", c["id"]
        assert not c["host_only"] or c["answer"] == "refuse", c["id"]
    for e in table.ENTRIES if nullable else ():
        nulled = {c["null"] for c in cases if c["entry"] == e and c["null"]}
        assert nulled >= set(nullable[e]), (e, sorted(set(nullable[e]) - nulled))


def assert_refused_before_launch(lib, table, entry, einval=None):
    """Every refused row of the entry point is refused on dummy aligned pointers, with an error text: every argument check sits before
    the launch.  einval: the code the argument checks return (a call that got as far as its launch returns another here: there is no
    device); None: any non-zero code."""
    buf = (ctypes.c_float * 256)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    rows = [c for c in table.all_cases() if c["entry"] == entry and c["answer"] == "refuse"]
    assert rows

    def one(c):
        rc = table.call(lib, c, table.dummy_pointers(c, ptr))
        err = lib.cmk_last_error().decode()
        assert rc != 0, (c["id"], "declared refuse, accepted")
        assert einval is None or rc == einval, (c["id"], "declared refuse, but the call went on to its launch", rc, err.strip())
        assert err.strip(), (c["id"], "refused without an error text")

    run_rows(rows, one)
