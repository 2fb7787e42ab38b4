"""One probe for the conv library: plan, time, check or loop conv problems of the model on chosen tile variants, through ops._ConvLaunch.

  python tools/conv_probe.py plan  --set pw -v 1/32/4 8/32/4 8/32/2              # host only: kernel, executed FLOPs, GroupNorm records or the refusal
  python tools/conv_probe.py time  --set v39 v99 roi --relu -v 6/16/roi 6/64/roi  # interleaved rounds, best of --rounds, `equal` to the first variant
  python tools/conv_probe.py time  --set tower --gn 32 --in-affine -v 6/16/1 6/64/1    # the five FCOS levels as ONE launch, conv + GroupNorm finalize
  python tools/conv_probe.py check --shape 1,1,400,1024,80,1,1 --relu --res add -v default 0/0/0/2 1/32/1/2     # error against float64, unwritten elements
  python tools/conv_probe.py loop  --row OSA2_x -v 6/64/1 --iters 3               # what a profiler wraps: launches and one synchronise, nothing else
  python tools/conv_probe.py time  --set small -v 11/2/1 --lib A.so B.so           # same-session A/B of library builds, one fresh child per (round, library)

Problems: rows of SHAPES by --set / --row, and --shape N,H,W,Cin,Cout,k,s (with --levels HxW,HxW,.. one launch of several maps).  The set
`tower` runs as one multi-problem launch; every other row is a launch of its own.

Variants: wm/sc/wn[/splitk[/tail]] as ops.Variant.of reads them (cmk.h: tune_wm, tune_sc, tune_wn).  `default` = zero tune fields, what
cmk_conv_resolve picks.  `tuned` = the problem's entry in the --table file (matched by k, stride, Cin, Cout, the residual slot and the
shapes; the strides of the model's concat buffers are ignored).  The wn field may be the word `roi`: 2 on rows of the set `roi`, 1 on every
other problem (the F(4x4) forms tile 14 x 14 RoI maps in pairs and feature maps in 12 x 40 tiles).  Variants with wm 10, 11 or 12 switch on
ops.ALLOW_SPLIT_BF16 / ALLOW_SPLIT_F16 before the weights are packed.

Data: seeded on the host (--seed): x ~ N(0,1), weights N(0,1) * sqrt(2 / (Cin k k)), the residual N(0,1), no scale or shift.

Faults: a refusal (the entry returns CMK_EINVAL before any launch) is recorded as n/a and the run goes on.  Any other non-zero return, a HIP
error text, or an exception from a synchronise ends the process at once with exit status 2: nothing more is launched.  With --lib every
child runs under --child-timeout seconds; the default is 60 s for start-up + 15 s per problem for its data, packing and first launches +
0.05 s per launch of a timing (rounds x (warm + iters) x variants x problems; the slowest launch of the table is under 5 ms).  A child that exits
non-zero, by a signal, or at the limit stops the driver: it prints what it has, starts no further child and exits 1.  No retries; one
child at a time."""
import argparse
import json
import os
import subprocess
import sys
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, R = 8, 400        # the bench batch; RoI maps of one step (8 images x 50)
SHAPES = [  # name, N, H, W, Cin, Cout, k, stride, sets
    ("stem_2", B, 400, 640, 64, 64, 3, 1, "v39"),
    ("OSA2_x", B, 200, 320, 128, 128, 3, 1, "v39 small"),
    ("OSA3_0", B, 100, 160, 256, 160, 3, 1, "v39 single"),
    ("OSA3_x", B, 100, 160, 160, 160, 3, 1, "v39 small"),
    ("OSA3_2_0", B, 100, 160, 512, 160, 3, 1, "v99"),                 # V-99 alone: the first conv of a stage-3 block after the first
    ("OSA4_0", B, 50, 80, 512, 192, 3, 1, "v39 single"),
    ("OSA4_x", B, 50, 80, 192, 192, 3, 1, "v39 single"),
    ("OSA4_2_0", B, 50, 80, 768, 192, 3, 1, "v39 single"),
    ("OSA5_0", B, 25, 40, 768, 224, 3, 1, "v39 single"),
    ("OSA5_x", B, 25, 40, 224, 224, 3, 1, "v39 single"),
    ("OSA5_2_0", B, 25, 40, 1024, 224, 3, 1, "v39 single"),
    ("fpn_p3", B, 100, 160, 256, 256, 3, 1, "v39 small tower"),       # also fcos_p3: the FPN output conv and a tower conv at P3 are one problem
    ("fpn_p4", B, 50, 80, 256, 256, 3, 1, "v39 single small tower"),  # also fcos_p4
    ("fpn_p5", B, 25, 40, 256, 256, 3, 1, "v39 single small tower"),  # also fcos_p5
    ("p6", B, 13, 20, 256, 256, 3, 1, "small tower"),
    ("p7", B, 7, 10, 256, 256, 3, 1, "tower"),
    ("cls_p3", B, 100, 160, 256, 80, 3, 1, "v39"),
    ("c256_p3", B, 100, 160, 256, 128, 3, 1, "extra"),               # two shapes outside the model, from the split-product 3x3 study
    ("c512", B, 50, 80, 512, 256, 3, 1, "extra"),
    ("roi", R, 14, 14, 256, 256, 3, 1, "roi small"),
    ("roi272", R, 14, 14, 272, 256, 3, 1, "roi"),                     # mask head conv 1 with the spatial-attention channels
    ("OSA2_cat", B, 200, 320, 768, 256, 1, 1, "pw"),
    ("OSA3_cat", B, 100, 160, 1056, 512, 1, 1, "pw"),
    ("OSA3_cat1", B, 100, 160, 1312, 512, 1, 1, "pw v99"),
    ("OSA4_cat0", B, 50, 80, 1472, 768, 1, 1, "pw"),                  # also OSA4_cat
    ("OSA4_cat1", B, 50, 80, 1728, 768, 1, 1, "pw"),                  # also OSA4_2cat
    ("OSA5_cat0", B, 25, 40, 1888, 1024, 1, 1, "pw"),                 # also OSA5_cat (of the split-product study)
    ("OSA5_cat1", B, 25, 40, 2144, 1024, 1, 1, "pw"),                 # also OSA5_cat (of the first conv benchmark)
    ("fpn_lat3", B, 100, 160, 512, 256, 1, 1, "pw"),                  # also lat3
    ("fpn_lat4", B, 50, 80, 768, 256, 1, 1, "pw"),
    ("fpn_lat5", B, 25, 40, 1024, 256, 1, 1, "pw"),
    ("deconv", R, 14, 14, 256, 1024, 1, 1, "pw roi"),                 # the mask head's 2x2 deconv as a GEMM
    ("miou_fc1", 1, 1, R, 12544, 1024, 1, 1, "fc"),                   # the fully connected layers: 400 rows as 1 x 400 pixels
    ("miou_fc2", 1, 1, R, 1024, 1024, 1, 1, "fc"),
    ("miou_out", 1, 1, R, 1024, 80, 1, 1, "fc"),
    ("stem_3", B, 400, 640, 64, 128, 3, 2, "s2"),
    ("miou_c4", R, 14, 14, 256, 256, 3, 2, "s2 roi"),
    ("p6_down", B, 25, 40, 256, 256, 3, 2, "s2"),                     # also p6 (of the stride-2 study): P5 -> P6
    ("p7_down", B, 13, 20, 256, 256, 3, 2, "s2"),
]
ONE_LAUNCH = ("tower",)          # sets whose rows are the problems of ONE launch (cmk_conv2d_nhwc_multi), in table order
SETS = sorted({s for row in SHAPES for s in row[8].split()})
DEFAULT_TABLE = os.path.join(ROOT, "centermask2_amd", "tuned", "mi355x_V-39-eSE_b8_800x1280.json")
EINVAL = -1                      # cmk.h CMK_EINVAL: refused at the front door, nothing launched


class Problem(NamedTuple):
    name: str
    shapes: tuple        # ((N, H, W), ...): more than one = one multi-problem launch
    cin: int
    cout: int
    k: int
    stride: int
    sets: tuple = ()

    @property
    def flops(self):
        """Algorithmic FLOPs: 2 x output pixels x Cin x Cout x taps."""
        pix = sum(n * (h if self.stride == 1 else (h - 1) // 2 + 1) * (w if self.stride == 1 else (w - 1) // 2 + 1) for n, h, w in self.shapes)
        return 2.0 * pix * self.cin * self.cout * self.k * self.k


class Fault(Exception):
    """A launch that failed otherwise than by a refusal: the process launches nothing more."""


def rows(sets=(), names=()):
    """The problems of these sets and row names, in table order, each once; a set of ONE_LAUNCH gives one problem of all its rows."""
    unknown = [s for s in sets if s not in SETS] + [n for n in names if n not in {r[0] for r in SHAPES}]
    if unknown:
        raise SystemExit("conv_probe: unknown set or row {} (sets: {})".format(unknown, " ".join(SETS)))
    out = []
    for s in sets:
        if s in ONE_LAUNCH:
            mine = [r for r in SHAPES if s in r[8].split()]
            assert len({r[4:8] for r in mine}) == 1, s
            out.append(Problem(s, tuple(r[1:4] for r in mine), *mine[0][4:8], sets=(s,)))
    for r in SHAPES:
        tags = r[8].split()
        if r[0] in names or any(s in tags for s in sets if s not in ONE_LAUNCH):
            out.append(Problem(r[0], (r[1:4],), *r[4:8], sets=tuple(tags)))
    return out


def explicit(shape, levels):
    """--shape N,H,W,Cin,Cout,k,s [--levels HxW,..] as a problem."""
    n, h, w, cin, cout, k, s = (int(v) for v in shape.split(","))
    hw = [tuple(int(v) for v in lv.split("x")) for lv in levels.split(",")] if levels else [(h, w)]
    return Problem("{}x{}x{}{}_{}-{}_k{}s{}".format(n, hw[0][0], hw[0][1], "+{}".format(len(hw) - 1) if len(hw) > 1 else "", cin, cout, k, s),
                   tuple((n, a, b) for a, b in hw), cin, cout, k, s)


def spell(v):
    """A Variant as wm/sc/wn[/splitk[/tail]]."""
    from centermask2_amd.ops import Variant
    return "/".join(str(f) for f in Variant.of(v).stored())


def parse_variant(text, p, table=None, res_slot=0):
    """The Variant a spelling means on problem p, or a str saying why there is none (`tuned` without an entry)."""
    from centermask2_amd import ops
    if text == "default":
        return ops.Variant(0, 0, 0)
    if text == "tuned":
        for key in sorted(table or {}):
            k, stride, cin, cout, _, _, res, shapes = ops._str_to_key(key)
            if (k, stride, cin, cout, res, shapes) == (p.k, p.stride, (p.cin + 15) // 16 * 16, p.cout, res_slot, tuple(p.shapes)):
                return ops.Variant.of(table[key])
        return "no entry in the table"
    f = text.split("/")
    if not 3 <= len(f) <= 5:
        raise SystemExit("conv_probe: variant {!r} is not wm/sc/wn[/splitk[/tail]], default or tuned".format(text))
    if f[2] == "roi":
        f[2] = 2 if "roi" in p.sets else 1
    return ops.Variant.of(tuple(int(x) for x in f))


def refusal(rc, lib):
    """None for a launch that went out; the library's message for a refusal; raises Fault for anything else."""
    if rc == 0:
        return None
    msg = lib.cmk_last_error().decode()
    if rc == EINVAL and "hip" not in msg:
        return msg
    raise Fault("rc {}: {}".format(rc, msg))


def synchronise():
    import torch
    try:
        torch.cuda.synchronize()
    except Exception as e:
        raise Fault("synchronise: {}".format(e))


# ---------------------------------------------------------------------------------------------------------------
# problems on the device
# ---------------------------------------------------------------------------------------------------------------
class Buffers:
    """The seeded tensors of one problem: inputs, packed weights, and per variant a launch with outputs of its own."""

    def __init__(self, p, a, dev):
        import torch
        from centermask2_amd import ops
        g = torch.Generator().manual_seed(a.seed)
        self.p, self.a, self.dev = p, a, dev
        cin_pad = (p.cin + 15) // 16 * 16
        self.x_host = [torch.randn((n, p.cin, h, w), generator=g) for n, h, w in p.shapes]
        self.w_host = torch.randn((p.cout, p.cin, p.k, p.k), generator=g) * (2.0 / (p.cin * p.k * p.k)) ** 0.5
        self.out_shapes = [(n,) + ops._out_hw(h, w, p.stride) for n, h, w in p.shapes]
        self.res_host = None
        if a.res:
            n, ho, wo = self.out_shapes[0]
            self.res_host = torch.randn((n, p.cout, ho, wo) if a.res == "add" else (n, p.cout, (ho + 1) // 2, (wo + 1) // 2), generator=g)
        self.aff_host = [(torch.rand((n, cin_pad), generator=g) + 0.5, torch.randn((n, cin_pad), generator=g) * 0.1) for n, _, _ in p.shapes] if a.in_affine else None
        self.xs = []
        for x in self.x_host:
            t = torch.zeros((x.shape[0], x.shape[2], x.shape[3], cin_pad), device=dev)
            t[..., :p.cin] = x.to(dev).permute(0, 2, 3, 1)
            self.xs.append(ops.View(t))
        self.pc = ops.PackedConv(self.w_host, None, None, dev, stride=p.stride)
        self.res = ops.as_view(self.res_host.to(dev)) if a.res else None
        self.aff = [(s.to(dev), t.to(dev)) for s, t in self.aff_host] if a.in_affine else None
        self.gamma, self.beta = torch.ones(p.cout, device=dev), torch.zeros(p.cout, device=dev)

    def launch(self, v):
        """A _ConvLaunch on NaN-filled outputs of its own with variant v set; .affine: the fused GroupNorm records' finalize, or None."""
        import torch
        from centermask2_amd import ops
        p, a = self.p, self.a
        ys = [ops.View(torch.full(s + (p.cout,), float("nan"), device=self.dev)) for s in self.out_shapes]
        single = len(p.shapes) == 1 and not a.gn
        L = ops._ConvLaunch(self.xs, [self.pc] * len(ys), ys, relu=a.relu, res=self.res, res_upsample=a.res == "upsample", in_affine=self.aff, single=single)
        L.set(v)
        L.affine = L.gn_stats(a.gn) if a.gn else None
        return L

    def go(self, L):
        """One launch (and the GroupNorm finalize of its records); returns (refusal text or None, the affines)."""
        from centermask2_amd import _lib
        why = refusal(L.run(), _lib.load())
        if why is None and L.affine is not None:
            return None, L.affine(0, L.n, self.gamma, self.beta, 1e-5)
        return why, None

    def timed(self, L, iters, what):
        """Milliseconds per launch over `iters` launches between two device events, ending in a synchronise."""
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(self.a.warm + iters):         # --warm untimed launches right ahead: every timing starts on a busy device
            if i == self.a.warm:
                e0.record()
            why = self.go(L)[0]
            if why is not None:
                raise Fault("{} {}: refused after it had launched: {}".format(self.p.name, what, why))
        e1.record()
        try:
            e1.synchronize()
        except Exception as e:
            raise Fault("synchronise: {}".format(e))
        return e0.elapsed_time(e1) / iters

    def reference(self):
        """Outputs (N, Ho, Wo, Cout) per problem computed on the host in --ref precision, as float64."""
        import torch
        import torch.nn.functional as F
        p, a, out, dt = self.p, self.a, [], getattr(torch, self.a.ref)
        for i, x in enumerate(self.x_host):
            x = x.to(dt)
            if a.in_affine:
                s, t = self.aff_host[i]
                x = (x * s[:, :p.cin].to(dt)[:, :, None, None] + t[:, :p.cin].to(dt)[:, :, None, None]).relu()
            y = F.conv2d(x, self.w_host.to(dt), None, stride=p.stride, padding=p.k // 2)
            if a.res:
                r = self.res_host.to(dt)
                y = y + (r if a.res == "add" else F.interpolate(r, scale_factor=2, mode="nearest")[:, :, :y.shape[2], :y.shape[3]])
            out.append((y.relu() if a.relu else y).permute(0, 2, 3, 1).double().contiguous())
        return out


def _setup(a, gpu=True):
    """(device, the `tuned` table, the residual slot of a problem key) of a run; switches the opt-in packings on where a variant needs them."""
    import torch
    from centermask2_amd import ops
    if gpu and not torch.cuda.is_available():
        raise SystemExit("conv_probe {}: needs a GPU (plan runs without one)".format(a.mode))
    if a.res and any(len(p.shapes) > 1 for p in a.problems):
        raise SystemExit("conv_probe: --res goes with single-problem launches")
    if any(t.split("/")[0] in ("10", "11", "12") for t in a.variants):
        ops.ALLOW_SPLIT_BF16 = ops.ALLOW_SPLIT_F16 = True          # the opt-in split forms need their packing
    table = None
    if "tuned" in a.variants:
        with open(a.table) as f:
            table = json.load(f)
    return torch.device("cuda", torch.cuda.current_device()) if gpu else None, table, {None: 0, "add": 1, "upsample": 2}[a.res] + (4 if a.in_affine else 0)


# ---------------------------------------------------------------------------------------------------------------
# modes
# ---------------------------------------------------------------------------------------------------------------
def plan(a):
    """Host only: what the library would launch, per (problem, variant)."""
    from centermask2_amd import _lib, ops
    (_, table, slot), out = _setup(a, gpu=False), []
    print("%-12s %-12s %-44s %10s  %s" % ("problem", "variant", "kernel", "exe GFLOP", "GroupNorm records"), flush=True)
    for p in a.problems:
        for text in a.variants:
            v = parse_variant(text, p, table, slot)
            row = dict(problem=p.name, variant=text)
            if isinstance(v, str):
                row["refused"] = v
            else:
                L = ops._ConvLaunch.planned(p.shapes, p.cin, p.cout, p.k, p.stride, relu=a.relu, res_mode=slot & 3, in_affine=a.in_affine,
                                            single=len(p.shapes) == 1 and not a.gn)
                L.set(v)
                if a.gn:
                    L.gn_stats(a.gn)
                try:
                    row["kernel"], row["flops"], row["gn_records"] = ops._plan(L.descs, L.n)
                except _lib.CmkError:
                    row["refused"] = _lib.load().cmk_last_error().decode()
            out.append(row)
            print("%-12s %-12s " % (p.name, text) + ("n/a: " + row["refused"] if "refused" in row else "%-44s %10.2f  %s" % (
                row["kernel"], row["flops"] / 1e9, row["gn_records"] if any(row["gn_records"]) else "-")), flush=True)
    return 0, out


def time_(a):
    """Best of --rounds interleaved rounds of --iters launches per (problem, variant); `eq`: the output has the first variant's bits."""
    import torch
    from centermask2_amd import ops
    (dev, table, slot), out, total = _setup(a), [], [0.0] * len(a.variants)
    print("%-12s " % "problem" + " ".join("%30s" % ("%s ms algTF exeTF ratio eq" % t) for t in a.variants), flush=True)
    for p in a.problems:
        buf, cells, first = Buffers(p, a, dev), [], None
        for text in a.variants:                      # warm-up: every (problem, variant) once; the return of this launch says whether it applies
            v = parse_variant(text, p, table, slot)
            c = dict(refused=v) if isinstance(v, str) else dict(L=buf.launch(v))
            if "L" in c:
                c["refused"], aff = buf.go(c["L"])
                synchronise()
            if c["refused"] is None:
                L = c["L"]
                first = first or (L, aff)
                c["kernel"], c["exe_flops"], _ = ops._plan(L.descs, L.n)
                c["equal"] = all(torch.equal(y.t, y0.t) for y, y0 in zip(L.ys, first[0].ys))
                c["maxdiff"] = max(float((y.t - y0.t).abs().max()) for y, y0 in zip(L.ys, first[0].ys))
                if aff is not None and first[1] is not None:
                    c["affines_equal"] = all(torch.equal(s, s0) and torch.equal(t, t0) for (s, t), (s0, t0) in zip(aff, first[1]))
                c["outputs"] = [y.t for y in L.ys] if a.keep else None
            cells.append(c)
        for _ in range(a.rounds):
            for c, text in zip(cells, a.variants):
                if c["refused"] is None:
                    c["ms"] = min(c.get("ms", float("inf")), buf.timed(c["L"], a.iters, text))
        ref = next((c["ms"] for c in cells if "ms" in c), None)
        line = "%-12s " % p.name
        for k, c in enumerate(cells):
            total[k] += c.get("ms", 0.0)
            line += "%30s " % "n/a" if "ms" not in c else "%9.3f %6.1f %6.1f %5.2f %s " % (
                c["ms"], p.flops / c["ms"] / 1e9, c["exe_flops"] / c["ms"] / 1e9, ref / c["ms"], "yes" if c["equal"] else " no")
        line += "  max|diff| vs first " + " ".join("%.1e" % c["maxdiff"] if "ms" in c else "n/a" for c in cells)
        print(line + ("   affines equal " + " ".join(str(c.get("affines_equal")) for c in cells) if a.gn else ""), flush=True)
        for c, text in zip(cells, a.variants):
            if c["refused"] is not None:
                print("  %s n/a: %s" % (text, c["refused"]), flush=True)
        out.append(dict({key: [c.get(key) for c in cells] for key in ("refused", "ms", "equal", "maxdiff", "affines_equal", "kernel", "exe_flops", "outputs")}, problem=p.name))
        del buf, cells, first
    print("%-12s " % "sum" + " ".join("%9.3f %20s" % (t, "") for t in total), flush=True)
    print("RESULT " + json.dumps({r["problem"]: r["ms"] for r in out}), flush=True)
    return 0, out


def check(a):
    """Max abs and normalised error of each variant against a float64 convolution on the host (--ref float32: torch's own fp32 one);
    unwritten elements of the NaN-filled output; the channels of the first bad elements; --reps: run-to-run differences."""
    import torch
    (dev, table, slot), out = _setup(a), []
    for p in a.problems:
        buf = Buffers(p, a, dev)
        ref = [r[:a.images] if a.images else r for r in buf.reference()]
        mag = max(float(r.abs().max()) for r in ref)
        print("%s: max|ref| %.3f" % (p.name, mag), flush=True)
        for text in a.variants:
            v = parse_variant(text, p, table, slot)
            row, errs, bits = dict(problem=p.name, variant=text, max_ref=mag), [], []
            if isinstance(v, str):
                row["refused"] = v
            else:
                L = buf.launch(v)
                for rep in range(a.reps):
                    for y in L.ys:
                        y.t.fill_(float("nan"))
                    why, _aff = buf.go(L)
                    if why is not None:
                        row["refused"] = why
                        break
                    synchronise()
                    diff = [y.t[:r.shape[0]].double().cpu() - r for y, r in zip(L.ys, ref)]
                    errs.append(max(float(d.nan_to_num(nan=float("inf")).abs().max()) for d in diff))
                    bits.append([y.t.clone() for y in L.ys] if a.reps > 1 else None)
            if "refused" in row:
                print("  %-12s n/a: %s" % (text, row["refused"]), flush=True)
            else:
                err = torch.cat([d.reshape(-1, p.cout) for d in diff]).abs()
                bad = err > a.bad
                row.update(max_abs=errs[-1], normalised=errs[-1] / max(1.0, mag), rms=float(err.nan_to_num(nan=0.0).pow(2).mean().sqrt()), per_rep=errs,
                           unwritten=sum(int(torch.isnan(y.t).sum()) for y in L.ys), bad=int(bad.sum()), bad_channels=sorted(set(torch.nonzero(bad)[:, 1].tolist()))[:12],
                           reps_equal=all(torch.equal(x, y) for b in bits[1:] for x, y in zip(b, bits[0])) if a.reps > 1 else None)
                if a.keep:
                    row["diff"], row["ref"] = diff, ref
                print("  %-12s max abs err %.3e  normalised %.3e  rms %.2e  unwritten %d  bad (> %g) %d of %d%s%s" % (
                    text, row["max_abs"], row["normalised"], row["rms"], row["unwritten"], a.bad, row["bad"], err.numel(),
                    "  channels {}".format(row["bad_channels"]) if row["bad"] else "",
                    "  per rep {} same bits {}".format(["%.2e" % e for e in errs], row["reps_equal"]) if a.reps > 1 else ""), flush=True)
            out.append(row)
        del buf
    return 0, out


def loop(a):
    """--iters launches of ONE (problem, variant) and a synchronise."""
    dev, table, slot = _setup(a)
    if len(a.problems) != 1 or len(a.variants) != 1:
        raise SystemExit("conv_probe loop: one problem and one variant")
    p, text = a.problems[0], a.variants[0]
    buf = Buffers(p, a, dev)
    v = parse_variant(text, p, table, slot)
    why = v if isinstance(v, str) else None
    L = None if why else buf.launch(v)
    for _ in range(0 if why else a.iters):
        why = why or buf.go(L)[0]
    synchronise()
    print("%s %s: %s" % (p.name, text, "n/a: " + why if why else "%d launches" % a.iters), flush=True)
    return int(why is not None), []


# ---------------------------------------------------------------------------------------------------------------
# --lib: same-session A/B of library builds
# ---------------------------------------------------------------------------------------------------------------
def run_child(cmd, timeout):
    """Start ONE child, wait for it under the time limit.  Returns (ok, the times of its RESULT line or None, what to print when not ok)."""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return False, None, "no answer within {:g} s: killed".format(timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        return False, None, "exit status {}{}\n{}\n{}".format(r.returncode, " (signal {})".format(-r.returncode) if r.returncode < 0 else "",
                                                             r.stdout[-600:], r.stderr[-1200:])
    return True, json.loads(lines[-1][len("RESULT "):]), ""


def ab(libs, rounds, child_cmd, timeout):
    """One fresh child per (round, library), alternating A, B, A, B; best of rounds per problem and library.  Stops at the first child that
    did not end well: prints what it has and returns 1."""
    times, status = {lib: {} for lib in libs}, 0
    for r in range(rounds):
        for lib in libs:
            ok, res, why = run_child(child_cmd(lib), timeout)
            if not ok:
                print("conv_probe: round {} of {}: {}\nno further child is started".format(r + 1, lib, why), flush=True)
                status = 1
                break
            for name, ms in res.items():
                old = times[lib].get(name)
                times[lib][name] = ms if old is None else [m if o is None else o if m is None else min(o, m) for o, m in zip(old, ms)]
        if status:
            break
    for lib in libs:
        cells = ["%s %s" % (name, "/".join("n/a" if m is None else "%.3f" % m for m in ms)) for name, ms in times[lib].items()]
        sums = [sum(ms[k] or 0.0 for ms in times[lib].values()) for k in range(len(next(iter(times[lib].values()), [])))]
        print("%-28s %s | sum %s" % (os.path.basename(lib), " ".join(cells), "/".join("%.3f" % s for s in sums)), flush=True)
    return status, times


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], epilog="sets: " + " ".join(SETS))
    ap.add_argument("mode", choices=("plan", "time", "check", "loop"))
    ap.add_argument("--set", nargs="+", default=[], dest="sets", help="rows of the shape table by set")
    ap.add_argument("--row", nargs="+", default=[], help="rows of the shape table by name")
    ap.add_argument("--shape", action="append", default=[], help="N,H,W,Cin,Cout,k,s: an explicit problem")
    ap.add_argument("--levels", help="HxW,HxW,..: the maps of the --shape problem, one multi-problem launch")
    ap.add_argument("-v", "--variants", nargs="+", default=["default"], help="wm/sc/wn[/splitk[/tail]] | default | tuned")
    ap.add_argument("--table", default=DEFAULT_TABLE, help="the table `tuned` reads")
    ap.add_argument("--relu", action="store_true")
    ap.add_argument("--res", choices=("add", "upsample"))
    ap.add_argument("--in-affine", action="store_true", help="the producer's GroupNorm + ReLU fused into the input staging")
    ap.add_argument("--gn", type=int, default=0, metavar="GROUPS", help="fused GroupNorm statistics of the output and their finalize")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="launches per timing (time), launches in all (loop)")
    ap.add_argument("--warm", type=int, default=10, help="time: untimed launches right ahead of every timing")
    ap.add_argument("--reps", type=int, default=1, help="check: repeat the launch, report run-to-run differences")
    ap.add_argument("--images", type=int, default=0, help="check: compare only the first K images of every output (0 = all)")
    ap.add_argument("--ref", choices=("float64", "float32"), default="float64", help="check: the precision of the host reference")
    ap.add_argument("--bad", type=float, default=1e-3, help="check: the error above which an element is listed as bad")
    ap.add_argument("--lib", nargs="+", default=[], help="time: library builds to compare, one child per (round, library)")
    ap.add_argument("--child-timeout", type=float, default=0.0, help="seconds per child (0 = sized from the work, see the docstring)")
    ap.add_argument("--child-lib", help=argparse.SUPPRESS)
    return ap


def main(argv=None, keep=False):
    """Returns (exit status, results).  keep: results carry the output and error tensors (in-process callers)."""
    a = parser().parse_args(argv)
    a.keep = keep
    a.problems = rows(a.sets, a.row) + [explicit(s, a.levels) for s in a.shape]
    if not a.problems:
        raise SystemExit("conv_probe: no problem given (--set, --row or --shape)")
    if a.lib:
        if a.mode != "time":
            raise SystemExit("conv_probe: --lib goes with time")
        argv = list(sys.argv[1:] if argv is None else argv)
        cut = argv.index("--lib")
        rest = argv[:cut] + [x for x in argv[cut + 1 + len(a.lib):]]
        timeout = a.child_timeout or 60.0 + 15.0 * len(a.problems) + 0.05 * (a.warm + a.iters) * len(a.variants) * len(a.problems)
        cmd = lambda lib: [sys.executable, os.path.abspath(__file__)] + rest + ["--rounds", "1", "--child-lib", os.path.abspath(lib)]
        return ab(a.lib, a.rounds, cmd, timeout)
    if a.child_lib:
        from centermask2_amd import _lib
        _lib.LIB_PATH = a.child_lib                     # before ops is imported
    from centermask2_amd import ops
    allow = ops.ALLOW_SPLIT_BF16, ops.ALLOW_SPLIT_F16
    try:
        return {"plan": plan, "time": time_, "check": check, "loop": loop}[a.mode](a)
    finally:
        ops.ALLOW_SPLIT_BF16, ops.ALLOW_SPLIT_F16 = allow          # in-process callers get their switches back


if __name__ == "__main__":
    try:
        sys.exit(main()[0])
    except Fault as e:
        print("conv_probe: FAULT, nothing more is launched: {}".format(e), flush=True)
        sys.exit(2)
