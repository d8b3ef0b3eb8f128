"""The purpose-built kernels' sweep, child process: ``python conv_special_child.py <table> <records.jsonl>``.

Runs every case of one table through ``kernels.ConvOp``, compares every result with the operand-exact reference
(tests/conv_exact_ref.py) and writes one JSON line per operation: case, operation, precision, ``last_kernel()`` (the launch tag),
whether the intended kernel took it and ``fallback_count()`` stood still, the checks (error, ``e32``, bound, the project's old
bound).  Several switches are read once per process (PCUDA_WGRAD3R, PCUDA_W3_MINCOUT), which is why every table is a process
of its own (tests/test_conv_special_gpu.py starts them one after the other).  Stops at the first HIP error and exits non-zero.

``_check``, ``_check_sums``, ``_dev``, ``_empty`` are those of tests/conv_variant_child.py.

Tables (the switch set of each in TABLES):
  ap_rs           conv3ap_kernel (csrc/conv_ap_impl.h) and conv3rs_kernel (csrc/conv_rs.hip): bf16x3 only (ap_layer_ok / rs_layer_ok);
                  small maps on the kernels through the test switches the kernel tests use
  w3_w1_direct    wgrad3_kernel (PCUDA_W3_MINCOUT=64: one 64-row tile in all), wgrad1, every direct kernel; PCUDA_WGRAD3R at its
                  default, which leaves maps below 64 rows to wgrad3
  w3r             wgrad3r_kernel behind PCUDA_WGRAD3R=2 (every eligible layer)
All tensors are aligned: these kernels refuse other views, and every operation asserts that the refusal path was NOT taken.  The
one kernel that takes another view (d1_dgrad_kernel reads its gradient dword by dword and checks its destination only) gets the
gradient one float behind the alignment.
"""
import json
import os
import re
import sys
import time
import traceback

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import conv_exact_ref as R  # noqa: E402
from conv_variant_child import _check, _check_sums, _dev, _empty  # noqa: E402

SLOPE = 0.2
SUM_TOL = 1e-3          # the kernel tests' bound on the BatchNorm partial sums (test_conv_ap_gpu.py, test_conv_rs_gpu.py)
NAN = float("nan")
SMALL = {"PCUDA_AP_MIN_ITEMS": "0", "PCUDA_RS_MIN_ROWS": "2", "PCUDA_RS_MIN_ITEMS": "0"}
TABLES = {
    "ap_rs": dict(SMALL),
    "w3_w1_direct": dict(SMALL, PCUDA_W3_MINCOUT="64"),
    "w3r": dict(SMALL, PCUDA_WGRAD3R="2"),
}


# ------------------------------------------------------------------------------------------ instantiation from tag + precision
def inst_of(tag, prec):
    """the template instantiation a launch tag (+ the precision) names, or None: the ids of test_conv_special_gpu.INSTANTIATIONS"""
    t = tag.split(" | ")[0]
    m = re.match(r"conv3rs .* stats(\d) acc(\d) aff(\d) ", t)
    if m and prec == "bf16x3":
        return "conv3rs-stats%s-acc%s-aff%s" % m.groups()
    m = re.match(r"conv3ap .* up\d fold(\d) stats(\d) acc(\d) ", t)
    if m and prec == "bf16x3":
        return "conv3ap-stats%s-acc%s-fold%s" % (m.group(2), m.group(3), m.group(1))
    m = re.match(r"wgrad3r .* up(\d) slices", t)
    if m:
        return "wgrad3r-%s-up%s" % (prec, m.group(1))
    if t.startswith("wgrad3 "):
        return "wgrad3-%s" % prec
    m = re.match(r"wgrad1 .* tile(\d+)x(\d+)$", t)
    if m:
        return "wgrad1-%s-co%d-ci%d" % (prec, int(m.group(1)) // 32, int(m.group(2)) // 32)
    m = re.match(r"direct (c1 fwd|c1 wgrad|1x1 fwd|1x1 dgrad\+bnred|1x1 dgrad|d1 dgrad|d1 wgrad|d5 fwd|d1 fwd \(mfma\)) ", t)
    if m:
        return "direct-%s-%s" % (m.group(1).replace(" (mfma)", "").replace(" ", "-"), prec)
    return None


def tag_int(tag, name):
    m = re.search(r" %s(\d+)" % name, tag)
    return int(m.group(1)) if m else None


# ------------------------------------------------------------------------------------------ data
class Data:
    """one case's tensors (CPU, float32) and memoised references"""

    def __init__(self, seed, n, c1, c2, cout, h, w, k, stride=1, pad=None, up=False):
        self.n, self.c1, self.c2, self.cin, self.cout = n, c1, c2, c1 + c2, cout
        pad = k // 2 if pad is None else pad
        self.g = g = R.Geom(n, c1 + c2, cout, h, w, k, stride, pad, 1, up)
        rng = np.random.default_rng(seed)
        t = lambda *sh, sd=1.0, mu=0.0: torch.from_numpy(rng.normal(mu, sd, sh).astype(np.float32))
        sh_, sw_ = (h // 2, w // 2) if up else (h, w)
        self.x1 = t(n, c1, sh_, sw_)
        self.x2 = t(n, c2, sh_, sw_) if c2 else None
        # the lazy-BatchNorm affine of source 1: shifts far from zero (a border padded before the affine would carry them)
        self.sc, self.sh = t(c1, sd=0.3, mu=1.0), t(c1, sd=0.3, mu=1.5)
        self.w, self.b = t(cout, self.cin, k, k, sd=0.1), t(cout, sd=0.1)
        self.dz = t(n, cout, g.oh, g.ow)
        self.scz, self.shz = t(cout, sd=0.3, mu=1.0), t(cout, sd=0.3, mu=1.5)      # (an affine on the gradient: conv3rs AFF dgrads)
        self.base = t(n, self.cin, h, w)
        self.a = t(n, self.cin, h, w)
        self.a_half = t(n, self.cin, sh_, sw_)
        self.mean = t(self.cin, sd=0.3)
        self.invstd = torch.from_numpy(rng.uniform(0.5, 2.0, (self.cin,)).astype(np.float32))
        self.base_w, self.base_b = t(cout, self.cin, k, k), t(cout)
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def xop(self, aff):
        """the operand of the forward / weight gradient: cat(affine(x1), x2)"""
        return self.memo(("xop", aff), lambda: R.source_operand(self.x1, self.sc if aff else None, self.sh if aff else None, self.x2))

    def zop(self, aff):
        return self.memo(("zop", aff), lambda: R.affine_operand(self.dz, self.scz if aff else None, self.shz if aff else None))


class Op:
    """one operation: name, precision, the substrings its launch tag must carry, thunk -> checks"""

    def __init__(self, name, prec, want, thunk, note=""):
        self.name, self.prec, self.want, self.thunk, self.note = name, prec, want, thunk, note


def _sums_of(red):
    part, nt = red
    return part[:nt].double().sum(0).cpu()


def _src(K, d, dev, aff):
    x1 = d.x1.to(dev)
    s = K.TA(x1, d.sc.to(dev), d.sh.to(dev)) if aff else x1
    return s, (d.x2.to(dev) if d.x2 is not None else None)


def _ta_with_shape(K):
    """``ConvOp.dgrad`` reads ``dy.shape`` / ``dy.device`` and hands dy to ``make_src``, which takes a TA: a TA that answers both
    reaches the C ABI's affine on the gradient (``pcuda_src.scale1`` of ``pcuda_conv2d_dgrad``: conv3rs<.., .., AFF = true> behind
    a data gradient), which no caller in the package uses"""
    class ShapedTA(K.TA):
        __slots__ = ()
        shape = property(lambda self: self.t.shape)
        device = property(lambda self: self.t.device)
    return ShapedTA


# ------------------------------------------------------------------------------------------ forward / data gradient (MFMA kernels)
def conv_ops(K, dev, d, prec, kern, fwd=(), dgrad=(), fold=(), model="mfma", bprec="same", mis_dy=0):
    """fwd: (aff, stats) pairs; dgrad: (aff, acc, bnred, split) tuples; fold: bnred flags.  kern: the tag's first word(s).
    bprec: the precision of the bound (None: one chain -- the direct kernels)"""
    g = d.g
    bp = prec if bprec == "same" else bprec
    old = R.OLD_TOL[prec]
    op = K.ConvOp(g.cin, g.cout, g.k, stride=g.stride, pad=g.pad, in_up=g.in_up)
    wd, bd = d.w.to(dev), d.b.to(dev)
    st = K.BNState()
    st.mean, st.invstd = d.mean.to(dev), d.invstd.to(dev)

    def fwd_ref(aff, pr, dt):
        return d.memo(("fwd", aff, pr, dt, model), lambda: R.forward_ref(g, d.xop(aff), d.w, d.b, SLOPE, pr, dt, model=model))

    def dg_ref(aff, pr, dt):
        return d.memo(("dg", aff, pr, dt, model), lambda: R.dgrad_ref(g, d.zop(aff), d.w, pr, dt, model=model))

    for aff, stats in fwd:
        def f(aff=aff, stats=stats):
            s, x2 = _src(K, d, dev, aff)
            out = _empty((g.n, g.cout, g.oh, g.ow), dev, 0, NAN)
            y, part, nt = op.forward(s, wd, bd, SLOPE, g.h, g.w, x2=x2, out=out, want_stats=stats)
            ref_old = fwd_ref(aff, None, torch.float64)
            chk = [_check("y", y, lambda dt: fwd_ref(aff, prec, dt), ref_old, bp, old_tol=old)]
            if stats:
                got = _sums_of((part, nt))
                o = R.bn_fwd_sums(ref_old)
                for i, nm in enumerate(("sum y", "sum y^2")):
                    chk.append(_check_sums(nm, got[:, i], lambda dt, i=i: R.bn_fwd_sums(fwd_ref(aff, prec, dt), dt)[i], o[i], max(SUM_TOL, old * 10), bp))
            return chk
        want = [kern + " "]
        if kern.startswith("conv3rs"):
            want += [" stats%d acc0 aff%d " % (int(stats), int(aff))]
        if kern.startswith("conv3ap"):
            want += [" up%d fold0 stats%d acc0 " % (int(g.in_up), int(stats))]
        yield Op("fwd%s%s" % ("_aff" if aff else "", "_stats" if stats else ""), prec, want, f)

    for aff, acc, bnred, split in dgrad:
        def f(aff=aff, acc=acc, bnred=bnred, split=split):
            dzd = _dev(d.dz, dev, mis_dy)
            s = _ta_with_shape(K)(dzd, d.scz.to(dev), d.shz.to(dev)) if aff else dzd
            dx = d.base.to(dev).clone() if acc else _empty((g.n, g.cin, g.h, g.w), dev, 0, NAN)
            dx2 = None
            if split:
                full = dx
                dx, dx2 = full[:, :split].contiguous(), full[:, split:].contiguous()
            r = op.dgrad(s, wd, g.h, g.w, dx=dx, dx2=dx2, accumulate=acc, bnred=(d.a.to(dev), st) if bnred else None)
            red = r[1] if bnred else None
            got_dx = torch.cat([dx, dx2], 1) if split else dx
            b64 = d.base.double() if acc else 0.0
            fn = lambda dt: dg_ref(aff, prec, dt) + (d.base.to(dt) if acc else 0.0)
            ref_old = dg_ref(aff, None, torch.float64) + b64
            chk = [_check("dx", got_dx, fn, ref_old, bp, old_tol=old)]
            if bnred:
                assert red is not None, "the fused BatchNorm-backward reduce was refused"
                got = _sums_of(red)
                o = R.bnred_sums(ref_old, d.a, d.mean, d.invstd)
                for i, nm in enumerate(("sum g", "sum g a_hat")):
                    chk.append(_check_sums(nm, got[:, i], lambda dt, i=i: R.bnred_sums(fn(dt), d.a, d.mean, d.invstd, dt)[i], o[i],
                                           max(SUM_TOL, old * 10), bp))
            return chk
        want = [kern + ("+bnred" if bnred and kern.startswith("direct") else "") + " "]
        if kern.startswith("conv3rs"):
            want += [" stats%d acc%d aff%d " % (2 if bnred else 0, int(acc), int(aff))]
        if kern.startswith("conv3ap"):
            want += [" up0 fold0 stats%d acc%d " % (2 if bnred else 0, int(acc))]
        yield Op("dgrad%s%s%s%s" % ("_aff" if aff else "", "_acc" if acc else "", "_bnred" if bnred else "", "_split%d" % split if split else ""),
                 prec, want, f)

    for bn in fold:
        def f(bn=bn):
            r = op.dgrad_fold(d.dz.to(dev), wd, g.h, g.w, bnred=(d.a_half.to(dev), st) if bn else None)
            dx, red = r if bn else (r, None)
            fn = lambda dt: R.fold2(dg_ref(False, prec, dt))
            ref_old = R.fold2(dg_ref(False, None, torch.float64))
            chk = [_check("dx", dx, fn, ref_old, bp, old_tol=old)]
            if bn:
                assert red is not None, "the fused BatchNorm-backward reduce was refused"
                got = _sums_of(red)
                o = R.bnred_sums(ref_old, d.a_half, d.mean, d.invstd)
                for i, nm in enumerate(("sum g", "sum g a_hat")):
                    chk.append(_check_sums(nm, got[:, i], lambda dt, i=i: R.bnred_sums(fn(dt), d.a_half, d.mean, d.invstd, dt)[i], o[i],
                                           max(SUM_TOL, old * 10), bp))
            return chk
        yield Op("dgrad_fold%s" % ("_bnred" if bn else ""), prec, [kern + " ", " fold1 stats%d acc0 " % (2 if bn else 0)], f)


# ------------------------------------------------------------------------------------------ weight gradient
def wgrad_ops(K, dev, d, prec, kern, aff, modes=("plain", "db", "acc"), rounded=True, has_db=True):
    """rounded False: a direct kernel (fp32 FMA on unrounded operands, one chain)"""
    g = d.g
    pr = prec if rounded else None
    old = R.OLD_TOL[prec] if rounded else 1e-4
    op = K.ConvOp(g.cin, g.cout, g.k, stride=g.stride, pad=g.pad, in_up=g.in_up)
    wg = lambda dt: d.memo(("wg", aff, pr, dt), lambda: R.wgrad_ref(g, d.xop(aff), d.dz, pr, dt))
    wg_old = lambda: d.memo(("wg", aff, None, torch.float64), lambda: R.wgrad_ref(g, d.xop(aff), d.dz, None))
    db = lambda dt: R.chan_sums(d.dz, dt)
    for mode in modes:
        def f(mode=mode):
            s, x2 = _src(K, d, dev, aff)
            dzd = d.dz.to(dev)
            acc = mode == "acc"
            with_db = has_db and mode != "plain"
            dw = d.base_w.to(dev).clone() if acc else torch.full(d.w.shape, NAN, device=dev)
            dbias = None
            if with_db:
                dbias = d.base_b.to(dev).clone() if acc else torch.full((g.cout,), NAN, device=dev)
            op.wgrad(s, dzd, dw, dbias, g.h, g.w, x2=x2, accumulate=acc)
            fn = (lambda dt: wg(dt) + d.base_w.to(dt)) if acc else wg
            chk = [_check("dw", dw, fn, wg_old() + (d.base_w.double() if acc else 0.0), pr, axis=0, old_tol=old)]
            if with_db:
                dbs = (lambda dt: (db(dt)[0] + d.base_b.to(dt), db(dt)[1] + d.base_b.abs().double())) if acc else db
                chk.append(_check_sums("db", dbias, dbs, dbs(torch.float64), 1e-4, None))
            return chk
        yield Op("wgrad_%s%s" % (mode, "_aff" if aff else ""), prec, [kern + " "], f)


# ------------------------------------------------------------------------------------------ the tables
BOTH = ("bf16x3", "bf16")
ALL_RS_FWD = [(False, False), (True, False), (False, True), (True, True)]
ALL_RS_DGRAD = [(a, c, b, 0) for a in (False, True) for c in (False, True) for b in (False, True)]


def table_ap_rs(K, dev):
    """conv3ap: rows % 64, reduction % 16, maps of whole 32 x 8 tiles, an even number of them.  (n, c1, c2, cout, h, w, up)"""
    P = "bf16x3"
    # forward: red = 16 (ONE chunk), one co tile, one tile pair in all
    d = Data(1, 2, 16, 0, 64, 8, 32, 3)
    yield "ap 2x16->64 8x32", d, conv_ops(K, dev, d, P, "conv3ap", fwd=[(False, False), (False, True)])
    # red = 48 (an odd 16-chunk inside a 32-record), two co tiles, two tile rows x two tile columns; dgrad: rows 128, red 48
    d = Data(2, 1, 48, 0, 128, 16, 64, 3)
    yield "ap 1x48->128 16x64", d, conv_ops(K, dev, d, P, "conv3ap", fwd=[(True, True), (False, False)])
    # two sources 48 + 80 (a boundary at a multiple of 16 that is no multiple of 32), the affine on the first; statistics
    d = Data(3, 2, 48, 80, 64, 8, 64, 3)
    yield "ap 2x(48+80)->64 8x64", d, conv_ops(K, dev, d, P, "conv3ap", fwd=[(True, True), (True, False)])
    # through the nearest-x2 fold (up1), three co tiles; the folded data gradient of the same layer (rows 64), with / without bnred
    d = Data(4, 2, 64, 0, 192, 16, 32, 3, up=True)
    yield "ap up 2x64->192 16x32", d, conv_ops(K, dev, d, P, "conv3ap", fwd=[(False, True), (False, False)], fold=[False, True])
    # data gradient: rows = cin, red = cout.  red 16: plain + accumulate, one tile pair
    d = Data(5, 2, 64, 0, 16, 8, 32, 3)
    yield "ap dgrad 2x64<-16 8x32", d, conv_ops(K, dev, d, P, "conv3ap", dgrad=[(False, False, False, 0), (False, True, False, 0)])
    # rows 128 (two co tiles), red 48: bnred, bnred + accumulate, split over two destinations 32 + 96 (plain and accumulating)
    d = Data(6, 2, 128, 0, 48, 16, 32, 3)
    yield "ap dgrad 2x128<-48 16x32", d, conv_ops(K, dev, d, P, "conv3ap", dgrad=[(False, False, True, 0), (False, True, True, 0),
                                                                                  (False, False, False, 32), (False, True, False, 32)])
    # more (tile pair, co tile) items than workgroups: 8 x 8 x 9 tiles / 2 = 288 items on at most 256 workgroups (one per compute
    # unit, csrc/conv_ap.hip:170), at the cheapest channel counts
    d = Data(7, 8, 16, 0, 64, 64, 288, 3)
    yield "ap 8x16->64 64x288", d, conv_ops(K, dev, d, P, "conv3ap", fwd=[(False, True)])

    # conv3rs: 32 -> 32 only.  (n, h, w): items = n x strips x row segments, grid = items / 4
    RS = [
        (11, 1, 2, 32, "h = 2 (top and bottom padding in one window), one strip: both halo columns outside the image"),
        (12, 2, 3, 32, "remainder 2 of the unroll of four"),
        (13, 1, 4, 96, "remainder 3; three strips: the halo columns are the neighbours' lines"),
        (14, 2, 19, 96, "remainder 2 behind four unrolled rounds, three strips, six items on two workgroups"),
        (15, 1, 37, 32, "rows split into two segments (18 + 19 rows: remainders 1 and 2): seams inside the image"),
        (16, 4, 64, 128, "4 x 4 strips x 4 segments of 16 rows = 64 items, 16 workgroups: the XCD mapping"),
    ]
    for seed, n, h, w, why in RS:
        d = Data(seed, n, 32, 0, 32, h, w, 3)
        yield "rs %dx32->32 %dx%d" % (n, h, w), d, conv_ops(K, dev, d, P, "conv3rs", fwd=ALL_RS_FWD, dgrad=ALL_RS_DGRAD)


def table_w3_w1_direct(K, dev):
    for prec in BOTH:
        # ---- wgrad3: cout % 64, sources % 32, maps of whole 32 x 4 tiles
        d = Data(21, 1, 32, 0, 64, 4, 32, 3)         # one tile in all (one co tile, one chunk, one pixel tile): ksplit 1
        yield "w3 1x32->64 4x32", d, wgrad_ops(K, dev, d, prec, "wgrad3", False)
        d = Data(22, 2, 32, 32, 128, 8, 64, 3)       # two sources + affine; 2 co tiles x 2 chunks x (2 x 2 pixel tiles x 2): ksplit 8
        yield "w3 2x(32+32)->128 8x64", d, wgrad_ops(K, dev, d, prec, "wgrad3", True)
        d = Data(23, 1, 64, 0, 192, 12, 32, 3)       # one source + affine, three co tiles, three pixel tiles: ksplit 3
        yield "w3 1x64->192 12x32", d, wgrad_ops(K, dev, d, prec, "wgrad3", True)
        # ---- wgrad1: co_b 1 / 2 (cout > 32), ci_b 1 / 2 / 3 (cin > 32, > 64)
        d = Data(31, 1, 20, 0, 24, 4, 4, 1)          # one 16-pixel step in all; ragged; co_b 1, ci_b 1
        yield "w1 1x20->24 4x4", d, wgrad_ops(K, dev, d, prec, "wgrad1", True)
        # co_b 2, ci_b 2, ragged both ways, the source boundary (24) inside a block; 15 steps per image, 30 in all over 3 wanted
        # workgroups: 10 does not divide 15, the divisor search raises steps_per_wg to 15
        d = Data(32, 2, 24, 16, 40, 12, 20, 1)
        yield "w1 2x(24+16)->40 12x20", d, wgrad_ops(K, dev, d, prec, "wgrad1", True)
        d = Data(33, 2, 48, 32, 24, 8, 8, 1)         # ci_b 3, co_b 1; the source boundary (48) inside block 1
        yield "w1 2x(48+32)->24 8x8", d, wgrad_ops(K, dev, d, prec, "wgrad1", True)
        d = Data(34, 1, 128, 0, 72, 8, 16, 1)        # co_b 2, ci_b 3: two co tiles (64 + 8) x two ci tiles (96 + 32)
        yield "w1 1x128->72 8x16", d, wgrad_ops(K, dev, d, prec, "wgrad1", False)
        d = Data(35, 3, 48, 0, 32, 4, 8, 1)          # co_b 1, ci_b 2
        yield "w1 3x48->32 4x8", d, wgrad_ops(K, dev, d, prec, "wgrad1", True, modes=("db",))
        d = Data(37, 2, 32, 0, 32, 4, 8, 1)          # co_b 1, ci_b 1 with one FULL 32 x 32 block
        yield "w1 2x32->32 4x8", d, wgrad_ops(K, dev, d, prec, "wgrad1", True)
        d = Data(36, 1, 32, 0, 64, 8, 8, 1)          # co_b 2, ci_b 1
        yield "w1 1x32->64 8x8", d, wgrad_ops(K, dev, d, prec, "wgrad1", False, modes=("acc",))
        # ---- direct kernels (fp32 FMA; weights hi + lo, hi in bf16 mode): one chain
        # first layer 1 -> cout, 3x3: aligned / ragged (two 256-quad blocks, the second partial; five channels)
        for seed, n, cout, h, w in ((41, 1, 32, 8, 16), (42, 2, 5, 36, 32)):
            d = Data(seed, n, 1, 0, cout, h, w, 3)
            yield "c1 %dx1->%d %dx%d" % (n, cout, h, w), d, conv_ops(K, dev, d, prec, "direct c1 fwd", fwd=[(False, True), (False, False)],
                                                                     model="direct", bprec=None)
            yield "c1 %dx1->%d %dx%d wgrad" % (n, cout, h, w), d, wgrad_ops(K, dev, d, prec, "direct c1 wgrad", False, rounded=False)
        # classifier 1x1, cout <= 8 (pw_fwd_kernel<4 / 5 / 8>): two sources + affine; dgrad plain / accumulate / split / bnred
        for seed, n, c1, c2, cout, h, w in ((43, 2, 16, 16, 4, 8, 8), (44, 2, 24, 24, 5, 6, 10), (45, 1, 20, 0, 8, 4, 4)):
            d = Data(seed, n, c1, c2, cout, h, w, 1)
            yield "pw %dx%d->%d %dx%d" % (n, c1 + c2, cout, h, w), d, conv_ops(
                K, dev, d, prec, "direct 1x1 fwd", fwd=[(True, False), (False, False)], model="direct", bprec=None)
            yield "pw %dx%d<-%d %dx%d dgrad" % (n, c1 + c2, cout, h, w), d, conv_ops(
                K, dev, d, prec, "direct 1x1 dgrad", dgrad=[(False, False, False, 0), (False, True, False, 0), (False, True, False, 8),
                                                            (False, False, True, 0), (False, True, True, 0)], model="direct", bprec=None)
        # discriminator first layer 4x4 / stride 2 / pad 2, cin <= 5: forward on d1_fwd_kernel (MFMA, cout 64: the ordinary
        # three planes), dgrad on d1_dgrad_kernel (gradient one float behind the alignment: it checks its destination only),
        # wgrad on d1_wgrad_kernel (cin <= 4, no bias gradient)
        for seed, n, cin, cout, h, w in ((46, 1, 4, 64, 8, 8), (47, 2, 5, 64, 6, 24), (48, 2, 3, 20, 6, 24)):
            d = Data(seed, n, cin, 0, cout, h, w, 4, stride=2, pad=2)
            if cout == 64:
                yield "d1 %dx%d->64 %dx%d fwd" % (n, cin, h, w), d, conv_ops(K, dev, d, prec, "direct d1 fwd (mfma)", fwd=[(False, False)])
            yield "d1 %dx%d<-%d %dx%d dgrad" % (n, cin, cout, h, w), d, conv_ops(
                K, dev, d, prec, "direct d1 dgrad", dgrad=[(False, False, False, 0), (False, True, False, 0)], model="direct", bprec=None,
                mis_dy=1 if cout != 64 else 0)
            if cin <= 4:
                yield "d1 %dx%d->%d %dx%d wgrad" % (n, cin, cout, h, w), d, wgrad_ops(K, dev, d, prec, "direct d1 wgrad", False, modes=("plain", "acc"),
                                                                                      rounded=False, has_db=False)
        # discriminator last layer cin -> 1, 4x4 / stride 2 / pad 2 on a map of at most 292 pixels; ragged: 72 channels, 17 x 13
        for seed, n, cin, h, w in ((49, 1, 64, 9, 9), (50, 2, 72, 17, 13)):
            d = Data(seed, n, cin, 0, 1, h, w, 4, stride=2, pad=2)
            yield "d5 %dx%d->1 %dx%d" % (n, cin, h, w), d, conv_ops(K, dev, d, prec, "direct d5 fwd", fwd=[(False, False)], model="direct", bprec=None)


def table_w3r(K, dev):
    for prec in BOTH:
        # in_h = 4 (two rows per wave), two sources 24 + 16 with the affine, ragged blocks on both sides (40 -> 24)
        d = Data(61, 1, 24, 16, 24, 4, 32, 3)
        yield "w3r 1x(24+16)->24 4x32", d, wgrad_ops(K, dev, d, prec, "wgrad3r", True)
        # 33 (image, strip) pairs over 512 / 16 tiles = 32 wanted slices: two pairs per slice, 17 slices, the last one short
        d = Data(62, 11, 128, 0, 128, 4, 96, 3)
        yield "w3r 11x128->128 4x96", d, wgrad_ops(K, dev, d, prec, "wgrad3r", False, modes=("db",))
        # 13 rows: 6 and 7 per wave (remainders 2 and 3 of the unroll of four); ragged 40 -> 24, three strips
        d = Data(63, 2, 40, 0, 24, 13, 96, 3)
        yield "w3r 2x40->24 13x96", d, wgrad_ops(K, dev, d, prec, "wgrad3r", True)
        # rsplit 2 (64 rows, one image, one strip, one tile): 16 rows per wave
        d = Data(64, 1, 32, 0, 24, 64, 32, 3)
        yield "w3r 1x32->24 64x32", d, wgrad_ops(K, dev, d, prec, "wgrad3r", True, modes=("acc",))
        # UP: the stored input at half resolution; ragged 48 -> 40, 10 logical rows (5 per wave: remainder 1), two strips
        d = Data(65, 2, 48, 0, 40, 10, 64, 3, up=True)
        yield "w3r up 2x48->40 10x64", d, wgrad_ops(K, dev, d, prec, "wgrad3r", True)
        # UP with two sources, rsplit 2
        d = Data(66, 1, 16, 16, 32, 64, 32, 3, up=True)
        yield "w3r up 1x(16+16)->32 64x32", d, wgrad_ops(K, dev, d, prec, "wgrad3r", True, modes=("db",))


BUILD = {"ap_rs": table_ap_rs, "w3_w1_direct": table_w3_w1_direct, "w3r": table_w3r}


def _ratio(q):
    return q["err"] / q["e32"] if q["e32"] > 0 else (0.0 if q["err"] == 0 else float("inf"))


def main(table, out_path):
    from pointcloududa_amd import kernels as K
    dev = torch.device("cuda", 0)
    t_start = time.time()
    with open(out_path, "w") as out:
        for case, d, ops in BUILD[table](K, dev):
            for o in ops:
                K.set_precision(o.prec)
                t0 = time.time()
                fb = K.fallback_count()
                checks = o.thunk()
                torch.cuda.synchronize()          # a HIP error of this operation surfaces here: nothing runs after it
                tag = K.last_kernel()
                attributed = all(s in tag + " " for s in o.want) and tag.startswith(o.want[0])
                worst = max(checks, key=_ratio)
                ok = all(q["err"] <= q["bound"] and q["old_err"] < q["old_bound"] for q in checks)
                rec = dict(table=table, case=case, op=o.name, prec=o.prec, last_kernel=tag, want=o.want, attributed=attributed,
                           fallbacks=K.fallback_count() - fb, err=worst["err"], e32=worst["e32"], bound=worst["bound"], ok=ok, checks=checks,
                           macs=d.g.macs, seconds=round(time.time() - t0, 4))
                out.write(json.dumps(rec) + "\n")
                out.flush()
        out.write(json.dumps(dict(table=table, done=True, seconds=round(time.time() - t_start, 2))) + "\n")


if __name__ == "__main__":
    try:
        main(sys.argv[1], sys.argv[2])
    except BaseException:      # a HIP error (or anything else): report and stop, non-zero
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(3)
