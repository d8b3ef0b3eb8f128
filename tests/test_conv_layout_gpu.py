"""The 2-D convolution kernels on tensors that are NOT dense and freshly allocated: the ABI (pcuda_src / pcuda_dst: any
pointer, any sample and channel stride, dense planes) admits channel slices, padded planes and odd storage offsets, and every
fast kernel sits behind a host-side alignment gate of its own.  Each case runs an entry with all operands dense -- asserting
the kernel family with ``K.last_kernel()`` --, then again with ONE operand at a time in each layout of
tests/layout_helpers.py, and holds every run to

  * the float64 reference (torch conv2d + autograd on the CPU, nearest x2 in front for ``in_up`` layers) within the
    project's tolerances: 1e-4 (bf16x3), 2e-2 (bf16), 1e-4 for bias gradients -- TOL of tests/test_conv_gpu.py;
  * ``canary_intact`` for a destination (pre-filled with NaN when not accumulating: every element written, nothing else);
  * NaN around every source: a read that leaves the plane shows in the values;
  * the SAME BITS as the dense run where ``last_kernel()`` reports the same tag: a layout moves addresses, not the order of
    summation.  (One exception, by the code: the per-tile BatchNorm / reduce partial sums when a DESTINATION moves.  The tag
    does not carry the epilogue, and the transposed epilogue -- te_dst_ok -- sums a tile's rows in another order than the
    plain one it falls back to; the stored tensor comes from the same accumulators and is still compared bit for bit.)

Every off-layout run prints ``DISPATCH ...`` with the kernel that took it; DESIGN.md's layout table is that output.

gate -> the cases on either side of it (x|y = that operand moved; "mis" = off4 off8 pad1 pad2; a channel slice of planes of 4k
floats keeps every gate's residues and stays on the dense run's kernel: the foreign sample stride is all it changes)
  te_dst_ok (conv_host.h)                       pass: pipe_te fwd+stats, dgrad+bnred dense, slice   refuse: pipe_te y|dx = mis -> igemm_generic (the
                                                                                                    build holds no plain-epilogue twin); s2_* (ox_mul = 2)
  fold_ok, dgrad_fold `a` (conv_igemm.hip:444,  pass: fold_pipe (ABI) dense, dx|a = off8 pad2 slice   refuse: fold_pipe (ABI) dx|a = off4 pad1 -> UNSUPPORTED
    :787; conv_ap.hip:123-125)                        ap_up (ABI) likewise                                  (wrapper: dgrad + upsample2_bwd); fold_none: no plan
  fused reduce, `a` 16 B (conv_igemm.hip:746,   pass: pipe_te, ap, rs, rs_aff, pw8 dgrad+bnred      refuse: ... a = mis -> red=separate (same kernel without
    conv_ap.hip:128, conv_direct.hip:469)             dense, a = slice                                     the reduce, or the plain one)
  ap_launch_ok (conv_ap.hip:117-131)            pass: ap, ap_cat, ap_up dense, slice                refuse: x|x2|y|dy|dx|dx2 = mis -> igemm8 / igemm_generic
  rs_try_launch `al` (conv_rs.hip:396)          pass: rs, rs_aff dense, slice                       refuse: x|y|dy|dx = mis -> igemm8
  aligned16 (conv_direct.hip:409/432/467/509,   pass: c1, pw8, d1a, d1b dense, slice; d1* dgrad     refuse: c1 x|y (-> igemm8, statistics by pcuda_bn_stats),
    conv_direct_d1.hip:268/305)                       dy, d1* wgrad dy (no gate: scalar reads)              c1 wgrad x|dy, pw8 *, d1* dgrad dx, d1* wgrad x = mis
  d1 forward 8 B (conv_direct_d1.hip:583)       pass: d1a, d1b fwd dense, x = off8 pad2, y = any    refuse: d1a, d1b fwd x = off4 pad1 -> igemm8
  wgrad3 / wgrad3r / wgrad1 16 B                pass: w3, w3_cat, w3r, w3r_up, w1, w1_cat dense     refuse: x|x2|dy = mis -> wgrad / wgrad8
  generic wgrad aligned4 (conv_wgrad.hip:271)   pass: wg_al dense (rows of 32)                      refuse: wg_al dy = mis; wg_52, wg_s2 (rows of 52 / 17)
  xq: in_w % 4 == 0 only (conv_igemm.hip:427,   on:  ig8_*, pipe_te, fold_pipe, ap* / rs* refused,   off: s2_odd33 dgrad, lrelu_odd (igemm8, rows of 17 / 19),
    conv_wgrad.hip:283)                               wg_al, wg_52: x|dy = mis are float4 loads off        wg_s2 (rows of 33)
                                                      16-byte alignment, right on gfx950
  fast_src_ok / fast_dst_ok (split positions)   pass: ig8_cat 64 + 32, w3_cat 64 + 64               refuse: s2_odd12 dx 12 + 12 (c1 & 7); 48 + 32 / 48 + 16 (c1 & 31)
                                                                                                    once wgrad1 / conv3ap refuse a view: w1_cat x|x2|dy = mis ->
                                                                                                    wgrad_generic, ap_cat fwd x|x2|y = mis -> igemm_generic
"""
import collections
import ctypes as C
import functools
import types
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from layout_helpers import LAYOUTS, canary_intact, place, place_view

pytestmark = pytest.mark.gpu
TOL = {"bf16x3": 1e-4, "bf16": 2e-2}        # tests/test_conv_gpu.py
BIAS_TOL = 1e-4
OFF_LAYOUTS = {"bf16x3": tuple(l for l in LAYOUTS if l != "dense"), "bf16": ("off4", "pad1")}
NAN = float("nan")

Case = collections.namedtuple("Case", "name n c1 c2 cout h w k s p d up aff bias slope dsplit")


def mk(name, n, cin, cout, h, w, k=3, s=1, p=1, d=1, up=False, c2=0, aff=False, bias=True, slope=0.01, dsplit=0):
    """h, w: the LOGICAL input size (doubled already for ``up``); c2: channels of the second source; dsplit: channels of the
    first of two gradient destinations"""
    return Case(name, n, cin - c2, c2, cout, h, w, k, s, p, d, up, aff, bias, slope, dsplit)


CASES = {c.name: c for c in [
    # generic implicit GEMM, few (tile, co-tile) items: the eight-wave kernel
    mk("ig8_3x3", 2, 48, 64, 32, 32, slope=1.0),                            # ragged 32-channel chunk, quad staging
    mk("ig8_short", 2, 8, 32, 12, 16, aff=True),                            # map shorter than a tile, lazy-BatchNorm affine
    mk("ig8_cat", 2, 96, 64, 32, 32, k=1, p=0, c2=32, aff=True, dsplit=64),  # 1x1 behind a concat 64 + 32
    mk("ig8_dil4", 2, 64, 64, 16, 16, p=4, d=4),
    # > 320 items: the four-wave software-pipelined kernel with the transposed epilogue
    mk("pipe_te", 44, 16, 32, 32, 64, aff=True),
    # stride-2 4x4 layers: paired column classes in the data gradient, odd maps (rows of 14 / 33 pixels: no quad staging)
    mk("s2_odd12", 2, 24, 40, 11, 14, k=4, s=2, p=2, bias=False, slope=0.2, dsplit=12),
    mk("s2_odd33", 2, 64, 128, 33, 33, k=4, s=2, p=2, bias=False, slope=0.2, dsplit=32),
    # anti-phase kernel (bf16x3 only)
    mk("ap", 2, 64, 64, 32, 32),
    mk("ap_cat", 2, 64, 64, 16, 64, c2=16, aff=True, dsplit=32),
    mk("ap_up", 2, 64, 64, 16, 64, up=True, slope=1.0),
    # row-streaming kernel of the 32 -> 32 layers (bf16x3 only)
    mk("rs", 2, 32, 32, 19, 32, slope=1.0),
    mk("rs_aff", 2, 32, 32, 6, 64, aff=True),
    # direct (vector-ALU) kernels
    mk("c1", 3, 1, 8, 36, 20),
    mk("pw8", 2, 64, 8, 8, 8, k=1, p=0, c2=32, aff=True, slope=1.0, dsplit=32),
    mk("d1a", 2, 1, 64, 16, 24, k=4, s=2, p=2, bias=False, slope=0.2),
    mk("d1b", 2, 4, 64, 64, 64, k=4, s=2, p=2, bias=False, slope=0.2),
    mk("d5", 2, 72, 1, 17, 13, k=4, s=2, p=2, bias=False, slope=1.0),
    # fused epilogues of the generic kernels
    mk("lrelu_odd", 2, 40, 24, 21, 19, bias=False),
    mk("fold_pipe", 44, 32, 16, 32, 64, up=True, bias=False),
    mk("fold_none", 2, 16, 8, 20, 24, up=True, bias=False),
    # weight gradients
    mk("w3", 1, 32, 128, 4, 32, slope=1.0),
    mk("w3_cat", 2, 128, 128, 16, 32, c2=64, aff=True),
    mk("w3r", 2, 32, 64, 64, 32),
    mk("w3r_up", 2, 64, 32, 64, 64, up=True, aff=True),
    mk("w1", 1, 20, 24, 4, 4, k=1, p=0),
    mk("w1_cat", 2, 80, 40, 12, 8, k=1, p=0, c2=32, aff=True),
    mk("wg_al", 2, 48, 80, 16, 32, aff=True),
    mk("wg_52", 2, 48, 80, 20, 52, bias=False),
    mk("wg_s2", 2, 64, 128, 33, 33, k=4, s=2, p=2, bias=False),
]}


def _f32(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _ref(cs):
    """inputs of one case and its float64 reference (computed once, shared by every test of the case, never written)"""
    rng = np.random.default_rng(zlib.crc32(cs.name.encode()))
    sh, sw = (cs.h // 2, cs.w // 2) if cs.up else (cs.h, cs.w)
    cin = cs.c1 + cs.c2
    r = types.SimpleNamespace(sh=sh, sw=sw, cin=cin)
    r.a = _f32(rng.normal(0, 1, (cs.n, cs.c1, sh, sw)))
    r.b = _f32(rng.normal(0, 1, (cs.n, cs.c2, sh, sw))) if cs.c2 else None
    r.sc = r.sf = None
    xa = r.a.double()
    if cs.aff:      # lazy BatchNorm: a shift far from 0, so that zero padding BEFORE the affine would show
        r.sc = _f32(rng.normal(1, 0.2, cs.c1))
        r.sf = _f32((0.6 + 0.2 * np.abs(rng.normal(0, 1, cs.c1))) * rng.choice([-1.0, 1.0], cs.c1))
        xa = xa * r.sc.double()[None, :, None, None] + r.sf.double()[None, :, None, None]
    r.wt = _f32(rng.normal(0, 0.1, (cs.cout, cin, cs.k, cs.k)))
    r.bias = _f32(rng.normal(0, 0.1, cs.cout)) if cs.bias else None
    xs = (torch.cat([xa, r.b.double()], 1) if cs.c2 else xa).requires_grad_(True)
    xu = F.interpolate(xs, scale_factor=2, mode="nearest") if cs.up else xs
    if cs.up:
        xu.retain_grad()
    w64 = r.wt.double().requires_grad_(True)
    b64 = r.bias.double().requires_grad_(True) if cs.bias else None
    z = F.conv2d(xu, w64, b64, stride=cs.s, padding=cs.p, dilation=cs.d)
    y = F.leaky_relu(z, cs.slope) if cs.slope != 1.0 else z
    r.gz = _f32(rng.normal(0, 1, z.shape))
    z.backward(r.gz.double())
    r.y = y.detach()
    r.stats = torch.stack([r.y.sum((0, 2, 3)), (r.y ** 2).sum((0, 2, 3))], 1)
    r.dx, r.dx_stored, r.dw = xu.grad.detach(), xs.grad.detach(), w64.grad.detach()
    r.db = b64.grad.detach() if cs.bias else None
    # what the fused epilogues read: the saved activation of the layer in front (at the stored resolution), its statistics,
    # a gradient already in the destination
    r.act = _f32(rng.normal(0, 1, (cs.n, cin, sh, sw)))
    r.mean = _f32(rng.normal(0, 0.3, cin))
    r.invstd = _f32(rng.uniform(0.5, 2.0, cin))
    r.base = _f32(rng.normal(0, 1, (cs.n, cin, cs.h, cs.w)))
    r.ahat = (r.act.double() - r.mean.double()[None, :, None, None]) * r.invstd.double()[None, :, None, None]
    return r


def _red_ref(g, ahat):
    return torch.stack([g.sum((0, 2, 3)), (g * ahat).sum((0, 2, 3))], 1)


class Bench:
    """one case on the device: the operands in a requested layout, the entries, the checks; failures are collected so that one
    run reports every layout that is wrong"""

    def __init__(self, K, dev, cs, prec):
        self.K, self.dev, self.cs, self.prec, self.r = K, dev, cs, prec, _ref(cs)
        self.tol, self.fails, self.layouts = TOL[prec], [], OFF_LAYOUTS[prec]
        r = self.r
        self.op = K.ConvOp(r.cin, cs.cout, cs.k, stride=cs.s, pad=cs.p, dil=cs.d, in_up=cs.up)
        self.w = r.wt.to(dev)
        self.b = r.bias.to(dev) if cs.bias else None
        self.sc, self.sf = (r.sc.to(dev), r.sf.to(dev)) if cs.aff else (None, None)
        self.st = K.BNState()
        self.st.mean, self.st.invstd = r.mean.to(dev), r.invstd.to(dev)

    # ---- operands ----
    def src(self, lay):
        x = place_view(self.r.a, self.dev, lay.get("x", "dense"))
        x2 = place_view(self.r.b, self.dev, lay.get("x2", "dense")) if self.cs.c2 else None
        return (self.K.TA(x, self.sc, self.sf) if self.cs.aff else x), x2

    def dst(self, shape, layout, base=None):
        return place(torch.full(shape, NAN) if base is None else base, self.dev, layout)

    def dsts(self, lay, acc, full=None):
        """the gradient destination(s) of the logical input: [(view, backing, reference, base)]"""
        cs, r = self.cs, self.r
        full = r.dx if full is None else full
        parts = [("dx", 0, r.cin)] if not cs.dsplit else [("dx", 0, cs.dsplit), ("dx2", cs.dsplit, r.cin)]
        out = []
        for name, lo, hi in parts:
            base = r.base[:, lo:hi].contiguous() if acc else None
            v, bk = self.dst((cs.n, hi - lo, cs.h, cs.w), lay.get(name, "dense"), base)
            out.append((v, bk, full[:, lo:hi] + base.double() if acc else full[:, lo:hi]))
        return out

    # ---- entries: each returns {tag, outs: {name: (view, backing, ref, tol)}, sums: {name: (tensor, ref, tol)}} ----
    def fwd(self, lay, stats=True):
        cs, r, K = self.cs, self.r, self.K
        x, x2 = self.src(lay)
        oh, ow = self.op.out_hw(cs.h, cs.w)
        yv, yb = self.dst((cs.n, cs.cout, oh, ow), lay.get("y", "dense"))
        fb = K.fallback_count()
        _, part, nt = self.op.forward(x, self.w, self.b, cs.slope, cs.h, cs.w, x2=x2, out=yv, want_stats=stats)
        res = dict(tag=K.last_kernel(), fb=K.fallback_count() - fb, outs={"y": (yv, yb, r.y, self.tol)}, sums={})
        if stats:
            res["sums"]["bn partial sums"] = (part[:nt].double().sum(0), r.stats, self.tol)
        return res

    def dgrad(self, lay, acc=False, bnred=False):
        cs, r, K = self.cs, self.r, self.K
        dy = place_view(r.gz, self.dev, lay.get("dy", "dense"))
        d = self.dsts(lay, acc)
        kw = {}
        if bnred:
            kw["bnred"] = (place_view(r.act, self.dev, lay.get("a", "dense")), self.st)
        fb = K.fallback_count()
        got = self.op.dgrad(dy, self.w, cs.h, cs.w, dx=d[0][0], dx2=d[1][0] if cs.dsplit else None, accumulate=acc, **kw)
        res = dict(tag=K.last_kernel(), fb=K.fallback_count() - fb, sums={},
                   outs={("dx", "dx2")[i]: (v, bk, ref, self.tol) for i, (v, bk, ref) in enumerate(d)})
        if bnred:
            red = got[1]
            res["red"] = red is not None
            if red is not None:
                g = r.dx + r.base.double() if acc else r.dx
                res["sums"]["bn-backward reduce"] = (red[0][:red[1]].double().sum(0), _red_ref(g, r.ahat), self.tol)
        return res

    def wgrad(self, lay, twice=False):
        """``twice``: a second, accumulating call into the same buffers (2 x the gradient, as the existing tests hold it)"""
        cs, r, K = self.cs, self.r, self.K
        x, x2 = self.src(lay)
        dy = place_view(r.gz, self.dev, lay.get("dy", "dense"))
        dw = torch.full(r.wt.shape, NAN, device=self.dev)
        db = torch.full((cs.cout,), NAN, device=self.dev) if cs.bias else None
        fb = K.fallback_count()
        self.op.wgrad(x, dy, dw, db, cs.h, cs.w, x2=x2, accumulate=False)
        if twice:
            self.op.wgrad(x, dy, dw, db, cs.h, cs.w, x2=x2, accumulate=True)
        m = 2.0 if twice else 1.0
        res = dict(tag=K.last_kernel(), fb=K.fallback_count() - fb, outs={}, sums={"dw": (dw, m * r.dw, self.tol)})
        if cs.bias:
            res["sums"]["db"] = (db, m * r.db, BIAS_TOL)
        return res

    def lrelu(self, lay):
        """dgrad * (act > 0 ? 1 : slope) through the wrapper, and the two-kernel form on the same operands"""
        cs, r, K = self.cs, self.r, self.K
        dy = place_view(r.gz, self.dev, lay.get("dy", "dense"))
        a = place_view(r.act, self.dev, lay.get("a", "dense"))
        got = self.op.dgrad_lrelu(dy, self.w, cs.h, cs.w, a, 0.2)
        tag = K.last_kernel()
        two = K.lrelu_bwd(self.op.dgrad(dy, self.w, cs.h, cs.w), a, 0.2)
        if not torch.equal(got, two):
            self.fails.append("%s lrelu %s: differs from dgrad + lrelu_bwd on the same operands" % (cs.name, lay))
        want = torch.where(r.act.double() > 0, r.dx, 0.2 * r.dx)
        return dict(tag=tag, fb=0, outs={"dz": (got, got, want, self.tol)}, sums={})

    def lrelu_abi(self, lay):
        """pcuda_conv2d_dgrad_lrelu itself, destination and activation in ONE layout (the entry wants equal plane strides);
        PCUDA_E_UNSUPPORTED is a legal answer (the wrapper then runs the two kernels) and is printed"""
        cs, r, K = self.cs, self.r, self.K
        from pointcloududa_amd import _lib as L
        layout = lay.get("dx", "dense")
        dy = place_view(r.gz, self.dev, lay.get("dy", "dense"))
        a = place_view(r.act, self.dev, layout)
        dz, bk = self.dst((cs.n, r.cin, cs.h, cs.w), layout)
        g = self.op.geom(cs.n, cs.h, cs.w)
        pk = self.op._packed("dgrad", self.w, g)
        src, dst = K.make_src(dy), K.make_dst(dz)
        rc = L.lib().pcuda_conv2d_dgrad_lrelu(C.byref(g), K._precision, C.byref(src), pk.data_ptr(), C.byref(dst), a.data_ptr(),
                                              a.stride(0), a.stride(1), 0.2, K._stream())
        if rc == L.PCUDA_E_UNSUPPORTED:
            return dict(tag="UNSUPPORTED", fb=0, outs={}, sums={})
        K.check(rc, "conv2d_dgrad_lrelu")
        want = torch.where(r.act.double() > 0, r.dx, 0.2 * r.dx)
        return dict(tag=K.last_kernel(), fb=0, outs={"dz": (dz, bk, want, self.tol)}, sums={})

    def fold(self, lay, bnred=False):
        """the data gradient of an ``in_up`` layer at the stored resolution through the wrapper (dgrad + 2x2 fold in one kernel,
        or the two kernels), against float64 and against the two-kernel form on the same operands"""
        cs, r, K = self.cs, self.r, self.K
        dy = place_view(r.gz, self.dev, lay.get("dy", "dense"))
        kw = {"bnred": (place_view(r.act, self.dev, lay.get("a", "dense")), self.st)} if bnred else {}
        got = self.op.dgrad_fold(dy, self.w, cs.h, cs.w, **kw)
        tag = K.last_kernel()
        res = dict(tag=tag, fb=0, sums={})
        if bnred:
            got, red = got
            res["red"] = red is not None
            if red is not None:
                res["sums"]["bn-backward reduce"] = (red[0][:red[1]].double().sum(0), _red_ref(r.dx_stored, r.ahat), self.tol)
        two = K.upsample2_bwd(self.op.dgrad(dy, self.w, cs.h, cs.w))
        e = rel_err(got, two)
        if not e < 1e-5:      # (the bound tests/test_conv_gpu.py holds the fold to: fp32 summation order of four terms)
            self.fails.append("%s fold %s: %.3g from dgrad + upsample2_bwd on the same operands" % (cs.name, lay, e))
        res["outs"] = {"dx_half": (got, got, r.dx_stored, self.tol)}
        return res

    def fold_abi(self, lay):
        """pcuda_conv2d_dgrad_fold itself with the destination (and the reduce's activation) in a layout"""
        cs, r, K = self.cs, self.r, self.K
        from pointcloududa_amd import _lib as L
        dy = place_view(r.gz, self.dev, "dense")
        a = place_view(r.act, self.dev, lay.get("a", "dense"))
        dx, bk = self.dst((cs.n, r.cin, r.sh, r.sw), lay.get("dx", "dense"))
        g = self.op.geom(cs.n, cs.h, cs.w)
        lib = L.lib()
        nt = lib.pcuda_conv2d_dgrad_tiles(C.byref(g), K._precision)
        red = torch.empty((max(nt, 1), r.cin, 2), device=self.dev)
        pk = self.op._packed("dgrad", self.w, g)
        src, dst = K.make_src(dy), K.make_dst(dx)
        if nt > 0:
            rc = lib.pcuda_conv2d_dgrad_fold(C.byref(g), K._precision, C.byref(src), pk.data_ptr(), C.byref(dst), a.data_ptr(),
                                             a.stride(0), a.stride(1), self.st.mean.data_ptr(), self.st.invstd.data_ptr(),
                                             red.data_ptr(), K._stream())
        else:
            rc = lib.pcuda_conv2d_dgrad_fold(C.byref(g), K._precision, C.byref(src), pk.data_ptr(), C.byref(dst), None, 0, 0,
                                             None, None, None, K._stream())
        if rc == L.PCUDA_E_UNSUPPORTED:
            return dict(tag="UNSUPPORTED", fb=0, outs={}, sums={})
        K.check(rc, "conv2d_dgrad_fold")
        sums = {"bn-backward reduce": (red[:nt].double().sum(0), _red_ref(r.dx_stored, r.ahat), self.tol)} if nt > 0 else {}
        return dict(tag=K.last_kernel(), fb=0, outs={"dx_half": (dx, bk, r.dx_stored, self.tol)}, sums=sums)

    # ---- checks ----
    def check(self, label, res, dense, moved_dst=False):
        for name, (v, bk, ref, tol) in res["outs"].items():
            e = rel_err(v, ref)
            print("    %s %s: rel_err %.3g (bound %g)" % (label, name, e, tol))
            if not e < tol:
                self.fails.append("%s %s: rel_err %.3g, bound %g [%s]" % (label, name, e, tol, res["tag"]))
            if not canary_intact(v, bk):
                self.fails.append("%s %s: wrote outside its view or left an element unwritten [%s]" % (label, name, res["tag"]))
        for name, (t, ref, tol) in res["sums"].items():
            e = rel_err(t, ref)
            print("    %s %s: rel_err %.3g (bound %g)" % (label, name, e, tol))
            if not e < tol:
                self.fails.append("%s %s: rel_err %.3g, bound %g [%s]" % (label, name, e, tol, res["tag"]))
        if dense is not None and res["tag"] == dense["tag"]:
            for name in res["outs"]:
                if name in dense["outs"] and not torch.equal(res["outs"][name][0], dense["outs"][name][0]):
                    self.fails.append("%s %s: same kernel as the dense run, other bits [%s]" % (label, name, res["tag"]))
            for name in res["sums"]:
                # (partial sums of a tile when a DESTINATION moved: the epilogue may differ behind one tag -- module docstring)
                if name in dense["sums"] and not (moved_dst and name in ("bn partial sums", "bn-backward reduce")) and \
                        not torch.equal(res["sums"][name][0], dense["sums"][name][0]):
                    self.fails.append("%s %s: same kernel as the dense run, other bits [%s]" % (label, name, res["tag"]))

    def sweep(self, what, run, operands, want=None, no_fallback=True):
        """dense first (the family must have run: ``want`` in its tag, no pruned-build fallback), then one operand at a time
        in every layout"""
        dense = run({})
        print("DISPATCH %s %s %s dense -> %s" % (self.prec, self.cs.name, what, dense["tag"]))
        if want is not None and (want not in dense["tag"] or (no_fallback and dense["fb"])):
            self.fails.append("%s %s dense: expected %r without fallback, ran %r (fallbacks %d)" %
                              (self.cs.name, what, want, dense["tag"], dense["fb"]))
        self.check("%s %s dense" % (self.cs.name, what), dense, None)
        for opnd in operands:
            for layout in self.layouts:
                label = "%s %s %s=%s" % (self.cs.name, what, opnd, layout)
                try:
                    res = run({opnd: layout})
                except RuntimeError as e:
                    self.fails.append("%s: raised %s" % (label, e))
                    continue
                print("DISPATCH %s %s -> %s%s" % (self.prec, label, res["tag"],
                                                   "" if "red" not in res else (" red=fused" if res["red"] else " red=separate")))
                self.check(label, res, dense, moved_dst=opnd in ("y", "dx", "dx2"))
        return dense

    def done(self):
        assert not self.fails, "\n" + "\n".join(self.fails)


@pytest.fixture
def bench(dev):
    from pointcloududa_amd import kernels as K
    made = []

    def make(name, prec):
        K.set_precision(prec)
        made.append(Bench(K, dev, CASES[name], prec))
        return made[-1]
    yield make
    K.set_precision("bf16x3")


@pytest.fixture
def small_maps(monkeypatch):
    """small maps on the anti-phase and row-streaming kernels, as their own tests run them (the dispatcher gives them launches
    with enough work items for the chip; read per call)"""
    monkeypatch.setenv("PCUDA_AP_MIN_ITEMS", "0")
    monkeypatch.setenv("PCUDA_RS_MIN_ITEMS", "0")
    monkeypatch.setenv("PCUDA_RS_MIN_ROWS", "2")


def _srcs(cs):
    return ["x", "x2"] if cs.c2 else ["x"]


def _dsts(cs):
    return ["dx", "dx2"] if cs.dsplit else ["dx"]


PRECS = ["bf16x3", "bf16"]

# (case, kernel of the dense forward, of the dense data gradient); None: that entry is not run for the case.
# "| igemm8" / "| igemm_pipe": the eight-wave / the four-wave pipelined kernel, no pruned-build fallback.  "| igemm": the
# default build holds no pipelined instantiation of this plan in at least one precision (csrc/variants.h: clamped eight-wave
# tiles, 8-pixel tiles), and the unpipelined igemm_generic takes the launch and counts a fallback -- per-element addresses,
# the kernel every refused view of the other rows ends on.
FWD_DGRAD = [
    ("ig8_3x3", "| igemm8", "| igemm8"), ("ig8_short", "| igemm", "| igemm"), ("ig8_cat", "| igemm8", "| igemm8"),
    ("ig8_dil4", "| igemm", "| igemm8"), ("pipe_te", "| igemm_pipe", "| igemm_pipe"),
    ("s2_odd12", "| igemm", "| igemm"), ("s2_odd33", "| igemm", "| igemm8"),
    ("c1", "direct c1 fwd", None), ("pw8", "direct 1x1 fwd", "direct 1x1 dgrad"),
    ("d1a", "direct d1 fwd (mfma)", "direct d1 dgrad"), ("d1b", "direct d1 fwd (mfma)", "direct d1 dgrad"),
    ("d5", "direct d5 fwd", None),
]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,kf,kd", FWD_DGRAD, ids=[c[0] for c in FWD_DGRAD])
def test_forward_and_dgrad_layouts(bench, name, kf, kd, prec):
    b = bench(name, prec)
    cs = b.cs
    # (the direct 1x1 / 4x4 stride-2 forwards have no statistics epilogue: with statistics those layers run on the MFMA kernels)
    stats = name not in ("pw8", "d1a", "d1b", "d5")
    b.sweep("fwd+stats" if stats else "fwd", lambda lay: b.fwd(lay, stats=stats), _srcs(cs) + ["y"], kf, no_fallback=kf != "| igemm")
    if kd is not None:
        d = b.sweep("dgrad", lambda lay: b.dgrad(lay), ["dy"] + _dsts(cs), kd, no_fallback=kd != "| igemm")
        b.sweep("dgrad+acc", lambda lay: b.dgrad(lay, acc=True), ["dy"] + _dsts(cs), kd, no_fallback=kd != "| igemm")
        if name.startswith("s2_") and " rows%d " % (2 * b.r.cin) not in d["tag"]:       # (conv_host.h, dgrad_pair_ok)
            b.fails.append("%s: the data gradient did not pair its column classes: %r" % (name, d["tag"]))
    b.done()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,want", [("pipe_te", "igemm_pipe+bnred"), ("pw8", "direct 1x1 dgrad+bnred")])
def test_dgrad_with_fused_reduce_layouts(bench, name, want, prec):
    """the reduce rides in the transposed epilogue (te_dst_ok) / the direct kernel and wants `a` 16-byte aligned; everything
    else gets the gradient from the plain kernel and leaves the reduce to the caller (red=separate)"""
    b = bench(name, prec)
    if name == "pw8":
        b.cs = b.cs._replace(dsplit=0)      # (the fused reduce has one destination)
    for acc in (False, True):
        d = b.sweep("dgrad+bnred" + ("+acc" if acc else ""), lambda lay: b.dgrad(lay, acc=acc, bnred=True), ["dy", "dx", "a"], want)
        if not d.get("red"):
            b.fails.append("%s: the dense run did not fuse the reduce" % name)
    b.done()


AP_RS = [("ap", "conv3ap", True), ("ap_cat", "conv3ap", False), ("rs", "conv3rs", True), ("rs_aff", "conv3rs", True)]


@pytest.mark.parametrize("name,want,red", AP_RS, ids=[c[0] for c in AP_RS])
def test_anti_phase_and_row_streaming_layouts(bench, small_maps, name, want, red):
    """bf16x3 only (neither kernel has a bf16 instantiation); statistics of a view the kernel refuses: the wrapper runs the
    convolution without them and pcuda_bn_stats on what it stored"""
    b = bench(name, "bf16x3")
    cs = b.cs
    b.sweep("fwd+stats", lambda lay: b.fwd(lay), _srcs(cs) + ["y"], want)
    b.sweep("fwd", lambda lay: b.fwd(lay, stats=False), _srcs(cs) + ["y"], want)
    b.sweep("dgrad", lambda lay: b.dgrad(lay), ["dy"] + _dsts(cs), want)
    b.sweep("dgrad+acc", lambda lay: b.dgrad(lay, acc=True), ["dy"] + _dsts(cs), want)
    if red:
        d = b.sweep("dgrad+bnred", lambda lay: b.dgrad(lay, bnred=True), ["dy", "dx", "a"], want + "+bnred")
        if not d.get("red"):
            b.fails.append("%s: the dense run did not fuse the reduce" % name)
    b.done()


def test_anti_phase_up_convolution_layouts(bench, small_maps):
    """forward through the nearest-x2 fold (the source at the stored resolution) and the folded data gradient (8-byte gates)"""
    b = bench("ap_up", "bf16x3")
    b.sweep("fwd+stats", lambda lay: b.fwd(lay), ["x", "y"], "conv3ap")
    b.sweep("dgrad_fold", lambda lay: b.fold(lay), ["dy"], "conv3ap+fold")
    d = b.sweep("dgrad_fold+bnred", lambda lay: b.fold(lay, bnred=True), ["dy", "a"], "conv3ap+fold")
    if not d.get("red"):
        b.fails.append("ap_up: the dense run did not fuse the reduce")
    b.sweep("dgrad_fold (ABI)", lambda lay: b.fold_abi(lay), ["dx", "a"], "conv3ap+fold")
    b.done()


@pytest.mark.parametrize("prec", PRECS)
def test_dgrad_with_leaky_relu_backward_layouts(bench, prec):
    b = bench("lrelu_odd", prec)
    b.sweep("dgrad_lrelu", lambda lay: b.lrelu(lay), ["dy", "a"], "| igemm8")
    b.sweep("dgrad_lrelu (ABI)", lambda lay: b.lrelu_abi(lay), ["dy", "dx"], "| igemm8")
    b.done()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,want", [("fold_pipe", "| igemm_pipe+fold"), ("fold_none", "| igemm")])
def test_dgrad_with_2x2_fold_layouts(bench, name, want, prec):
    b = bench(name, prec)
    nf = name == "fold_pipe"        # (fold_none: no folding plan, dgrad + upsample2_bwd; its bf16 plan is in no configuration)
    b.sweep("dgrad_fold", lambda lay: b.fold(lay), ["dy"], want, no_fallback=nf)
    b.sweep("dgrad_fold+bnred", lambda lay: b.fold(lay, bnred=True), ["dy", "a"], want, no_fallback=nf)
    if name == "fold_pipe":
        b.sweep("dgrad_fold (ABI)", lambda lay: b.fold_abi(lay), ["dx", "a"], want)
    b.done()


WGRAD = [("w3", "wgrad3 "), ("w3_cat", "wgrad3 "), ("w3r", "wgrad3r "), ("w3r_up", "wgrad3r "), ("w1", "wgrad1 "), ("w1_cat", "wgrad1 "),
         ("wg_al", "wgrad "), ("wg_52", "wgrad "), ("wg_s2", "wgrad "), ("c1", "direct c1 wgrad"), ("d1a", "direct d1 wgrad"),
         ("d1b", "direct d1 wgrad")]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,want", WGRAD, ids=[c[0] for c in WGRAD])
def test_wgrad_layouts(bench, name, want, prec):
    b = bench(name, prec)
    # (wg_52 is the geometry of test_pruned_build_falls_back_to_the_generic_kernels: in no configuration, so the generic
    #  variant of its family may take it and count a fallback)
    ops = _srcs(b.cs) + ["dy"]
    d = b.sweep("wgrad", lambda lay: b.wgrad(lay), ops, None)
    if not d["tag"].startswith(want) or (name != "wg_52" and d["fb"]):
        b.fails.append("%s wgrad dense: expected %r without fallback, ran %r (fallbacks %d)" % (name, want, d["tag"], d["fb"]))
    if name == "w3r_up" and " up1 " not in d["tag"]:
        b.fails.append("w3r_up: not the UP variant: %r" % d["tag"])
    b.sweep("wgrad x2 (accumulate)", lambda lay: b.wgrad(lay, twice=True), ops, None)
    b.done()
