"""Operand-exact float64 references of the MFMA convolution kernels, and Python mirrors of the variant keys.

The kernels round their two operands to bf16 with round-to-nearest-even (``pack_bf16x2`` / ``split2``, csrc/common.h:77-91;
the weights in ``pack_multi_kernel``, csrc/conv_igemm.hip:45-47) and multiply on ``v_mfma_f32_32x32x16_bf16``: a bf16 x bf16 product
has 16 significant bits and is exact in fp32, so all a correct kernel has left is the rounding of its fp32 accumulation.

* bf16 mode: one product plane, hi x hi, hi = bf16(a).
* bf16x3 mode: hi = bf16(a), lo = bf16(a - hi) and THREE planes: lo x hi, hi x lo, hi x hi; lo x lo is dropped.
  Forward / dgrad: csrc/conv_igemm_impl.h:537-541 (``al*bh``, ``ah*bl``, ``ah*bh``: a = packed weights, b = staged activations; the
  same three lines in the generic kernel at :126 and the eight-wave kernel at :1078).  Weight gradient: ``wgrad_mfma_phase``,
  csrc/conv_wgrad_impl.h:237-241 (a = dZ rows, b = X read back transposed).

Every reference here is the float64 sum of exactly those planes (float64 adds 2^-53 per step to exact products: nothing next to
fp32's 2^-24), followed, in float64, by what the kernels do in fp32 behind the sum: bias, LeakyReLU, the mask of the fused
LeakyReLU backward, the 2x2 fold, the accumulation into an existing buffer.  ``e32`` is the error of the SAME expression
evaluated in float32 by torch's CPU convolutions: the yardstick for "one correct fp32 summation order", from which the tests take
their bound (4 x e32: two correct orders differ from float64 by amounts of that size each, and split-K adds a reduction level;
times the number of accumulation chains the mode interleaves in one accumulator, ``ACC_CHAINS``).

The error measure is per output channel, ``chan_err``: max |got - ref| over the channel / max |ref| over the channel, maximised
over channels (for a weight gradient the channel is a ``cout`` row), so that a wrong 32-channel chunk cannot hide behind the
scale of the others.  Per-channel SUMS (bias gradient, BatchNorm partial sums) cancel, so a channel's own value is no scale for
its summation error: ``sum_err`` divides by the channel's sum of |terms| instead, the quantity every fp32 summation bound is
stated in.

The purpose-built kernels (anti-phase, row-streaming, wgrad3, wgrad3r, wgrad1, the direct kernels; tests/conv_special_child.py)
need three things more:

* The affine on load (the lazy BatchNorm, ``pcuda_src.scale1 / shift1``): every kernel applies it as ONE ``fmaf(x, sc, sh)`` in
  fp32 BEFORE the bf16 split (csrc/conv_rs.hip:166 and :177 for the halo pixel, csrc/conv_wgrad3r.hip:163-164,
  csrc/conv_wgrad1.hip:129, csrc/conv_wgrad3.hip:244, csrc/conv_ap_impl.h:252, csrc/conv_direct.hip:289 in pw_fwd_kernel, which
  then multiplies the unrounded result), and padding is zero AFTER the affine
  (conv_rs.hip:162 ``vm``, conv_wgrad3r.hip:160 ``rvalid`` / :125 ``hvalid``).  ``affine_operand`` is
  ``float32(float64(x) * sc + sh)``: the product of two fp32 values is exact in float64 (48 bits), so this is the singly
  rounded FMA up to double rounding -- the float64 sum rounds to 53 bits before the rounding to 24, which moves the result by
  one fp32 ulp where the float64 value falls within 2^-29 ulp of an fp32 tie (about one element in 2^28; it changes a bf16 hi
  plane only if the element also sits on a bf16 tie).  The references take the OPERAND (``source_operand``), so their zero
  padding is applied after the affine by construction.
* Two sources (the zero-copy concat): ``source_operand(x1, sc, sh, x2)`` = cat(affine(x1), x2), the affine on the first source
  only, as every caller uses it.
* The direct (vector-ALU) kernels' operand model, ``model="direct"``: they rebuild the weight from the packed planes as
  hi + lo -- hi alone in bf16 mode, whose records carry no lo plane (``if (p.rec > IG_REC) v += ...[32]``:
  csrc/conv_direct.hip:68-69 c1_fwd, :255-258 pw_fwd, :323-326 pw_dgrad; csrc/conv_direct_d1.hip:55-58 d1_dgrad, :373-375
  d5_fwd) -- and multiply UNROUNDED fp32 activations with fp32 FMA: one plane (x, hi + lo) or (x, hi), one chain
  (``bound_of(e32, None)``).  hi + lo is exact in fp32 (16 significant bits).  The direct weight gradients (c1_wgrad_kernel,
  d1_wgrad_kernel) read no packed weight and round nothing: ``prec=None``.  ``d1_fwd_kernel`` (conv_direct_d1.hip:524-540) is
  an MFMA kernel with the ordinary split and the three planes: the ordinary model.
  Against the bf16x3 model the direct one keeps what that drops: with x = xh + xl + r, |xl| <= 2^-9 |x|, |r| <= 2^-18 |x|,
  |wl| <= 2^-9 |w|:  direct - bf16x3 = sum xl wl + sum r (wh + wl), at most (2^-18 + 2^-18 (1 + 2^-8)) sum |x| |w|
  <= 2^-17 (1 + 2^-8) sum |x| |w| (tests/test_conv_exact_ref.py checks it).
"""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn import grad as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILT_VARIANTS = os.path.join(ROOT, "pointcloududa_amd", "csrc", "built_variants.h")
OLD_TOL = {"bf16x3": 1e-4, "bf16": 2e-2}       # the project's bounds against the unrounded fp64 convolution (rel_err)
FACTOR = 4.0                                   # kernel bound = FACTOR x ACC_CHAINS[prec] x e32
# Accumulation chains per output.  The kernels add all product planes of a 16-product step into ONE fp32 accumulator
# (conv_igemm_impl.h:537-541, conv_wgrad_impl.h:237-241): in bf16x3 mode three roundings per step, each at the magnitude of the
# running FULL sum.  The float32 evaluation behind e32 convolves each plane on its own and adds the three results once; the lo
# planes' sums are 2^-8 of the hi plane's, their rounding is invisible, so e32 holds the rounding of ONE chain whatever the
# mode.  A correct bf16x3 kernel therefore has three times the rounding steps e32 was measured on, a bf16 kernel the same.
ACC_CHAINS = {"bf16": 1, "bf16x3": 3}


def bound_of(e32, prec):
    """the kernels' bound for a quantity whose float32 evaluation is e32 off float64; prec None: no MFMA in it (bias gradient)"""
    return FACTOR * (ACC_CHAINS[prec] if prec else 1) * e32


# ------------------------------------------------------------------------------------------ operand rounding
def bf16_rne(a):
    """bf16(a) as float32 (``tensor.to(torch.bfloat16)`` rounds to nearest even)"""
    return a.float().to(torch.bfloat16).float()


def split_hi_lo(a):
    """(hi, lo) as float32: hi = bf16(a), lo = bf16(a - hi), the subtraction in fp32 as in ``split2`` (it is exact)"""
    a = a.float()
    hi = bf16_rne(a)
    return hi, bf16_rne(a - hi)


def planes(a, b, prec):
    """the (a-plane, b-plane) pairs whose products the MFMA phases accumulate (module docstring)"""
    ah, al = split_hi_lo(a)
    bh, bl = split_hi_lo(b)
    if prec == "bf16":
        return [(ah, bh)]
    assert prec == "bf16x3", prec
    return [(al, bh), (ah, bl), (ah, bh)]


def affine_operand(x, sc=None, sh=None):
    """the fp32 value a kernel splits: fmaf(x, sc, sh) per channel (module docstring: float32(float64(x) * sc + sh))"""
    if sc is None:
        return x.float()
    assert x.dtype == sc.dtype == sh.dtype == torch.float32
    return (x.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]).float()


def source_operand(x1, sc=None, sh=None, x2=None):
    """cat(affine(x1), x2): the operand of a launch with one or two sources, the affine on the first"""
    a = affine_operand(x1, sc, sh)
    return a if x2 is None else torch.cat([a, x2.float()], 1)


def planes_direct(x, w, prec):
    """the direct kernels' one product plane: (unrounded activation, hi + lo of the weight; hi alone in bf16 mode)"""
    wh, wl = split_hi_lo(w)
    assert prec in ("bf16", "bf16x3"), prec
    return [(x.float(), wh + wl if prec == "bf16x3" else wh)]


def _act_w_planes(act, w, prec, model):
    if prec is None:
        return [(act.float(), w.float())]
    if model == "direct":
        return planes_direct(act, w, prec)
    assert model == "mfma", model
    return planes(act, w, prec)


# ------------------------------------------------------------------------------------------ error measures
def _np(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def chan_err(got, ref, axis=1):
    """max over channels of (max |got - ref| over the channel) / (max |ref| over the channel); an all-zero reference channel must
    be reproduced exactly (it then contributes 0, otherwise inf)"""
    got, ref = _np(got), _np(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.all(np.isfinite(got)):
        return float("inf")
    got, ref = np.moveaxis(got, axis, 0), np.moveaxis(ref, axis, 0)
    d = np.abs(got - ref).reshape(ref.shape[0], -1).max(1)
    s = np.abs(ref).reshape(ref.shape[0], -1).max(1)
    r = np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(r.max())


def sum_err(got, ref, scale):
    """per-channel sums: max over channels of |got - ref| / scale, scale = the channel's sum of |terms|"""
    got, ref, scale = _np(got), _np(ref), _np(scale)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    if not np.all(np.isfinite(got)):
        return float("inf")
    d = np.abs(got - ref)
    r = np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(r.max())


def rel_err(a, b):
    """the project's whole-tensor measure (tests/conftest.py): max |a - b| / max |b|"""
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if not np.all(np.isfinite(a)):
        return float("inf")
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


# ------------------------------------------------------------------------------------------ the three operations
class Geom:
    """(n, cin, cout, h, w, k, stride, pad, dil, in_up): h, w = the LOGICAL input size (doubled already when in_up)"""

    def __init__(self, n, cin, cout, h, w, k, stride=1, pad=0, dil=1, in_up=False):
        self.n, self.cin, self.cout, self.h, self.w, self.k = n, cin, cout, h, w, k
        self.stride, self.pad, self.dil, self.in_up = stride, pad, dil, bool(in_up)
        f = lambda v: (v + 2 * pad - dil * (k - 1) - 1) // stride + 1
        self.oh, self.ow = f(h), f(w)

    @property
    def macs(self):
        return self.n * self.oh * self.ow * self.cout * self.cin * self.k * self.k

    def kw(self):
        return dict(stride=self.stride, padding=self.pad, dilation=self.dil)

    def up(self, x):
        return F.interpolate(x, scale_factor=2, mode="nearest") if self.in_up else x


def _sum_planes(fn, pl, dtype):
    out = None
    for a, b in pl:
        t = fn(a.to(dtype), b.to(dtype))
        out = t if out is None else out + t
    return out


def _lrelu(z, slope):
    return z if slope == 1.0 else torch.where(z > 0, z, z * slope)


def fold2(d):
    """the nearest-x2 backward: 2x2 sums"""
    n, c, h, w = d.shape
    return d.reshape(n, c, h // 2, 2, w // 2, 2).sum((3, 5))


def forward_ref(g, x, w, b, slope, prec, dtype=torch.float64, model="mfma"):
    """y = lrelu(conv(up(x), w) + b) on the kernels' operand planes (prec) or on the unrounded operands (prec=None), evaluated
    in ``dtype``.  x is the STORED input (half resolution when in_up: rounding commutes with the nearest-x2 fold); with an
    affine on load or two sources: ``source_operand(...)``.  model: "mfma" or "direct" (module docstring)."""
    xu = g.up(x.float())
    pl = _act_w_planes(xu, w, prec, model)
    z = _sum_planes(lambda a, c: F.conv2d(a, c, None, **g.kw()), pl, dtype)
    if b is not None:
        z = z + b.to(dtype)[None, :, None, None]
    return _lrelu(z, slope)


def dgrad_ref(g, dy, w, prec, dtype=torch.float64, base=None, mask=None, fold=False, model="mfma"):
    """dx (logical resolution; folded 2x2 when ``fold``) = conv^T(dy, w) [+ base] [* (a > 0 ? 1 : slope), mask = (a, slope)]"""
    pl = _act_w_planes(dy, w, prec, model)
    size = (g.n, g.cin, g.h, g.w)
    d = _sum_planes(lambda a, c: G.conv2d_input(size, c, a, **g.kw()), pl, dtype)
    if fold:
        d = fold2(d)
    if base is not None:
        d = d + base.to(dtype)
    if mask is not None:
        a, slope = mask
        d = torch.where(a > 0, d, d * slope)
    return d


def wgrad_ref(g, x, dz, prec, dtype=torch.float64, base=None):
    """dw = sum over pixels of dz x up(x) [+ base]; the rounded pair is (dz, x)"""
    xu = g.up(x.float())
    pl = [(dz.float(), xu)] if prec is None else planes(dz, xu, prec)
    size = (g.cout, g.cin, g.k, g.k)
    d = _sum_planes(lambda a, c: G.conv2d_weight(c, size, a, **g.kw()), pl, dtype)
    if base is not None:
        d = d + base.to(dtype)
    return d


def chan_sums(t, dtype=torch.float64):
    """(sum, sum of |terms|) per channel of an NCHW tensor"""
    t = t.to(dtype)
    return t.sum((0, 2, 3)), t.abs().double().sum((0, 2, 3))


def bn_fwd_sums(y, dtype=torch.float64):
    """the forward BatchNorm partial sums of the exact output: (Sy, Sy^2) and their |term| scales"""
    y = y.to(dtype)
    s1, a1 = chan_sums(y, dtype)
    s2, a2 = chan_sums(y * y, dtype)
    return (s1, a1), (s2, a2)


def bnred_sums(gd, a, mean, invstd, dtype=torch.float64):
    """the dgrad ``bnred`` partial sums of the exact gradient: (Sg, Sg a_hat), a_hat = (a - mean) * invstd, and their scales"""
    gd = gd.to(dtype)
    ahat = (a.to(dtype) - mean.to(dtype)[None, :, None, None]) * invstd.to(dtype)[None, :, None, None]
    s1, a1 = chan_sums(gd, dtype)
    s2, a2 = chan_sums(gd * ahat, dtype)
    return (s1, a1), (s2, a2)


def e32_of(fn, measure=chan_err, **kw):
    """fn(dtype) evaluated in float32 against float64, in ``measure``: (e32, the float64 value)"""
    r64 = fn(torch.float64)
    r32 = fn(torch.float32)
    assert r32.dtype == torch.float32 and r64.dtype == torch.float64
    return measure(r32, r64, **kw), r64


# ------------------------------------------------------------------------------------------ variant keys (csrc/variants.h)
_PF_W = {0: 0, 1: 1, 2: 3, 3: 2}       # wgrad_key: pf 0 / 1 / 2 / 3 -> the two-bit code
_PF_W_INV = {v: k for k, v in _PF_W.items()}
_TAPS_W = {1: 0, 9: 1, 16: 2}
_TAPS_W_INV = {v: k for k, v in _TAPS_W.items()}


def pipe_key(x3, co_blks, clamp, npb, pf, xq, stats, te):
    return (int(x3) | (co_blks - 1) << 1 | int(clamp) << 2 | (npb - 1) << 3 | (pf - 1) << 4 | int(xq) << 6 | stats << 7 |
            int(te) << 9)


def pipe_fields(key):
    return dict(x3=key & 1, co_blks=(key >> 1 & 1) + 1, clamp=key >> 2 & 1, npb=(key >> 3 & 1) + 1, pf=(key >> 4 & 3) + 1,
                xq=key >> 6 & 1, stats=key >> 7 & 3, te=key >> 9 & 1)


def ig8_key(x3, co_blks, clamp, npbt, pf, xq, stats):
    return (int(x3) | (co_blks - 1) << 1 | int(clamp) << 2 | int(npbt == 8) << 3 | (pf - 1) << 4 | int(xq) << 6 |
            int(stats) << 7)


def ig8_fields(key):
    return dict(x3=key & 1, co_blks=(key >> 1 & 1) + 1, clamp=key >> 2 & 1, npbt=8 if key >> 3 & 1 else 4,
                pf=(key >> 4 & 3) + 1, xq=key >> 6 & 1, stats=key >> 7 & 1)


def wgrad_key(x3, co_blks, mode, taps_max, pf, nw, xq):
    return (int(x3) | (co_blks - 1) << 1 | mode << 2 | _TAPS_W[taps_max] << 4 | _PF_W[pf] << 6 | int(nw == 8) << 8 |
            int(xq) << 9)


def wgrad_fields(key):
    return dict(x3=key & 1, co_blks=(key >> 1 & 1) + 1, mode=key >> 2 & 3, taps_max=_TAPS_W_INV.get(key >> 4 & 3),
                pf=_PF_W_INV[key >> 6 & 3], nw=8 if key >> 8 & 1 else 4, xq=key >> 9 & 1)


KEY_FN = {"pipe": pipe_key, "ig8": ig8_key, "wgrad": wgrad_key}
FIELDS_FN = {"pipe": pipe_fields, "ig8": ig8_fields, "wgrad": wgrad_fields}
KEY_BITS = {"pipe": 10, "ig8": 8, "wgrad": 10}


def fields_legal(family, f):
    """what the dispatch tables can instantiate (launch_pipe_* / igemm8_dispatch in csrc/conv_igemm_impl.h, wgrad_dispatch in
    csrc/conv_wgrad_impl.h)"""
    if family == "pipe":
        # pf 1..3; stats 0 / 1 / 2, 2 (the fused BatchNorm-backward reduce) only on the transposed epilogue
        return f["pf"] in (1, 2, 3) and f["stats"] in (0, 1, 2) and (f["stats"] != 2 or f["te"] == 1)
    if family == "ig8":
        # pf 1..2; 128-pixel tiles (npbt 4) only with two row blocks
        return f["pf"] in (1, 2) and (f["npbt"] == 8 or f["co_blks"] == 2)
    if family == "wgrad":
        if f["taps_max"] is None or f["mode"] > 2:
            return False
        if f["nw"] == 8:      # eight waves: 16-tap groups, pf 1 / 2
            return f["taps_max"] == 16 and f["pf"] in (1, 2)
        # four waves: pf 0 / 1 / 3; quad staging needs a register prefetch
        return f["pf"] in (0, 1, 3) and (f["xq"] == 0 or f["pf"] > 0)
    raise KeyError(family)


def variant_id(family, key):
    """e.g. ``wgrad-663-bf16x3-cb2-mode1-t9-pf3-xq``"""
    f = FIELDS_FN[family](key)
    parts = [family, str(key), "bf16x3" if f["x3"] else "bf16", "cb%d" % f["co_blks"]]
    if family == "wgrad":
        parts += ["mode%d" % f["mode"], "t%s" % f["taps_max"], "pf%d" % f["pf"]] + (["w8"] if f["nw"] == 8 else [])
    else:
        parts += (["clamp"] if f["clamp"] else []) + ["npb%d" % (f["npb"] if family == "pipe" else f["npbt"]), "pf%d" % f["pf"]]
    parts += ["xq"] if f["xq"] else []
    if family != "wgrad" and f["stats"]:
        parts += ["stats%d" % f["stats"]]
    if family == "pipe" and f["te"]:
        parts += ["te"]
    return "-".join(parts)


def parse_built_variants(path=BUILT_VARIANTS):
    """({'pipe': [...], 'ig8': [...], 'wgrad': [...]}, (n_pipe, n_ig8, n_wgrad) of the header's comment)"""
    with open(path) as fh:
        text = fh.read()
    out = {}
    for fam, macro in (("pipe", "PCUDA_BUILT_PIPE"), ("ig8", "PCUDA_BUILT_IG8"), ("wgrad", "PCUDA_BUILT_WGRAD")):
        m = re.search(r"#define\s+%s\s+(.*)" % macro, text)
        out[fam] = [int(v) for v in re.findall(r"(\d+)u", m.group(1))]
    m = re.search(r"(\d+)\s*\+\s*(\d+)\s*\+\s*(\d+)\s+instantiations", text)
    return out, tuple(int(v) for v in m.groups())
