"""torch-tensor front end of the C ABI (ctypes calls on torch's current HIP stream).

torch is used here for device memory (``torch.empty``) and the stream handle only; every
arithmetic step is a kernel of libpcuda_hip.so.  There is no fallback: a tensor that is not
on a HIP device, or a missing library, raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref
from typing import Optional, Tuple

import torch

from . import _lib as L
from ._lib import ACT_SIGMOID, ACT_SOFTMAX, PREC_BF16, PREC_BF16X3, ConvGeom, Dst, Src, check

_PREC = {"bf16x3": PREC_BF16X3, "bf16": PREC_BF16}
_precision = _PREC.get(os.environ.get("PCUDA_PRECISION", "bf16x3").lower(), PREC_BF16X3)


def set_precision(name: str) -> None:
    """'bf16x3' (parity mode: split-bf16 MFMA, ~fp32 accuracy) or 'bf16' (throughput mode)."""
    global _precision
    _precision = _PREC[name.lower()]


def get_precision() -> str:
    return "bf16x3" if _precision == PREC_BF16X3 else "bf16"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError("pointcloududa_amd kernels need HIP device tensors (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError("expected %s, got %s" % (dtype, t.dtype))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _images(what, t, dtypes=(torch.uint8,), dim=4):
    """the head of the image wrappers: a device tensor of one of ``dtypes`` with ``dim`` dimensions -> (the contiguous
    tensor, its shape)"""
    layout = "[B,H,W,C] images" if dim == 4 else "[N,H,W] slices"
    if len(dtypes) == 1:
        _req(t, dtypes[0])
        layout = "uint8 " + layout
    else:
        if t.dtype not in dtypes:
            raise TypeError("%s: fp32 or uint8 images, got %s" % (what, t.dtype))
        _req(t, t.dtype)
    if t.dim() != dim:
        raise TypeError("%s: %s" % (what, layout))
    t = t.contiguous()
    return t, tuple(t.shape)


def _program(what, b, opcode, seed, **columns):
    """a slot program's device arrays against a batch of ``b``: ``opcode`` int32 and ``seed`` int64 ``[b,S]``, every column
    ``name=(tensor, dtype, width)`` ``[b,S,width]`` -> (S, the contiguous tensors: opcode, the columns in order, seed)"""
    cols = list(columns.values())
    _req(opcode, torch.int32)
    for t, dtype, _ in cols:
        _req(t, dtype)
    _req(seed, torch.int64)
    slots = opcode.shape[1] if opcode.dim() == 2 else -1
    if tuple(opcode.shape) != (b, slots) or tuple(seed.shape) != (b, slots) or \
            any(tuple(t.shape) != (b, slots, n) for t, _, n in cols):
        raise ValueError("%s: the program's arrays do not match the batch of %d" % (what, b))
    return slots, [t.contiguous() for t in [opcode] + [c[0] for c in cols] + [seed]]


def _workspace(nbytes, device):
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def _out(what, out, like, name="out"):
    """a caller's result tensor checked before anything is launched (the entry points only see a pointer): ``None`` -> a new
    tensor like ``like``; else a contiguous device tensor of ``like``'s dtype and shape"""
    if out is None:
        return torch.empty_like(like)
    if not torch.is_tensor(out) or not out.is_cuda or out.dtype != like.dtype or out.shape != like.shape or \
            not out.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s tensor of shape %s"
                         % (what, name, str(like.dtype).replace("torch.", ""), list(like.shape)))
    return out


def _labels_io(what, labels, labels_out, shape):
    """the optional int32 labels next to images of ``shape`` ``(b, h, w)`` and their result tensor -> (the contiguous labels,
    ``labels_out``), or ``(None, None)`` without labels"""
    if labels is None:
        return None, None
    _req(labels, torch.int32)
    labels = labels.contiguous()
    if tuple(labels.shape) != shape:
        raise ValueError("%s: label shape %r does not match the images" % (what, tuple(labels.shape)))
    return labels, _out(what, labels_out, labels, "labels_out")


def _planes(t: torch.Tensor) -> Tuple[int, int, int, int, int]:
    """(n, c, hw, sn, sc) of a [N,C,...] tensor whose trailing dims form a dense plane."""
    _req(t)
    n, c = t.shape[0], t.shape[1]
    hw = 1
    for d in t.shape[2:]:
        hw *= d
    exp = 1
    for d in range(t.dim() - 1, 1, -1):
        if t.shape[d] != 1 and t.stride(d) != exp:
            raise ValueError("tensor planes must be dense (shape %s strides %s)" % (tuple(t.shape), t.stride()))
        exp *= t.shape[d]
    return n, c, hw, t.stride(0), t.stride(1)


class TA:
    """A tensor with an optional per-channel affine still to be applied on load
    (= a BatchNorm output that was never materialised)."""
    __slots__ = ("t", "scale", "shift")

    def __init__(self, t, scale=None, shift=None):
        self.t, self.scale, self.shift = t, scale, shift


def _as_ta(x):
    return x if isinstance(x, TA) else TA(x)


def make_src(a, b=None) -> Src:
    a = _as_ta(a)
    _, c1, _, sn1, sc1 = _planes(a.t)
    s = Src()
    s.p1, s.sn1, s.sc1, s.scale1, s.shift1, s.c1 = a.t.data_ptr(), sn1, sc1, _ptr(a.scale), _ptr(a.shift), c1
    if b is not None:
        b = _as_ta(b)
        _, _, _, sn2, sc2 = _planes(b.t)
        s.p2, s.sn2, s.sc2, s.scale2, s.shift2 = b.t.data_ptr(), sn2, sc2, _ptr(b.scale), _ptr(b.shift)
    return s


def make_dst(a: torch.Tensor, b: Optional[torch.Tensor] = None) -> Dst:
    _, c1, _, sn1, sc1 = _planes(a)
    d = Dst()
    d.p1, d.sn1, d.sc1, d.c1 = a.data_ptr(), sn1, sc1, c1
    if b is not None:
        _, _, _, sn2, sc2 = _planes(b)
        d.p2, d.sn2, d.sc2 = b.data_ptr(), sn2, sc2
    return d


# ------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------
# PCUDA_BNRED=0: the BatchNorm-backward reduce of a block's first BatchNorm as its own kernel instead of riding in the
# epilogue of the second convolution's dgrad (A/B switch)
_fuse_bnred = os.environ.get("PCUDA_BNRED", "1") != "0"
# PCUDA_FOLD_DGRAD=0: the 2x2 fold behind an up-convolution's data gradient as its own kernel (upsample2_bwd) again (A/B switch)
_fold_dgrad = os.environ.get("PCUDA_FOLD_DGRAD", "1") != "0"


def upsample_red_only(dx, bnred):
    """(dx, None): the caller computes the BatchNorm-backward reduce of ``dx`` itself (bn_backward without ``red``)"""
    return dx, None


_conv_ops = weakref.WeakSet()      # every ConvOp alive (repack_owner finds a network's layers through their ``owner``)


class ConvOp:
    """Geometry + packed-weight cache of one nn.Conv2d (square kernel, groups=1)."""

    def __init__(self, cin, cout, k, stride=1, pad=0, dil=1, in_up=False):
        self.cin, self.cout, self.k, self.stride, self.pad, self.dil, self.in_up = cin, cout, k, stride, pad, dil, in_up
        self._pk = {}     # (kind, prec) -> (weight ptr, version, generation, packed tensor)
        self._last_fwd = None   # (weight tensor, geometry) of the latest forward-layout pack: what repack_owner replays
        _conv_ops.add(self)
        # training: a forward-layout repack is followed by a dgrad in the same step, so both go out in one launch;
        # set False for layers whose input never needs a gradient / for inference-only use
        self.pack_dgrad_with_fwd = os.environ.get("PCUDA_PACK_ALL", "1") != "0"
        self.owner = None  # object whose ``_wgen`` counter is bumped when weights change behind torch's back

    def out_hw(self, in_h, in_w):
        f = lambda v: (v + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1
        return f(in_h), f(in_w)

    def geom(self, n, in_h, in_w) -> ConvGeom:
        """in_h/in_w: LOGICAL input size (already doubled when in_up)."""
        oh, ow = self.out_hw(in_h, in_w)
        return ConvGeom(n, self.cin, self.cout, in_h, in_w, oh, ow, self.k, self.stride, self.pad, self.dil,
                        1 if self.in_up else 0)

    def _packed(self, kind: str, w: torch.Tensor, g: ConvGeom):
        key = (kind, _precision)
        hit = self._pk.get(key)
        gen = getattr(self.owner, "_wgen", 0)
        if hit is not None and hit[0] == w.data_ptr() and hit[1] == w._version and hit[2] == gen:
            return hit[3]
        _req(w)
        if not w.is_contiguous():
            raise ValueError("conv weight must be contiguous OIHW")
        lib = L.lib()
        if kind == "fwd":
            nbytes = lib.pcuda_conv2d_packed_fwd_bytes(C.byref(g), _precision)
        else:
            nbytes = lib.pcuda_conv2d_packed_dgrad_bytes(C.byref(g), _precision)
        if nbytes == 0:
            raise RuntimeError("conv geometry rejected by libpcuda_hip")
        buf = hit[3] if (hit is not None and hit[3].numel() == nbytes) else torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        if kind == "fwd" and self.pack_dgrad_with_fwd:
            # the weights changed (optimiser step): repack the forward layout AND the dgrad layouts in one launch
            dkey = ("dgrad", _precision)
            dhit = self._pk.get(dkey)
            dbytes = lib.pcuda_conv2d_packed_dgrad_bytes(C.byref(g), _precision)
            dbuf = dhit[3] if (dhit is not None and dhit[3].numel() == dbytes) else torch.empty(
                dbytes, dtype=torch.uint8, device=w.device)
            check(lib.pcuda_conv2d_pack_all(C.byref(g), _precision, w.data_ptr(), buf.data_ptr(), dbuf.data_ptr(),
                                            _stream()), "pack_all")
            self._pk[dkey] = (w.data_ptr(), w._version, gen, dbuf)
        else:
            fn = lib.pcuda_conv2d_pack_fwd if kind == "fwd" else lib.pcuda_conv2d_pack_dgrad
            check(fn(C.byref(g), _precision, w.data_ptr(), buf.data_ptr(), _stream()), "pack_" + kind)
        self._pk[key] = (w.data_ptr(), w._version, gen, buf)
        if kind == "fwd":
            self._last_fwd = (w, g)
        return buf

    def forward(self, x, w, b, slope, in_h, in_w, x2=None, out=None, want_stats=False):
        """x (and x2 for a channel concat): tensors or TA.  Returns (y, partials|None, ntiles)."""
        xa = _as_ta(x)
        n = xa.t.shape[0]
        g = self.geom(n, in_h, in_w)
        if out is None:
            out = torch.empty((n, self.cout, g.out_h, g.out_w), dtype=torch.float32, device=w.device)
        pk = self._packed("fwd", w, g)
        lib = L.lib()
        partials, nt = None, 0
        if want_stats:
            nt = lib.pcuda_conv2d_fwd_tiles(C.byref(g), _precision)
            partials = torch.empty((nt, self.cout, 2), dtype=torch.float32, device=w.device)
        src, dst = make_src(xa, x2), make_dst(out)
        rc = lib.pcuda_conv2d_forward(C.byref(g), _precision, C.byref(src), pk.data_ptr(), _ptr(b), float(slope),
                                      C.byref(dst), _ptr(partials), _stream())
        if rc == L.PCUDA_E_UNSUPPORTED and want_stats:
            # the partial sums are sized by the tiles of the kernel the GEOMETRY selects (pcuda_conv2d_fwd_tiles); a view that
            # kernel cannot address (off its alignment, split) runs on one with other tiles: the convolution without
            # statistics, then the statistics of what it stored as their own kernel
            check(lib.pcuda_conv2d_forward(C.byref(g), _precision, C.byref(src), pk.data_ptr(), _ptr(b), float(slope),
                                           C.byref(dst), None, _stream()), "conv2d_forward")
            partials, nt, _ = bn_stats(out)
            return out, partials, nt
        check(rc, "conv2d_forward")
        return out, partials, nt

    def dgrad(self, dy, w, in_h, in_w, dx=None, dx2=None, accumulate=False, bnred=None):
        """dy: [n,cout,oh,ow].  dx (+dx2 split along channels) = gradient of the logical input.
        ``bnred=(a, BNState)``: the BatchNorm-backward reduce of the layer in front of this convolution rides in the
        epilogue; returns (dx, (partials, ntiles)) -- or (dx, None) where the geometry does not allow it."""
        n = dy.shape[0]
        g = self.geom(n, in_h, in_w)
        if dx is None:
            dx = torch.empty((n, self.cin, in_h, in_w), dtype=torch.float32, device=dy.device)
        pk = self._packed("dgrad", w, g)
        src, dst = make_src(dy), make_dst(dx, dx2)
        if bnred is not None:
            a, st = bnred
            lib = L.lib()
            nt = lib.pcuda_conv2d_dgrad_tiles(C.byref(g), _precision) if (_fuse_bnred and dx2 is None) else 0
            if nt > 0:
                _, _, _, asn, asc = _planes(a)
                red = torch.empty((nt, self.cin, 2), dtype=torch.float32, device=dy.device)
                rc = lib.pcuda_conv2d_dgrad_bnred(C.byref(g), _precision, C.byref(src), pk.data_ptr(), C.byref(dst),
                                                  1 if accumulate else 0, a.data_ptr(), asn, asc, st.mean.data_ptr(),
                                                  st.invstd.data_ptr(), red.data_ptr(), _stream())
                if rc == 0:
                    return dx, (red, nt)
                if rc != L.PCUDA_E_UNSUPPORTED:
                    check(rc, "conv2d_dgrad_bnred")
            check(lib.pcuda_conv2d_dgrad(C.byref(g), _precision, C.byref(src), pk.data_ptr(), C.byref(dst),
                                         1 if accumulate else 0, _stream()), "conv2d_dgrad")
            return dx, None
        check(L.lib().pcuda_conv2d_dgrad(C.byref(g), _precision, C.byref(src), pk.data_ptr(), C.byref(dst),
                                         1 if accumulate else 0, _stream()), "conv2d_dgrad")
        return dx

    def dgrad_lrelu(self, dy, w, in_h, in_w, a, slope):
        """lrelu_bwd(dgrad(dy), a, slope) in one kernel where the plan allows it (pcuda_conv2d_dgrad_lrelu): the LeakyReLU
        backward of the layer in front rides in the data-gradient epilogue (GAN.py:97-108 going back)"""
        if _fuse_lrelu_dgrad and self.k > 1 and a.is_contiguous():
            n = dy.shape[0]
            g = self.geom(n, in_h, in_w)
            dz = torch.empty((n, self.cin, in_h, in_w), dtype=torch.float32, device=dy.device)
            pk = self._packed("dgrad", w, g)
            src, dst = make_src(dy), make_dst(dz)
            _, _, _, asn, asc = _planes(a)
            rc = L.lib().pcuda_conv2d_dgrad_lrelu(C.byref(g), _precision, C.byref(src), pk.data_ptr(), C.byref(dst),
                                                  a.data_ptr(), asn, asc, float(slope), _stream())
            if rc == 0:
                return dz
            if rc != L.PCUDA_E_UNSUPPORTED:
                check(rc, "conv2d_dgrad_lrelu")
        return lrelu_bwd(self.dgrad(dy, w, in_h, in_w), a, slope)

    def dgrad_fold(self, dy, w, in_h, in_w, bnred=None):
        """The data gradient of an ``in_up`` layer at the STORED (half) resolution: dgrad + the 2x2 fold of the nearest-x2
        backward in one kernel (pcuda_conv2d_dgrad_fold); ``bnred=(a, BNState)`` as in ``dgrad``.  Returns (dx_half, (partials,
        ntiles) | None) like ``upsample2_bwd(dgrad(...), bnred)``, which it falls back to where the plan does not fold."""
        assert self.in_up
        n = dy.shape[0]
        g = self.geom(n, in_h, in_w)
        lib = L.lib()
        if _fold_dgrad and in_h % 2 == 0 and in_w % 4 == 0:
            pk = self._packed("dgrad", w, g)
            dx = torch.empty((n, self.cin, in_h // 2, in_w // 2), dtype=torch.float32, device=dy.device)
            src, dst = make_src(dy), make_dst(dx)
            a_p = m_p = i_p = r_p = None
            asn = asc = 0
            red, nt = None, 0
            if bnred is not None and _fuse_bnred:
                a, st = bnred
                nt = lib.pcuda_conv2d_dgrad_tiles(C.byref(g), _precision)
                if nt > 0:
                    _, _, _, asn, asc = _planes(a)
                    red = torch.empty((nt, self.cin, 2), dtype=torch.float32, device=dy.device)
                    a_p, m_p, i_p, r_p = a.data_ptr(), st.mean.data_ptr(), st.invstd.data_ptr(), red.data_ptr()
            rc = lib.pcuda_conv2d_dgrad_fold(C.byref(g), _precision, C.byref(src), pk.data_ptr(), C.byref(dst), a_p, asn, asc,
                                             m_p, i_p, r_p, _stream())
            if rc == 0:
                if bnred is None:
                    return dx
                return (dx, (red, nt)) if red is not None else upsample_red_only(dx, bnred)
            if rc != L.PCUDA_E_UNSUPPORTED:
                check(rc, "conv2d_dgrad_fold")
        d_up = self.dgrad(dy, w, in_h, in_w)
        return upsample2_bwd(d_up, bnred=bnred)

    def wgrad(self, x, dy, dw, db, in_h, in_w, x2=None, accumulate=True):
        xa = _as_ta(x)
        n = xa.t.shape[0]
        g = self.geom(n, in_h, in_w)
        lib = L.lib()
        ws_bytes = lib.pcuda_conv2d_wgrad_workspace_size(C.byref(g))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dy.device)
        _, _, _, sn, sc = _planes(dy)
        src = make_src(xa, x2)
        pend = getattr(_deferred, "jobs", None)
        if pend is not None:
            # inside ``deferred_wgrad_reduces()``: only the partial sums now; the split-K reduce of every layer of the
            # pass goes out in one launch when the block ends (the workspace lives in the pending list until then)
            job = L.ReduceJob()
            check(lib.pcuda_conv2d_wgrad_partial(C.byref(g), _precision, C.byref(src), dy.data_ptr(), sn, sc, dw.data_ptr(),
                                                 _ptr(db), 1 if accumulate else 0, ws.data_ptr(), ws_bytes, C.byref(job),
                                                 _stream()), "conv2d_wgrad_partial")
            if job.ksplit > 0:
                if any(j.dw == job.dw for j, _ in pend):
                    flush_wgrad_reduces()        # two gradients into one buffer: keep their order
                pend.append((job, ws))
                if _batch_reduce_n >= 2 and len(pend) >= _batch_reduce_n:
                    flush_wgrad_reduces()
            return
        check(lib.pcuda_conv2d_wgrad(C.byref(g), _precision, C.byref(src), dy.data_ptr(), sn, sc, dw.data_ptr(),
                                     _ptr(db), 1 if accumulate else 0, ws.data_ptr(), ws_bytes, _stream()),
              "conv2d_wgrad")


# PCUDA_BATCH_REDUCE=1: the split-K reduces of a backward pass in one launch per 56 layers instead of one per layer.
# OFF by default -- measured SLOWER (51.7 vs 49.5 ms per step, same box): a layer's partial sums (~35 MB) are still in
# the 256 MB infinity cache when its own reduce follows at once, and the workspace block is reused by the next layer; all
# of a pass's partials together (~1.4 GB) go out to HBM and come back.  The launches were not the cost.
# PCUDA_BATCH_REDUCE=k (k >= 2): flush every k layers -- the pending slabs (k x ~35 MB) stay inside the infinity cache.
_batch_reduce_n = int(os.environ.get("PCUDA_BATCH_REDUCE", "0") or 0)
_batch_reduce = _batch_reduce_n >= 1
_deferred = threading.local()


def flush_wgrad_reduces():
    """Run the pending split-K reduces of this thread's ``deferred_wgrad_reduces`` block (one launch per 56 layers).
    Call before anything reads the weight gradients inside the block (e.g. the all-reduce hook of the backward pass)."""
    pend = getattr(_deferred, "jobs", None)
    if not pend:
        return
    arr = (L.ReduceJob * len(pend))(*[j for j, _ in pend])
    check(L.lib().pcuda_wgrad_reduce_batch(arr, len(pend), _stream()), "wgrad_reduce_batch")
    del pend[:]          # (stream order keeps the workspaces valid: the allocator reuses them behind the reduce)


class deferred_wgrad_reduces:
    """``with deferred_wgrad_reduces():`` around one backward pass of a network (one stream, each weight once)."""

    def __enter__(self):
        self.outer = getattr(_deferred, "jobs", None)
        if _batch_reduce and self.outer is None:
            _deferred.jobs = []
        return self

    def __exit__(self, *exc):
        if _batch_reduce and self.outer is None:
            try:
                if exc[0] is None:
                    flush_wgrad_reduces()
            finally:
                _deferred.jobs = None
        return False


_batch_repack = os.environ.get("PCUDA_PACK_TABLE", "1") != "0"


def repack_owner(owner):
    """All packed-weight layouts of ``owner``'s convolutions in ONE launch (called behind the optimiser kernel that
    changed the weights).  The jobs -- raw pointers of the flat master weights and of the packed buffers, which both
    stay put -- are collected once into a device table and replayed every step; layers that have not run yet (no
    packed buffers) keep the lazy per-layer path.  Lazily, the segmenter's 43 repack launches sat in the dependent
    chain of the next forward pass."""
    if not _batch_repack:
        return False
    lib = L.lib()
    ops = [op for op in _conv_ops if op.owner is owner and op._last_fwd is not None]
    if not ops:
        return False
    gen = getattr(owner, "_wgen", 0)
    key, entries = [], []
    for op in ops:
        w, g = op._last_fwd
        fhit = op._pk.get(("fwd", _precision))
        dhit = op._pk.get(("dgrad", _precision)) if op.pack_dgrad_with_fwd else None
        if fhit is None or fhit[0] != w.data_ptr() or (op.pack_dgrad_with_fwd and dhit is None):
            continue
        entries.append((op, w, g, fhit[3], None if dhit is None else dhit[3]))
        key.append((id(op), w.data_ptr(), fhit[3].data_ptr(), 0 if dhit is None else dhit[3].data_ptr()))
    if not entries:
        return False
    key = (tuple(sorted(key)), _precision)
    tab = getattr(owner, "_pack_table", None)
    if tab is None or tab[0] != key:
        jb = lib.pcuda_conv2d_pack_job_bytes()
        chunks, blocks = [], []
        for op, w, g, fb, db in entries:
            host = C.create_string_buffer(jb * 8)
            jblk = (C.c_int * 8)()
            nj = lib.pcuda_conv2d_pack_jobs_fill(C.byref(g), _precision, w.data_ptr(), fb.data_ptr(),
                                                 None if db is None else db.data_ptr(), host, 8, jblk)
            if nj < 0:
                check(nj, "pack_jobs_fill")
            chunks.append(host.raw[:jb * nj]); blocks += list(jblk[:nj])
        dev = entries[0][1].device
        blob = torch.frombuffer(bytearray(b"".join(chunks)), dtype=torch.uint8).to(dev)
        first = torch.tensor([sum(blocks[:j]) for j in range(len(blocks))], dtype=torch.int32).to(dev)
        tab = (key, blob, first, len(blocks), sum(blocks))
        owner._pack_table = tab
    check(lib.pcuda_conv2d_pack_table(tab[1].data_ptr(), tab[2].data_ptr(), tab[3], tab[4], _stream()), "pack_table")
    for op, w, g, fb, db in entries:          # the caches are current for this weight generation
        op._pk[("fwd", _precision)] = (w.data_ptr(), w._version, gen, fb)
        if db is not None:
            op._pk[("dgrad", _precision)] = (w.data_ptr(), w._version, gen, db)
    return True


# ------------------------------------------------------------------------------------------
# BatchNorm pieces
# ------------------------------------------------------------------------------------------
class BNState:
    """per-forward statistics of one BatchNorm layer"""
    __slots__ = ("mean", "invstd", "scale", "shift", "count")

    @classmethod
    def empty(cls, c, count, device):
        """the four [c] vectors a finalize kernel fills (one buffer) and the element count they stand for"""
        st = cls()
        buf = torch.empty((4, c), dtype=torch.float32, device=device)
        st.mean, st.invstd, st.scale, st.shift, st.count = buf[0], buf[1], buf[2], buf[3], count
        return st


def _opt_planes(t: Optional[torch.Tensor]):
    """(pointer, batch stride, channel stride) of an optional [N,C,...] tensor; (None, 0, 0) where there is none"""
    return (None, 0, 0) if t is None else (t.data_ptr(),) + _planes(t)[3:]


def _ntiles(n, c, hw):
    """tiles of n x c planes of hw elements as the library counts them (pcuda_bn_stats' query form: nothing is launched)"""
    nt = C.c_int(0)
    check(L.lib().pcuda_bn_stats(None, 0, 0, n, c, hw, None, C.byref(nt), None), "bn_stats(query)")
    return nt.value


def bn_finalize(partials, ntiles, count, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1) -> BNState:
    c = partials.shape[1]
    st = BNState.empty(c, count, partials.device)
    check(L.lib().pcuda_bn_finalize(partials.data_ptr(), ntiles, c, count, _ptr(gamma), _ptr(beta), eps, momentum,
                                    _ptr(running_mean), _ptr(running_var), st.mean.data_ptr(), st.invstd.data_ptr(),
                                    st.scale.data_ptr(), st.shift.data_ptr(), _stream()), "bn_finalize")
    return st


def bn_stats(a: torch.Tensor):
    n, c, hw, sn, sc = _planes(a)
    nt = _ntiles(n, c, hw)
    partials = torch.empty((nt, c, 2), dtype=torch.float32, device=a.device)
    check(L.lib().pcuda_bn_stats(a.data_ptr(), sn, sc, n, c, hw, partials.data_ptr(), None, _stream()), "bn_stats")
    return partials, nt, n * hw


def bn_apply(a: torch.Tensor, st: BNState, relu=False, out=None, fma=False):
    """a * scale + shift per channel (then relu).  ``fma``: rounded once, as a convolution applies a pending BatchNorm
    (``TA``) in its load -- the value the fused network's next layer reads"""
    n, c, hw, sn, sc = _planes(a)
    if out is None:
        out = torch.empty_like(a, memory_format=torch.contiguous_format)
    _, _, _, osn, osc = _planes(out)
    flags = (1 if relu else 0) | (2 if fma else 0)      # PCUDA_BN_APPLY_RELU | PCUDA_BN_APPLY_FMA
    check(L.lib().pcuda_bn_apply(a.data_ptr(), sn, sc, st.scale.data_ptr(), st.shift.data_ptr(), flags,
                                 out.data_ptr(), osn, osc, n, c, hw, _stream()), "bn_apply")
    return out


# PCUDA_PN_SMALL=0: the point-cloud discriminator's small tensors take the general kernels (one element per workgroup on
# [B, C], the dense gradient behind the max over points) instead of csrc/pointnet_small.hip -- same bits, the A/B switch
_pn_small = os.environ.get("PCUDA_PN_SMALL", "1") != "0"


def _bn1d_ok(*ts):
    """[B, C] tensors the one-launch BatchNorm1d kernels take: B <= 1024, channels contiguous"""
    return _pn_small and all(t.dim() == 2 and t.shape[0] <= 1024 and t.stride(1) == 1 and t.shape[1] <= t.stride(0) <= 1 << 20
                             for t in ts)


def bn1d_forward(a, gamma, beta, running_mean, running_var, relu=False, eps=1e-5, momentum=0.1):
    """training BatchNorm1d on [B, C]: (BNState, y) of bn_stats -> bn_finalize -> bn_apply in one launch, or None where
    the fused kernel does not apply (B > 1024, strided channels, PCUDA_PN_SMALL=0)"""
    _req(a)
    if not _bn1d_ok(a):
        return None
    b, c = a.shape
    st = BNState.empty(c, b, a.device)
    y = torch.empty((b, c), dtype=torch.float32, device=a.device)
    check(L.lib().pcuda_bn1d_fwd(a.data_ptr(), a.stride(0), b, c, _ptr(gamma), _ptr(beta), eps, momentum,
                                 _ptr(running_mean), _ptr(running_var), st.mean.data_ptr(), st.invstd.data_ptr(),
                                 st.scale.data_ptr(), st.shift.data_ptr(), 1 if relu else 0, y.data_ptr(), y.stride(0),
                                 _stream()), "bn1d_fwd")
    return st, y


def bn_backward(dy, a, st: BNState, gamma, dgamma, dbeta, dy2=None, post_relu=False, act_slope=1.0,
                accumulate=True, red=None, frozen=False):
    """Backward of [a = lrelu(z, act_slope)] -> BN (post_relu=False) or a -> BN -> ReLU (post_relu=True).
    Returns dz (gradient w.r.t. the pre-activation conv output, or w.r.t. a when post_relu).
    ``frozen``: ``st`` holds the running statistics (eval-mode BatchNorm): the layer is a fixed affine."""
    if dy2 is None and red is None and not frozen and _bn1d_ok(a, dy):
        # [B, C]: reduce, finalize and apply in one launch (a second share, partials from a dgrad epilogue and frozen
        # statistics have no fused form)
        _req(a); _req(dy)
        b, c = a.shape
        dz = torch.empty((b, c), dtype=torch.float32, device=a.device)
        check(L.lib().pcuda_bn1d_bwd(dy.data_ptr(), dy.stride(0), a.data_ptr(), a.stride(0), b, c, _ptr(gamma),
                                     st.mean.data_ptr(), st.invstd.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(),
                                     1 if post_relu else 0, float(act_slope), _ptr(dgamma), _ptr(dbeta),
                                     1 if accumulate else 0, dz.data_ptr(), dz.stride(0), _stream()), "bn1d_bwd")
        return dz
    n, c, hw, asn, asc = _planes(a)
    dyp, d2p = _opt_planes(dy), _opt_planes(dy2)
    lib = L.lib()
    pr = 1 if post_relu else 0
    if red is not None:          # (partials, ntiles) from the producing dgrad's epilogue (ConvOp.dgrad(bnred=...))
        assert dy2 is None and not post_relu

    def reduce():
        if red is not None:
            return red
        part = torch.empty((_ntiles(n, c, hw), c, 2), dtype=torch.float32, device=a.device)
        check(lib.pcuda_bn_bwd_reduce(*dyp, *d2p, a.data_ptr(), asn, asc, st.mean.data_ptr(), st.invstd.data_ptr(),
                                      st.scale.data_ptr(), st.shift.data_ptr(), pr, n, c, hw, part.data_ptr(), None,
                                      _stream()), "bn_bwd_reduce")
        return part, part.shape[0]

    def apply(coef, dz):
        check(lib.pcuda_bn_bwd_apply(*dyp, *d2p, a.data_ptr(), asn, asc, coef.data_ptr(), st.scale.data_ptr(),
                                     st.shift.data_ptr(), pr, float(act_slope), *_opt_planes(dz), n, c, hw, _stream()),
              "bn_bwd_apply")

    return _bn_backward_chain(a, n * hw, st, gamma, dgamma, dbeta, accumulate, frozen, reduce, apply)


def _bn_backward_chain(a, count, st, gamma, dgamma, dbeta, accumulate, frozen, reduce, apply):
    """``reduce()`` -> (partials [ntiles, c, 2], ntiles), pcuda_bn_bwd_finalize (``frozen``: -count), ``apply(coef, dz)``"""
    c = a.shape[1]
    part, ntiles = reduce()
    coef = torch.empty((c, 3), dtype=torch.float32, device=a.device)
    check(L.lib().pcuda_bn_bwd_finalize(part.data_ptr(), ntiles, c, -count if frozen else count, _ptr(gamma),
                                        st.invstd.data_ptr(), st.mean.data_ptr(), _ptr(dgamma), _ptr(dbeta),
                                        1 if accumulate else 0, coef.data_ptr(), _stream()), "bn_bwd_finalize")
    dz = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    apply(coef, dz)
    return dz


def make_pooled(g, idx, h, w, g2=None):
    """gradient arriving through a 2x2 max-pool, read in place by the kernel that consumes it (pcuda_pooled)"""
    p = L.Pooled()
    p.g, p.g_sn, p.g_sc = _opt_planes(g)
    p.g2, p.g2_sn, p.g2_sc = _opt_planes(g2)
    assert idx.is_contiguous() and idx.dtype == torch.uint8
    p.idx, p.h, p.w = idx.data_ptr(), h, w
    return p


_fuse_pool = os.environ.get("PCUDA_FUSE_POOL_BWD", "1") != "0"
_fuse_lrelu_dgrad = os.environ.get("PCUDA_FUSE_LRELU_DGRAD", "1") != "0"


def lrelu_bwd_pooled(g, idx, a, slope, g2=None, dy=None):
    """lrelu_bwd(maxpool2_bwd(g (+ g2), idx), a, dy2=dy) without the full-resolution intermediate"""
    n, c, hw, asn, asc = _planes(a)
    h, w = a.shape[2], a.shape[3]
    if not _fuse_pool:
        return lrelu_bwd(maxpool2_bwd(g, idx, h, w, dy2=g2), a, slope, dy2=dy)
    dz = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    pool = make_pooled(g, idx, h, w, g2)
    check(L.lib().pcuda_lrelu_bwd_pooled(C.byref(pool), *_opt_planes(dy), a.data_ptr(), asn, asc, float(slope),
                                         *_opt_planes(dz), n, c, _stream()), "lrelu_bwd_pooled")
    return dz


def bn_backward_pooled(g, idx, a, st: BNState, gamma, dgamma, dbeta, g2=None, dy=None, act_slope=1.0, accumulate=True,
                       frozen=False):
    """bn_backward(maxpool2_bwd(g (+ g2), idx), a, ..., dy2=dy) without the full-resolution intermediate"""
    n, c, hw, asn, asc = _planes(a)
    h, w = a.shape[2], a.shape[3]
    if not _fuse_pool:
        return bn_backward(maxpool2_bwd(g, idx, h, w, dy2=g2), a, st, gamma, dgamma, dbeta, dy2=dy, act_slope=act_slope,
                           accumulate=accumulate, frozen=frozen)
    lib = L.lib()
    dyp = _opt_planes(dy)
    pool = make_pooled(g, idx, h, w, g2)

    def reduce():
        part = torch.empty((_ntiles(n, c, hw), c, 2), dtype=torch.float32, device=a.device)
        check(lib.pcuda_bn_bwd_reduce_pooled(C.byref(pool), *dyp, a.data_ptr(), asn, asc, st.mean.data_ptr(),
                                             st.invstd.data_ptr(), n, c, part.data_ptr(), None, _stream()),
              "bn_bwd_reduce_pooled")
        return part, part.shape[0]

    def apply(coef, dz):
        check(lib.pcuda_bn_bwd_apply_pooled(C.byref(pool), *dyp, a.data_ptr(), asn, asc, coef.data_ptr(), float(act_slope),
                                            *_opt_planes(dz), n, c, _stream()), "bn_bwd_apply_pooled")

    return _bn_backward_chain(a, n * hw, st, gamma, dgamma, dbeta, accumulate, frozen, reduce, apply)


def lrelu_bwd(dy, a, slope, dy2=None):
    n, c, hw, asn, asc = _planes(a)
    dz = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    check(L.lib().pcuda_lrelu_bwd(*_opt_planes(dy), *_opt_planes(dy2), a.data_ptr(), asn, asc, float(slope),
                                  *_opt_planes(dz), n, c, hw, _stream()), "lrelu_bwd")
    return dz


def channel_sum(dz, db, accumulate=True):
    n, c, hw, sn, sc = _planes(dz)
    ws = torch.empty((_ntiles(n, c, hw), c), dtype=torch.float32, device=dz.device)
    check(L.lib().pcuda_channel_sum(dz.data_ptr(), sn, sc, n, c, hw, db.data_ptr(), 1 if accumulate else 0,
                                    ws.data_ptr(), ws.numel() * 4, _stream()), "channel_sum")


# ------------------------------------------------------------------------------------------
# pooling / resampling / adds
# ------------------------------------------------------------------------------------------
def maxpool2_fwd(x):
    xa = _as_ta(x)
    n, c, _, sn, sc = _planes(xa.t)
    h, w = xa.t.shape[2], xa.t.shape[3]
    y = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=xa.t.device)
    idx = torch.empty((n, c, h // 2, w // 2), dtype=torch.uint8, device=xa.t.device)
    check(L.lib().pcuda_maxpool2_fwd(xa.t.data_ptr(), sn, sc, _ptr(xa.scale), _ptr(xa.shift), y.data_ptr(),
                                     y.stride(0), y.stride(1), idx.data_ptr(), n, c, h, w, _stream()), "maxpool2_fwd")
    return y, idx


def maxpool2_bwd(dy, idx, h, w, dy2=None):
    n, c, _, dsn, dsc = _planes(dy)
    dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dy.device)
    check(L.lib().pcuda_maxpool2_bwd(dy.data_ptr(), dsn, dsc, *_opt_planes(dy2), idx.data_ptr(), dx.data_ptr(),
                                     dx.stride(0), dx.stride(1), 0, n, c, h, w, _stream()), "maxpool2_bwd")
    return dx


def upsample2_bwd(dy, bnred=None):
    """2x2 fold (backward of nearest x2).  ``bnred=(a, BNState)``: the BatchNorm-backward reduce of the layer that
    consumes the result rides along; returns (dx, (partials, ntiles))."""
    n, c, _, dsn, dsc = _planes(dy)
    h, w = dy.shape[2] // 2, dy.shape[3] // 2
    dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dy.device)
    lib = L.lib()
    if bnred is not None and _fuse_bnred:
        a, st = bnred
        _, _, _, asn, asc = _planes(a)
        red = torch.empty((_ntiles(n, c, h * w), c, 2), dtype=torch.float32, device=dy.device)
        check(lib.pcuda_upsample2_bwd_bnred(dy.data_ptr(), dsn, dsc, dx.data_ptr(), dx.stride(0), dx.stride(1), 0,
                                            a.data_ptr(), asn, asc, st.mean.data_ptr(), st.invstd.data_ptr(),
                                            red.data_ptr(), None, n, c, h, w, _stream()), "upsample2_bwd_bnred")
        return dx, (red, red.shape[0])
    check(lib.pcuda_upsample2_bwd(dy.data_ptr(), dsn, dsc, dx.data_ptr(), dx.stride(0), dx.stride(1), 0, n, c, h,
                                  w, _stream()), "upsample2_bwd")
    return (dx, None) if bnred is not None else dx


def bilinear_fwd(x, oh, ow):
    """[n,c,h,w] -> [n,c,oh,ow], align_corners=True (nn.UpsamplingBilinear2d)"""
    n, c, _, xsn, xsc = _planes(x)
    h, w = x.shape[2], x.shape[3]
    y = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    check(L.lib().pcuda_bilinear_fwd(x.data_ptr(), xsn, xsc, n, c, h, w, y.data_ptr(), oh, ow, _stream()), "bilinear_fwd")
    return y


def bilinear_bwd(dy, h, w):
    _req(dy)
    dy = dy.contiguous()
    n, c, oh, ow = dy.shape
    dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dy.device)
    check(L.lib().pcuda_bilinear_bwd(dy.data_ptr(), n, c, oh, ow, dx.data_ptr(), dx.stride(0), dx.stride(1), h, w,
                                     _stream()), "bilinear_bwd")
    return dx


def d1_forward_direct(op, n, h, w):
    """True where ``op.forward`` runs on the direct first-layer kernel (pcuda_conv2d_d1_forward_ok): no unfolded tensor"""
    g = op.geom(n, h, w)
    return bool(L.lib().pcuda_conv2d_d1_forward_ok(C.byref(g)))


def unfold_taps(x, k, stride, pad, dil=1):
    """[n,c,h,w] -> [n,c*k*k,oh,ow]: every tap of a k x k window as its own channel (zero outside the image)"""
    n, c, _, xsn, xsc = _planes(x)
    h, w = x.shape[2], x.shape[3]
    oh = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
    ow = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    u = torch.empty((n, c * k * k, oh, ow), dtype=torch.float32, device=x.device)
    check(L.lib().pcuda_unfold_taps(x.data_ptr(), xsn, xsc, n, c, h, w, k, stride, pad, dil, u.data_ptr(), oh, ow,
                                    _stream()), "unfold_taps")
    return u


def add_n(ts, out=None):
    ts = [t for t in ts if t is not None]
    for t in ts:
        _req(t)
        if not t.is_contiguous():
            raise ValueError("add_n needs contiguous tensors")
    if out is None:
        out = torch.empty_like(ts[0])
    p = [t.data_ptr() for t in ts] + [None] * (4 - len(ts))
    check(L.lib().pcuda_add4(p[0], p[1], p[2], p[3], out.data_ptr(), out.numel(), _stream()), "add4")
    return out


def mul(a, b):
    _req(a); _req(b)
    a, b = a.contiguous(), b.contiguous()
    y = torch.empty_like(a)
    check(L.lib().pcuda_mul(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), _stream()), "mul")
    return y


# ------------------------------------------------------------------------------------------
# losses / entropy
# ------------------------------------------------------------------------------------------
def _mode(m):
    return ACT_SIGMOID if m in (ACT_SIGMOID, "sigmoid") else ACT_SOFTMAX


def entropy_fwd(logits, mode="sigmoid", norm=1.0, want_prob=False):
    _req(logits)
    logits = logits.contiguous()
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    ent = torch.empty_like(logits)
    prob = torch.empty_like(logits) if want_prob else None
    check(L.lib().pcuda_entropy_fwd(logits.data_ptr(), _mode(mode), float(norm), ent.data_ptr(), _ptr(prob), n, c, hw,
                                    _stream()), "entropy_fwd")
    return ent, prob


def entropy_bwd(logits, mode, norm, dent=None, dprob=None, out=None, accumulate=False, dmean=None):
    """``dmean``: device scalar, gradient of the map's mean over batch and pixels (sum over channels)"""
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    if out is None:
        out = torch.empty_like(logits)
    check(L.lib().pcuda_entropy_bwd2(logits.data_ptr(), _mode(mode), float(norm),
                                     _ptr(None if dent is None else dent.contiguous()),
                                     _ptr(None if dprob is None else dprob.contiguous()),
                                     _ptr(None if dmean is None else dmean.contiguous()), out.data_ptr(),
                                     1 if accumulate else 0, n, c, hw, _stream()), "entropy_bwd")
    return out


def sum_all(x, scale=1.0):
    """scale * sum(x) as a 0-dim device tensor (fixed summation order)"""
    _req(x)
    x = x.contiguous()
    lib = L.lib()
    nb = lib.pcuda_sum_all_workspace_size()
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    check(lib.pcuda_sum_all(x.data_ptr(), x.numel(), float(scale), out.data_ptr(), ws.data_ptr(), nb, _stream()), "sum_all")
    return out


def seg_loss_fwd(logits, onehot, mode="sigmoid"):
    _req(logits)
    _req(onehot, torch.uint8)
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    lib = L.lib()
    nb = lib.pcuda_seg_loss_workspace_size(n, c, hw)
    ws = torch.empty(nb, dtype=torch.uint8, device=logits.device)
    out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
    check(lib.pcuda_seg_loss_fwd(logits.data_ptr(), onehot.data_ptr(), _mode(mode), n, c, hw, out2.data_ptr(),
                                 ws.data_ptr(), nb, _stream()), "seg_loss_fwd")
    return out2, ws


def seg_loss_bwd(logits, onehot, mode, ws, g_main=None, g_jac=None):
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    d = torch.empty_like(logits)
    check(L.lib().pcuda_seg_loss_bwd(logits.data_ptr(), onehot.data_ptr(), _mode(mode), n, c, hw, _ptr(g_main),
                                     _ptr(g_jac), d.data_ptr(), ws.data_ptr(), _stream()), "seg_loss_bwd")
    return d


def _probs_truth(what, probs, truth):
    """the operands of an overlap loss on given probabilities -> (probs, truth as the kernel reads it, n, c, hw)"""
    _req(probs)
    if truth.dtype not in (torch.float32, torch.uint8):
        truth = truth.float()      # the reference casts any dtype: ``true.type(probas.type())`` (loss.py:27)
    _req(truth, truth.dtype)
    if truth.shape != probs.shape:
        raise ValueError("%s: `true` %r and probabilities %r differ in shape" % (what, tuple(truth.shape), tuple(probs.shape)))
    n, c = probs.shape[:2]
    return probs.contiguous(), truth.contiguous(), n, c, probs.numel() // (n * c)


def _probs_grad(truth, shape):
    """-> (the gradient tensor of an overlap loss on given probabilities, whether the truth is uint8, n, c, hw)"""
    n, c = shape[:2]
    hw = 1
    for d in shape[2:]:
        hw *= d
    return torch.empty(shape, dtype=torch.float32, device=truth.device), 1 if truth.dtype == torch.uint8 else 0, n, c, hw


def jaccard_fwd(probs, truth, eps):
    """probs fp32 [n,c,...]; truth one-hot, fp32 or uint8, same shape -> (loss scalar, workspace, the truth tensor the kernel
    read)"""
    probs, truth, n, c, hw = _probs_truth("jaccard", probs, truth)
    lib = L.lib()
    nb = lib.pcuda_jaccard_workspace_size(c)
    ws = torch.empty(nb, dtype=torch.uint8, device=probs.device)
    loss = torch.empty((), dtype=torch.float32, device=probs.device)
    check(lib.pcuda_jaccard_fwd(probs.data_ptr(), truth.data_ptr(), 1 if truth.dtype == torch.uint8 else 0, n, c, hw,
                                float(eps), loss.data_ptr(), ws.data_ptr(), nb, _stream()), "jaccard_fwd")
    return loss, ws, truth


def jaccard_bwd(truth, shape, eps, ws, gout):
    dp, u8, n, c, hw = _probs_grad(truth, shape)
    check(L.lib().pcuda_jaccard_bwd(truth.data_ptr(), u8, n, c, hw, float(eps), _ptr(gout), dp.data_ptr(), ws.data_ptr(),
                                    _stream()), "jaccard_bwd")
    return dp


_OVERLAP = {"dice": L.OV_DICE_CLASS, "dice_sample": L.OV_DICE_SAMPLE, "class": L.OV_DICE_CLASS, "sample": L.OV_DICE_SAMPLE}


def _overlap(name):
    """'dice' / 'class' (per class) or 'dice_sample' / 'sample' (per sample) -> PCUDA_OV_*"""
    if name not in _OVERLAP:
        raise ValueError("Dice term %r: one of %s" % (name, ", ".join(sorted(_OVERLAP))))
    return _OVERLAP[name]


def seg_loss_ov_fwd(logits, onehot, mode="sigmoid", overlap="dice", eps=1e-7):
    """seg_loss_fwd with a Dice overlap term ('dice': per class, 'dice_sample': per sample) -> (out2 = [main, dice], workspace)"""
    _req(logits)
    _req(onehot, torch.uint8)
    ov = _overlap(overlap)
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    lib = L.lib()
    nb = lib.pcuda_seg_loss_ov_workspace_size(n, c, hw, ov)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=logits.device)
    out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
    check(lib.pcuda_seg_loss_ov_fwd(logits.data_ptr(), onehot.data_ptr(), _mode(mode), ov, float(eps), n, c, hw,
                                    out2.data_ptr(), ws.data_ptr(), nb, _stream()), "seg_loss_ov_fwd")
    return out2, ws


def seg_loss_ov_bwd(logits, onehot, mode, overlap, ws, g_main=None, g_ov=None):
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    d = torch.empty_like(logits)
    check(L.lib().pcuda_seg_loss_ov_bwd(logits.data_ptr(), onehot.data_ptr(), _mode(mode), _overlap(overlap), n, c, hw,
                                        _ptr(g_main), _ptr(g_ov), d.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "seg_loss_ov_bwd")
    return d


def dice_fwd(probs, truth, eps, reduce="class"):
    """probs fp32 [n,c,...]; truth one-hot, fp32 or uint8, same shape; reduce 'class' | 'sample' -> (loss scalar, workspace,
    the truth tensor the kernel read)"""
    red = _overlap(reduce)
    probs, truth, n, c, hw = _probs_truth("dice", probs, truth)
    lib = L.lib()
    nb = lib.pcuda_dice_workspace_size(n, c, hw, red)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=probs.device)
    loss = torch.empty((), dtype=torch.float32, device=probs.device)
    check(lib.pcuda_dice_fwd(probs.data_ptr(), truth.data_ptr(), 1 if truth.dtype == torch.uint8 else 0, n, c, hw, red,
                             float(eps), loss.data_ptr(), ws.data_ptr(), nb, _stream()), "dice_fwd")
    return loss, ws, truth


def dice_bwd(truth, shape, reduce, ws, gout):
    dp, u8, n, c, hw = _probs_grad(truth, shape)
    check(L.lib().pcuda_dice_bwd(truth.data_ptr(), u8, n, c, hw, _overlap(reduce), _ptr(gout), dp.data_ptr(), ws.data_ptr(),
                                 ws.numel(), _stream()), "dice_bwd")
    return dp


def dice_labels_fwd(logits, labels, eps=1e-6):
    """logits fp32 [n,c,...]; labels uint8 or int64 [n,...] -> (loss scalar, workspace, the labels the kernel read, the device
    counter (int64 scalar) of labels outside [0, c))"""
    _req(logits)
    if labels.dtype not in (torch.uint8, torch.int64):
        raise TypeError("dice_labels: uint8 or int64 labels, got %s" % labels.dtype)
    _req(labels, labels.dtype)
    logits, labels = logits.contiguous(), labels.contiguous()
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    if labels.numel() != n * hw:
        raise ValueError("dice_labels: labels %r do not match logits %r" % (tuple(labels.shape), tuple(logits.shape)))
    lib = L.lib()
    nb = lib.pcuda_dice_labels_workspace_size(n, c, hw)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    bad = torch.empty((), dtype=torch.int64, device=logits.device)
    check(lib.pcuda_dice_labels_fwd(logits.data_ptr(), labels.data_ptr(), 1 if labels.dtype == torch.int64 else 0, n, c, hw,
                                    float(eps), loss.data_ptr(), bad.data_ptr(), ws.data_ptr(), nb, _stream()),
          "dice_labels_fwd")
    return loss, ws, labels, bad


def dice_labels_bwd(logits, labels, ws, gout):
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    d = torch.empty_like(logits)
    check(L.lib().pcuda_dice_labels_bwd(logits.data_ptr(), labels.data_ptr(), 1 if labels.dtype == torch.int64 else 0, n, c,
                                        hw, _ptr(gout), d.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "dice_labels_bwd")
    return d


def bce_const_fwd(x, label, want_acc=False):
    _req(x)
    x = x.contiguous()
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    acc = torch.empty((), dtype=torch.float32, device=x.device) if want_acc else None
    check(L.lib().pcuda_bce_const_fwd(x.data_ptr(), x.numel(), float(label), loss.data_ptr(), _ptr(acc), _stream()),
          "bce_const_fwd")
    return loss, acc


def bce_const_bwd(x, label, gout, gscale=1.0):
    x = x.contiguous()
    dx = torch.empty_like(x)
    check(L.lib().pcuda_bce_const_bwd(x.data_ptr(), x.numel(), float(label), _ptr(gout), float(gscale), dx.data_ptr(),
                                      _stream()), "bce_const_bwd")
    return dx


def nn_loss_fwd(x, y):
    _req(x); _req(y)
    x, y = x.contiguous(), y.contiguous()
    b, npts = x.shape[0], x.shape[1]
    idx = torch.empty((2, b, npts), dtype=torch.int32, device=x.device)
    val = torch.empty(L.lib().pcuda_nn_loss_workspace_floats(b, npts), dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    check(L.lib().pcuda_nn_loss_fwd(x.data_ptr(), y.data_ptr(), b, npts, loss.data_ptr(), idx.data_ptr(),
                                    val.data_ptr(), _stream()), "nn_loss_fwd")
    return loss, idx, val


def nn_loss_bwd(x, y, idx, val, gout):
    x, y = x.contiguous(), y.contiguous()
    b, npts = x.shape[0], x.shape[1]
    dx = torch.empty_like(x)
    check(L.lib().pcuda_nn_loss_bwd(x.data_ptr(), y.data_ptr(), b, npts, idx.data_ptr(), val.data_ptr(), _ptr(gout),
                                    dx.data_ptr(), _stream()), "nn_loss_bwd")
    return dx


def dice_metric(logits, onehot):
    _req(logits); _req(onehot, torch.uint8)
    logits = logits.contiguous()
    n, c = logits.shape[:2]
    hw = logits.numel() // (n * c)
    ws = torch.empty(3 * c, dtype=torch.int64, device=logits.device)
    out = torch.empty((), dtype=torch.float32, device=logits.device)
    check(L.lib().pcuda_dice_metric(logits.data_ptr(), onehot.data_ptr(), n, c, hw, out.data_ptr(), ws.data_ptr(),
                                    ws.numel() * 8, _stream()), "dice_metric")
    return out


def assemble_batch(images_hwc, mask_labels, num_classes, crop=0):
    """[B,H,W,C] fp32 images (+ [B,H,W] int32 labels) -> ([B,C,h,w] fp32, [B,K,h,w] uint8 one-hot | None)."""
    _req(images_hwc)
    images_hwc = images_hwc.contiguous()
    b, h, w, c = images_hwc.shape
    oh, ow = (2 * (crop // 2), 2 * (crop // 2)) if crop else (h, w)
    out = torch.empty((b, c, oh, ow), dtype=torch.float32, device=images_hwc.device)
    onehot = None
    if mask_labels is not None:
        _req(mask_labels, torch.int32)
        mask_labels = mask_labels.contiguous()
        if tuple(mask_labels.shape) != (b, h, w):
            raise ValueError("assemble_batch: mask shape %r does not match the images" % (tuple(mask_labels.shape),))
        onehot = torch.empty((b, num_classes, oh, ow), dtype=torch.uint8, device=images_hwc.device)
    check(L.lib().pcuda_assemble_batch(images_hwc.data_ptr(), _ptr(mask_labels), b, h, w, c, int(crop), int(num_classes),
                                       out.data_ptr(), _ptr(onehot), _stream()), "assemble_batch")
    return out, onehot


def minmax(x):
    """fp32 tensor -> device tensor [2] = (min, max) over every element (no host read)."""
    _req(x)
    x = x.contiguous()
    nbytes = L.lib().pcuda_minmax_workspace_size()
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    check(L.lib().pcuda_minmax(x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "minmax")
    return out


AUG_NONE, AUG_MINMAX, AUG_DIV255 = 0, 1, 2


def _augment_assemble(what, dequant, images_hwc, mask_labels, inv_mats, order, cval, num_classes, crop, rescale, minmax,
                      want_images, want_onehot, want_full_mask, want_labels, want_u8):
    """the body of ``augment_assemble`` and ``augment_assemble_dequant``: checks, output tensors, one launch"""
    if images_hwc.dtype not in ((torch.uint8,) if dequant else (torch.float32, torch.uint8)):
        raise TypeError("%s: %s images" % (what, "uint8" if dequant else "fp32 or uint8"))
    _req(images_hwc, images_hwc.dtype)
    _req(inv_mats, torch.float64); _req(order, torch.int32); _req(cval, torch.int32)
    images_hwc = images_hwc.contiguous()
    b, h, w, c = images_hwc.shape
    if tuple(inv_mats.shape) != (b, 2, 3) or tuple(order.shape) != (b,) or tuple(cval.shape) != (b,):
        raise ValueError("%s: per-sample parameters do not match the batch of %d" % (what, b))
    dev = images_hwc.device
    oh, ow = (2 * (crop // 2), 2 * (crop // 2)) if crop else (h, w)
    if mask_labels is not None:
        _req(mask_labels, torch.int32)
        mask_labels = mask_labels.contiguous()
        if tuple(mask_labels.shape) != (b, h, w):
            raise ValueError("%s: mask shape %r does not match the images" % (what, tuple(mask_labels.shape)))
    else:
        want_onehot = want_full_mask = want_labels = False
    out = {}
    if want_images:
        out["images"] = torch.empty((b, c, oh, ow), dtype=torch.float32, device=dev)
    if want_onehot:
        out["onehot"] = torch.empty((b, num_classes, oh, ow), dtype=torch.uint8, device=dev)
    if want_full_mask:
        out["full_mask"] = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    if want_labels:
        out["labels"] = torch.empty((b, h, w), dtype=torch.int32, device=dev)
    if want_u8:
        out["images_u8"] = torch.empty((b, h, w, c), dtype=torch.uint8, device=dev)
    if minmax is not None:
        _req(minmax)
    head = (images_hwc.data_ptr(),) if dequant else (images_hwc.data_ptr(), int(images_hwc.dtype == torch.uint8))
    mid = (_ptr(minmax),) if dequant else (int(rescale), _ptr(minmax))
    fn = L.lib().pcuda_augment_assemble_dequant if dequant else L.lib().pcuda_augment_assemble
    check(fn(*head, _ptr(mask_labels), b, h, w, c, int(crop), int(num_classes), inv_mats.contiguous().data_ptr(),
             order.contiguous().data_ptr(), cval.contiguous().data_ptr(), *mid, _ptr(out.get("images")), _ptr(out.get("onehot")),
             _ptr(out.get("full_mask")), _ptr(out.get("labels")), _ptr(out.get("images_u8")), _stream()), what)
    return out


def augment_assemble(images_hwc, mask_labels, inv_mats, order, cval, num_classes=5, crop=0, rescale=AUG_NONE, minmax=None,
                     want_images=True, want_onehot=True, want_full_mask=False, want_labels=False, want_u8=False):
    """Flips + affine + rescale + batch assembly in one launch (``pcuda_augment_assemble``).  images ``[B,H,W,C]`` fp32 or
    uint8, labels ``[B,H,W]`` int32 or None, ``inv_mats`` float64 ``[B,2,3]``, ``order`` / ``cval`` int32 ``[B]``, all on
    the device -> dict with the outputs asked for: ``images`` fp32 ``[B,C,h,w]``, ``onehot`` uint8 ``[B,K,h,w]`` (cropped),
    ``full_mask`` uint8 ``[B,H,W]``, ``labels`` int32 ``[B,H,W]``, ``images_u8`` uint8 ``[B,H,W,C]`` (full size)."""
    return _augment_assemble("augment_assemble", False, images_hwc, mask_labels, inv_mats, order, cval, num_classes, crop, rescale,
                             minmax, want_images, want_onehot, want_full_mask, want_labels, want_u8)


def quantize_u8(x, minmax, out=None):
    """fp32 tensor and the device ``(min, max)`` pair of ``minmax(x)`` -> uint8 tensor of ``x``'s shape
    (``pcuda_quantize_u8``): ``trunc(((x - min) * 255) / (max - min))`` in fp32, clamped to [0, 255]; ``max == min`` and NaN
    elements give 0.  No host read.  ``x`` and ``out`` may be any views with contiguous elements (a misaligned one takes the
    kernel's one-element path)."""
    _req(x); _req(minmax)
    if minmax.numel() != 2 or not minmax.is_contiguous():
        raise ValueError("quantize_u8: minmax is the contiguous (min, max) pair of kernels.minmax")
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    elif not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or out.shape != x.shape or not out.is_contiguous():
        raise ValueError("quantize_u8: out must be a contiguous uint8 tensor of shape %s" % list(x.shape))
    check(L.lib().pcuda_quantize_u8(x.data_ptr(), x.numel(), minmax.data_ptr(), out.data_ptr(), _stream()), "quantize_u8")
    return out


def augment_assemble_dequant(images_u8, mask_labels, inv_mats, order, cval, minmax, num_classes=5, crop=0, want_images=True,
                             want_onehot=True, want_full_mask=False, want_labels=False, want_u8=False):
    """``augment_assemble`` on uint8 images that ``quantize_u8`` made, back to fp32 behind the warp
    (``pcuda_augment_assemble_dequant``): ``images = min + float(q') * (max - min) / 255``; ``minmax`` is the device pair the
    images were quantised with.  Outputs as ``augment_assemble``."""
    if minmax is None:
        raise TypeError("augment_assemble_dequant: minmax is required (the pair the images were quantised with)")
    if minmax.numel() != 2 or not minmax.is_contiguous():
        raise ValueError("augment_assemble_dequant: minmax is the contiguous (min, max) pair of kernels.minmax")
    return _augment_assemble("augment_assemble_dequant", True, images_u8, mask_labels, inv_mats, order, cval, num_classes, crop,
                             AUG_MINMAX, minmax, want_images, want_onehot, want_full_mask, want_labels, want_u8)


def photometric(images_u8, opcode, iarg, farg, seed, out=None):
    """A per-sample photometric program over uint8 ``[B,H,W,C]`` images (``pcuda_photometric``): ``opcode`` int32 ``[B,S]``,
    ``iarg`` int32 ``[B,S,4]``, ``farg`` float64 ``[B,S,16]``, ``seed`` int64 ``[B,S]`` (the bits of the 64-bit Philox key), all on
    the device, ``S`` = 0..8 -> a new uint8 tensor (the input is never written)."""
    images_u8, (b, h, w, c) = _images("photometric", images_u8)
    slots, arrays = _program("photometric", b, opcode, seed, iarg=(iarg, torch.int32, 4), farg=(farg, torch.float64, 16))
    out = _out("photometric", out, images_u8)
    nbytes = L.lib().pcuda_photometric_workspace_size(b, h, w, c) if slots > 1 else 0
    ws = _workspace(nbytes, images_u8.device)
    check(L.lib().pcuda_photometric(images_u8.data_ptr(), out.data_ptr(), b, h, w, c, slots, *(t.data_ptr() for t in arrays),
                                    _ptr(ws), nbytes, _stream()), "photometric")
    return out


def geometric(images_u8, labels, opcode, iarg, farg, seed, out=None, labels_out=None, cubic=False):
    """A per-sample geometric program over uint8 ``[B,H,W,C]`` images and optional int32 ``[B,H,W]`` labels
    (``pcuda_geometric``): ``opcode`` int32 ``[B,S]``, ``iarg`` int32 ``[B,S,4]``, ``farg`` float64 ``[B,S,32]``, ``seed`` int64
    ``[B,S]`` (the bits of the 64-bit Philox key), all on the device, ``S`` = 0..8 -> ``(images, labels or None)``, new tensors
    (the inputs are never written).  ``cubic=True`` goes through ``pcuda_geometric_cubic`` (the same arguments and workspace):
    order 3 samples cubically there; without it order 3 samples as order 1."""
    images_u8, (b, h, w, c) = _images("geometric", images_u8)
    slots, arrays = _program("geometric", b, opcode, seed, iarg=(iarg, torch.int32, 4), farg=(farg, torch.float64, 32))
    labels, labels_out = _labels_io("geometric", labels, labels_out, (b, h, w))
    out = _out("geometric", out, images_u8)
    nbytes = L.lib().pcuda_geometric_workspace_size(b, h, w, c, int(labels is not None)) if slots > 1 else 0
    ws = _workspace(nbytes, images_u8.device)
    run_fn = L.lib().pcuda_geometric_cubic if cubic else L.lib().pcuda_geometric
    check(run_fn(images_u8.data_ptr(), out.data_ptr(), _ptr(labels), _ptr(labels_out), b, h, w, c, slots,
                 *(t.data_ptr() for t in arrays), _ptr(ws), nbytes, _stream()), "geometric_cubic" if cubic else "geometric")
    return out, labels_out


def _stylize(name, images_u8, opcode, iarg, farg, table, seed, out):
    images_u8, (b, h, w, c) = _images("stylize", images_u8)
    slots, arrays = _program("stylize", b, opcode, seed, iarg=(iarg, torch.int32, 12), farg=(farg, torch.float64, 16),
                             table=(table, torch.float64, 768))
    out = _out("stylize", out, images_u8)
    size_fn, run_fn = getattr(L.lib(), "pcuda_%s_workspace_size" % name), getattr(L.lib(), "pcuda_" + name)
    nbytes = size_fn(b, h, w, c) if slots > 0 else 0
    ws = _workspace(nbytes, images_u8.device)
    check(run_fn(images_u8.data_ptr(), out.data_ptr(), b, h, w, c, slots, *(t.data_ptr() for t in arrays), _ptr(ws), nbytes,
                 _stream()), name)
    return out


def stylize(images_u8, opcode, iarg, farg, table, seed, out=None, connect=False):
    """A per-sample stylize program over uint8 ``[B,H,W,C]`` images (``pcuda_stylize``): ``opcode`` int32 ``[B,S]``, ``iarg`` int32
    ``[B,S,12]``, ``farg`` float64 ``[B,S,16]``, ``table`` float64 ``[B,S,768]``, ``seed`` int64 ``[B,S]`` (the bits of the 64-bit
    Philox key), all on the device, ``S`` = 0..8 -> a new uint8 tensor (the input is never written).  ``connect=True`` goes
    through ``pcuda_stylize_connect`` (and its larger workspace): SUPERPIXELS slots with ``iarg[5] > 0`` get the connectivity
    pass; without it ``iarg[5]`` is never read.  Neither reads ``iarg[6]`` (``stylize_scaled`` does)."""
    return _stylize("stylize_connect" if connect else "stylize", images_u8, opcode, iarg, farg, table, seed, out)


def stylize_scaled(images_u8, opcode, iarg, farg, table, seed, out=None):
    """``stylize`` through ``pcuda_stylize_scaled`` (f9c; a larger workspace again), which serves connected and unconnected slots
    alike: ``iarg[5]`` is honoured as with ``connect=True``, and SUPERPIXELS slots whose ``iarg[6]`` = max_size is at least 1 and
    below ``max(H, W)`` run at their working size.  With ``iarg[6] = 0`` everywhere it is ``stylize(.., connect=True)`` bit for
    bit."""
    return _stylize("stylize_scaled", images_u8, opcode, iarg, farg, table, seed, out)


def crop_pad(images_u8, labels, opcode, iarg, out=None, labels_out=None):
    """CropAndPad with numpy's pad modes over uint8 ``[B,H,W,C]`` images and optional int32 ``[B,H,W]`` labels (``pcuda_crop_pad``):
    ``opcode`` int32 ``[B]`` (0 copy, 1 crop-and-pad), ``iarg`` int32 ``[B,6]`` = (top, right, bottom, left, mode, cval), both on the
    device -> ``(images, labels or None)``, new tensors unless ``out`` / ``labels_out`` are given (the inputs are never written)."""
    images_u8, (b, h, w, c) = _images("crop_pad", images_u8)
    _req(opcode, torch.int32); _req(iarg, torch.int32)
    if tuple(opcode.shape) != (b,) or tuple(iarg.shape) != (b, 6):
        raise ValueError("crop_pad: the program's arrays do not match the batch of %d" % b)
    labels, labels_out = _labels_io("crop_pad", labels, labels_out, (b, h, w))
    out = _out("crop_pad", out, images_u8)
    nbytes = L.lib().pcuda_crop_pad_workspace_size(b, h, w, c)
    ws = _workspace(nbytes, images_u8.device)
    check(L.lib().pcuda_crop_pad(images_u8.data_ptr(), out.data_ptr(), _ptr(labels), _ptr(labels_out), b, h, w, c,
                                 opcode.contiguous().data_ptr(), iarg.contiguous().data_ptr(), _ptr(ws), nbytes, _stream()),
          "crop_pad")
    return out, labels_out


def match_hist(images, tvalues, tquantiles, tlen, out=None):
    """Histogram matching of ``[B,H,W,C]`` fp32 or uint8 images against a template's tables (``pcuda_match_hist``): ``tvalues`` and
    ``tquantiles`` float64 ``[C,T]`` (per channel the template's sorted distinct values and ``cumsum(counts) / M``), ``tlen`` int32
    ``[C]`` valid entries, all on the device -> a new tensor of the images' dtype (the input is never written)."""
    images, (b, h, w, c) = _images("match_hist", images, (torch.float32, torch.uint8))
    _req(tvalues, torch.float64); _req(tquantiles, torch.float64); _req(tlen, torch.int32)
    if tvalues.dim() != 2 or tvalues.shape[0] != c or tvalues.shape[1] < 1 or tquantiles.shape != tvalues.shape or \
            tuple(tlen.shape) != (c,):
        raise ValueError("match_hist: the tables do not match the %d channels of the images" % c)
    out = _out("match_hist", out, images)
    is_u8 = int(images.dtype == torch.uint8)
    nbytes = L.lib().pcuda_match_hist_workspace_size(b, h, w, c, is_u8)
    ws = _workspace(nbytes, images.device)
    check(L.lib().pcuda_match_hist(images.data_ptr(), out.data_ptr(), is_u8, b, h, w, c, tvalues.contiguous().data_ptr(),
                                   tquantiles.contiguous().data_ptr(), tlen.contiguous().data_ptr(), int(tvalues.shape[1]),
                                   _ptr(ws), nbytes, _stream()), "match_hist")
    return out


def hist_bank_storage(r, rh, rw, c, is_u8, device):
    """``(bank, workspace or None, flag)`` device tensors sized for ``hist_bank_build`` of ``[r,rh,rw,c]`` references"""
    lib = L.lib()
    bank = torch.empty(lib.pcuda_hist_bank_size(r, rh, rw, c, int(is_u8)), dtype=torch.uint8, device=device)
    ws = _workspace(lib.pcuda_hist_bank_workspace_size(r, rh, rw, c, int(is_u8)), device)
    return bank, ws, torch.zeros(1, dtype=torch.int32, device=device)


def hist_bank_build(references, bank=None, workspace=None, flag=None):
    """The bank of ``[R,H,W,C]`` fp32 or uint8 reference images (``pcuda_hist_bank_build``): fp32 -> the sorted keys of every
    plane, uint8 -> 256 counts per plane.  ``bank`` / ``workspace`` / ``flag`` (``hist_bank_storage``) are filled in place
    when given, so a rebuild allocates nothing; ``flag`` is 1 afterwards when a reference value is not finite.  Returns
    ``(bank, workspace, flag)``; the references are never written."""
    if references.dtype not in (torch.float32, torch.uint8):
        raise TypeError("hist_bank_build: fp32 or uint8 references, got %s" % (references.dtype,))
    _req(references, references.dtype)
    if references.dim() != 4 or not references.is_contiguous():
        raise TypeError("hist_bank_build: contiguous [R,H,W,C] references")
    r, rh, rw, c = references.shape
    is_u8 = int(references.dtype == torch.uint8)
    if bank is None:
        bank, workspace, flag = hist_bank_storage(r, rh, rw, c, is_u8, references.device)
    _req(bank, torch.uint8); _req(flag, torch.int32)
    nbytes = 0 if workspace is None else workspace.numel()
    check(L.lib().pcuda_hist_bank_build(references.data_ptr(), is_u8, r, rh, rw, c, bank.data_ptr(), bank.numel(), flag.data_ptr(),
                                        _ptr(workspace), nbytes, _stream()), "hist_bank_build")
    return bank, workspace, flag


def match_hist_bank(images, bank, ref_shape, ref_index, out=None):
    """Histogram matching of ``[B,H,W,C]`` fp32 or uint8 images against a bank (``pcuda_match_hist_bank``): ``bank`` as
    ``hist_bank_build`` left it for references of ``ref_shape = (R, RH, RW, C)`` and the images' dtype, ``ref_index`` int32
    ``[B]`` on the device (sample i takes reference ``ref_index[i]``, clamped into ``[0, R)``) -> a new tensor of the images'
    dtype (the input is never written)."""
    images, (b, h, w, c) = _images("match_hist_bank", images, (torch.float32, torch.uint8))
    r, rh, rw, rc = (int(v) for v in ref_shape)
    is_u8 = int(images.dtype == torch.uint8)
    _req(bank, torch.uint8); _req(ref_index, torch.int32)
    if rc != c:
        raise ValueError("match_hist_bank: the bank has %d channels, the images %d" % (rc, c))
    if tuple(ref_index.shape) != (b,) or not ref_index.is_contiguous():
        raise ValueError("match_hist_bank: ref_index must be a contiguous int32 [%d] tensor" % b)
    if bank.numel() < L.lib().pcuda_hist_bank_size(r, rh, rw, c, is_u8):
        raise ValueError("match_hist_bank: the bank is smaller than %r references of the images' dtype need" % (tuple(ref_shape),))
    out = _out("match_hist_bank", out, images)
    nbytes = L.lib().pcuda_match_hist_bank_workspace_size(b, h, w, c, is_u8)
    ws = _workspace(nbytes, images.device)
    check(L.lib().pcuda_match_hist_bank(images.data_ptr(), out.data_ptr(), is_u8, b, h, w, c, bank.data_ptr(), r, rh, rw,
                                        ref_index.data_ptr(), _ptr(ws), nbytes, _stream()), "match_hist_bank")
    return out


def fourier_bank_storage(r, h, w, c, radius, device):
    """``(bank, workspace)`` device tensors sized for ``fourier_bank_build`` of ``[r,h,w,c]`` references at ``radius``"""
    lib = L.lib()
    nbytes = lib.pcuda_fourier_bank_size(r, c, radius)
    if nbytes == 0 or lib.pcuda_fourier_bank_workspace_size(r, h, w, c, radius) == 0:
        raise ValueError("fourier_bank_build: unsupported [%d,%d,%d,%d] references at radius %d (1..4 channels, radius 0..32, "
                         "2 radius + 1 <= min(H, W), sides up to 4096)" % (r, h, w, c, radius))
    return (torch.empty(nbytes, dtype=torch.uint8, device=device),
            _workspace(lib.pcuda_fourier_bank_workspace_size(r, h, w, c, radius), device))


def fourier_bank_build(references, radius, bank=None, workspace=None):
    """The amplitude bank of ``[R,H,W,C]`` fp32 or uint8 target images (``pcuda_fourier_bank_build``): per plane the float64
    ``|T[ky, kx]|`` of the low-frequency block, ``ky = -radius..radius``, ``kx = 0..radius``.  ``bank`` / ``workspace``
    (``fourier_bank_storage``) are filled in place when given, so a rebuild allocates nothing.  Returns ``(bank, workspace)``;
    the references are never written."""
    if references.dtype not in (torch.float32, torch.uint8):
        raise TypeError("fourier_bank_build: fp32 or uint8 references, got %s" % (references.dtype,))
    _req(references, references.dtype)
    if references.dim() != 4 or not references.is_contiguous():
        raise TypeError("fourier_bank_build: contiguous [R,H,W,C] references")
    r, h, w, c = references.shape
    radius = int(radius)
    if bank is None:
        bank, workspace = fourier_bank_storage(r, h, w, c, radius, references.device)
    _req(bank, torch.uint8)
    nbytes = 0 if workspace is None else workspace.numel()
    check(L.lib().pcuda_fourier_bank_build(references.data_ptr(), int(references.dtype == torch.uint8), r, h, w, c, radius,
                                           bank.data_ptr(), bank.numel(), _ptr(workspace), nbytes, _stream()), "fourier_bank_build")
    return bank, workspace


def fourier_adapt(images, bank, ref_count, radius, ref_index, sample_radius=None, clip=None, out=None):
    """Fourier domain adaptation of ``[B,H,W,C]`` fp32 or uint8 images against a bank (``pcuda_fourier_adapt``): ``bank`` as
    ``fourier_bank_build`` left it for ``ref_count`` references of the images' ``H, W, C`` at ``radius``; ``ref_index`` int32
    ``[B]`` on the device (sample i takes reference ``ref_index[i]``, clamped below ``ref_count``; a negative entry passes the
    sample through), ``sample_radius`` int32 ``[B]`` on the device or ``None``; ``clip = (lo, hi)`` for fp32 images -> a new
    tensor of the images' dtype unless ``out`` is given (the input is never written)."""
    images, (b, h, w, c) = _images("fourier_adapt", images, (torch.float32, torch.uint8))
    r, radius = int(ref_count), int(radius)
    _req(bank, torch.uint8); _req(ref_index, torch.int32)
    if tuple(ref_index.shape) != (b,) or not ref_index.is_contiguous():
        raise ValueError("fourier_adapt: ref_index must be a contiguous int32 [%d] tensor" % b)
    if sample_radius is not None:
        _req(sample_radius, torch.int32)
        if tuple(sample_radius.shape) != (b,) or not sample_radius.is_contiguous():
            raise ValueError("fourier_adapt: sample_radius must be a contiguous int32 [%d] tensor" % b)
    if r < 1 or bank.numel() < L.lib().pcuda_fourier_bank_size(r, c, radius):
        raise ValueError("fourier_adapt: the bank is smaller than %d references of %d channels at radius %d need" % (r, c, radius))
    lo = hi = 0.0
    if clip is not None:
        if images.dtype != torch.float32:
            raise TypeError("fourier_adapt: clip goes with fp32 images (uint8 images are clipped to 0..255)")
        lo, hi = float(clip[0]), float(clip[1])
        if not lo <= hi:
            raise ValueError("fourier_adapt: clip = (lo, hi) with lo <= hi, got %r" % (clip,))
    out = _out("fourier_adapt", out, images)
    nbytes = L.lib().pcuda_fourier_adapt_workspace_size(b, h, w, c, radius)
    ws = _workspace(nbytes, images.device)
    check(L.lib().pcuda_fourier_adapt(images.data_ptr(), out.data_ptr(), int(images.dtype == torch.uint8), b, h, w, c,
                                      bank.data_ptr(), r, radius, ref_index.data_ptr(), _ptr(sample_radius), int(clip is not None),
                                      lo, hi, _ptr(ws), nbytes, _stream()), "fourier_adapt")
    return out


def clahe(images_u8, clip_limit=2.0, tiles_x=4, tiles_y=4, to_float=False, out=None):
    """CLAHE of uint8 ``[N,H,W]`` slices (``pcuda_clahe``: the convention of include/pcuda_hip.h, written after OpenCV's
    ``createCLAHE(clip_limit, (tiles_x, tiles_y)).apply``) -> a new uint8 ``[N,H,W]`` tensor, or fp32 ``[N,3,H,W]`` holding
    ``u8 / 255`` in all three channels when ``to_float`` (the input is never written)."""
    images_u8, (n, h, w) = _images("clahe", images_u8, dim=3)
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=images_u8.device) if to_float else torch.empty_like(images_u8)
    else:
        _req(out, torch.float32 if to_float else torch.uint8)
        if tuple(out.shape) != ((n, 3, h, w) if to_float else (n, h, w)) or not out.is_contiguous():
            raise ValueError("clahe: out does not match the result's shape")
    nbytes = L.lib().pcuda_clahe_workspace_size(n, int(tiles_x), int(tiles_y))
    ws = _workspace(nbytes, images_u8.device)
    check(L.lib().pcuda_clahe(images_u8.data_ptr(), out.data_ptr(), n, h, w, float(clip_limit), int(tiles_x), int(tiles_y),
                              int(bool(to_float)), _ptr(ws), nbytes, _stream()), "clahe")
    return out


_PRE_DTYPES = {torch.float32: 0, torch.int16: 1, torch.uint8: 2}      # PCUDA_PRE_F32 / _I16 / _U8 (3: _U8_RAW)


def rescale_resize_crop_u8(volume, resize_h=None, resize_w=None, crop=0, out=None, raw=False):
    """A fp32, int16 or uint8 ``[N,H,W]`` volume -> uint8 (``pcuda_rescale_resize_crop_u8``): its own minimum / maximum (reduced on
    the device) stretched to 0..255 in float64 and truncated, a nearest-neighbour resize to ``(resize_h, resize_w)`` (None: the
    source size) and the centre crop of ``crop`` (0: none; else ``2 * (crop // 2)`` rows and columns) in one pass over the
    output -> a new tensor (the input is never written).  ``raw`` (uint8 volumes only): the values are kept as they are, no
    rescale (``PCUDA_PRE_U8_RAW``)."""
    if raw and volume.dtype != torch.uint8:
        raise TypeError("rescale_resize_crop_u8: raw takes a uint8 volume, got %s" % (volume.dtype,))
    if volume.dtype not in _PRE_DTYPES:
        raise TypeError("rescale_resize_crop_u8: a fp32, int16 or uint8 volume, got %s" % (volume.dtype,))
    _req(volume, volume.dtype)
    if volume.dim() != 3:
        raise TypeError("rescale_resize_crop_u8: an [N,H,W] volume")
    volume = volume.contiguous()
    n, sh, sw = volume.shape
    resize_h = sh if resize_h is None else int(resize_h)
    resize_w = sw if resize_w is None else int(resize_w)
    crop = int(crop)
    if crop < 0 or (crop > 0 and (crop // 2 < 1 or resize_h // 2 - crop // 2 < 0 or resize_w // 2 - crop // 2 < 0)):
        raise ValueError("rescale_resize_crop_u8: the crop window of %d leaves the %dx%d slice" % (crop, resize_h, resize_w))
    oh, ow = (2 * (crop // 2),) * 2 if crop > 0 else (resize_h, resize_w)
    if out is None:
        out = torch.empty((n, oh, ow), dtype=torch.uint8, device=volume.device)
    else:
        _req(out, torch.uint8)
        if tuple(out.shape) != (n, oh, ow) or not out.is_contiguous():
            raise ValueError("rescale_resize_crop_u8: out does not match the result's shape")
    nbytes = L.lib().pcuda_rescale_resize_crop_u8_workspace_size()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=volume.device)
    check(L.lib().pcuda_rescale_resize_crop_u8(volume.data_ptr(), 3 if raw else _PRE_DTYPES[volume.dtype], n, sh, sw, resize_h, resize_w, crop,
                                               out.data_ptr(), _ptr(ws), nbytes, _stream()), "rescale_resize_crop_u8")
    return out


def _zoom_geometry(what, volume, zoomed_hw, crop, dtypes=_PRE_DTYPES):
    """the shared host checks of the zoom wrappers -> (contiguous volume, n, sh, sw, zh, zw, crop, oh, ow)"""
    if volume.dtype not in dtypes:
        raise TypeError("%s: a %s volume, got %s" % (what, " / ".join(str(d).replace("torch.", "") for d in dtypes), volume.dtype))
    _req(volume, volume.dtype)
    if volume.dim() != 3:
        raise TypeError("%s: an [N,H,W] volume" % what)
    volume = volume.contiguous()
    n, sh, sw = volume.shape
    zh, zw = int(zoomed_hw[0]), int(zoomed_hw[1])
    crop = int(crop)
    if zh < 1 or zw < 1:
        raise ValueError("%s: a zoomed slice of at least 1x1, got %dx%d" % (what, zh, zw))
    if crop < 0 or (crop > 0 and (crop // 2 < 1 or zh // 2 - crop // 2 < 0 or zw // 2 - crop // 2 < 0)):
        raise ValueError("%s: the crop window of %d leaves the %dx%d slice" % (what, crop, zh, zw))
    oh, ow = (2 * (crop // 2),) * 2 if crop > 0 else (zh, zw)
    return volume, n, sh, sw, zh, zw, crop, oh, ow


def _zoom_out(what, out, shape, dtype, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _req(out, dtype)
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError("%s: out does not match the result's shape" % what)
    return out


def zoom_linear_crop(volume, zoomed_hw, crop=0, out=None):
    """``scipy.ndimage.zoom(volume, [1, zh / H, zw / W], order=1)`` of a fp32, int16 or uint8 ``[N,H,W]`` volume and the centre crop
    of ``crop`` (0: none; else ``2 * (crop // 2)`` rows and columns), only the crop window computed (``pcuda_zoom_linear_crop``)
    -> a new tensor of the volume's dtype (the input is never written)."""
    volume, n, sh, sw, zh, zw, crop, oh, ow = _zoom_geometry("zoom_linear_crop", volume, zoomed_hw, crop)
    out = _zoom_out("zoom_linear_crop", out, (n, oh, ow), volume.dtype, volume.device)
    nbytes = L.lib().pcuda_zoom_linear_crop_workspace_size(zh, zw, crop)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=volume.device)
    check(L.lib().pcuda_zoom_linear_crop(volume.data_ptr(), _PRE_DTYPES[volume.dtype], n, sh, sw, zh, zw, crop, out.data_ptr(),
                                         _ptr(ws), nbytes, _stream()), "zoom_linear_crop")
    return out


def zoom_standardize(volume, zoomed_hw, crop=0, channels=1, out=None, stats=None):
    """The image chain of the reference's ``.npy`` preparation in one call (``pcuda_zoom_standardize``): zoom, crop, the volume's
    mean and standard deviation over the cropped zoomed values (on the device), ``(x - mean) / std`` in float64 -> fp32
    ``[N,oh,ow]`` (``channels=1``) or ``[N,3,oh,ow]``.  -> ``(out, stats)``; ``stats``: float64 ``[2]`` on the device, mean and std."""
    volume, n, sh, sw, zh, zw, crop, oh, ow = _zoom_geometry("zoom_standardize", volume, zoomed_hw, crop)
    if channels not in (1, 3):
        raise ValueError("zoom_standardize: channels is 1 or 3, got %r" % (channels,))
    out = _zoom_out("zoom_standardize", out, (n, oh, ow) if channels == 1 else (n, 3, oh, ow), torch.float32, volume.device)
    stats = _zoom_out("zoom_standardize", stats, (2,), torch.float64, volume.device)
    nbytes = L.lib().pcuda_zoom_standardize_workspace_size(_PRE_DTYPES[volume.dtype], n, zh, zw, crop)
    ws = _workspace(nbytes, volume.device)
    check(L.lib().pcuda_zoom_standardize(volume.data_ptr(), _PRE_DTYPES[volume.dtype], n, sh, sw, zh, zw, crop, int(channels),
                                         out.data_ptr(), stats.data_ptr(), _ptr(ws), nbytes, _stream()), "zoom_standardize")
    return out, stats


def zoom_labels(labels, zoomed_hw, num_classes=4, remap=(), crop=0, out=None):
    """The label chain of the reference's ``.npy`` preparation fused (``pcuda_zoom_labels``): int16 or uint8 raw codes ``[N,H,W]``,
    the ``(from, to)`` pairs of ``remap`` applied in order, then ``argmax(zoom(onehot, order=1))`` without the one-hot tensor, and the
    crop -> ``(uint8 [N,oh,ow], counter)``; ``counter``: int64 ``[1]`` on the device, the number of input values that are no class."""
    labels, n, sh, sw, zh, zw, crop, oh, ow = _zoom_geometry("zoom_labels", labels, zoomed_hw, crop,
                                                             {torch.int16: 1, torch.uint8: 2})
    pairs = [(int(a), int(b)) for a, b in remap]
    if not 2 <= int(num_classes) <= 8:
        raise ValueError("zoom_labels: 2..8 classes, got %r" % (num_classes,))
    if len(pairs) > 8:
        raise ValueError("zoom_labels: a remap table of at most 8 (from, to) pairs, got %d" % len(pairs))
    out = _zoom_out("zoom_labels", out, (n, oh, ow), torch.uint8, labels.device)
    nbytes = L.lib().pcuda_zoom_labels_workspace_size(zh, zw, crop)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=labels.device)
    table = (C.c_int * max(2 * len(pairs), 1))(*[v for p in pairs for v in p])
    check(L.lib().pcuda_zoom_labels(labels.data_ptr(), _PRE_DTYPES[labels.dtype], n, sh, sw, zh, zw, crop, int(num_classes),
                                    C.cast(table, C.c_void_p), len(pairs), out.data_ptr(), _ptr(ws), nbytes, _stream()), "zoom_labels")
    return out, ws[:8].view(torch.int64)


_VOL_DTYPES = {torch.float32: 0, torch.int16: 1, torch.uint8: 2, torch.float64: 4, torch.int32: 5}    # PCUDA_VOL_*
_VOL_NAMES = {torch.float32: "float32", torch.int16: "int16", torch.uint8: "uint8", torch.float64: "float64", torch.int32: "int32"}


def _volume_view(what, view, dtypes):
    """the host checks of the volume wrappers: a 3-D device view [Z,R,C] of any stride -> (Z, R, C, sz, sr, sc)"""
    if not torch.is_tensor(view) or view.dtype not in dtypes:
        raise TypeError("%s: a %s volume, got %s" % (what, " / ".join(_VOL_NAMES[d] for d in dtypes), getattr(view, "dtype", type(view))))
    if view.dim() != 3:
        raise ValueError("%s: a [Z,R,C] view, got %d dimensions" % (what, view.dim()))
    _req(view, view.dtype)
    (z, r, c), (sz, sr, sc) = view.shape, view.stride()
    if z * r * c and any(n > 1 and s <= 0 for n, s in ((z, sz), (r, sr), (c, sc))):
        raise ValueError("%s: a positive stride on every axis longer than 1 (an expanded view?), got strides %r" % (what, (sz, sr, sc)))
    if max(z, r, c) >= 2 ** 31:
        raise ValueError("%s: sides below 2^31, got %r" % (what, (z, r, c)))
    return z, r, c, sz, sr, sc


def volume_slices(view, flip_r=False, flip_c=False, window=3, out=None):
    """A fp32, float64, int16 or uint8 device view ``[Z,R,C]`` of ANY stride (``pcuda_volume_slices``) -> contiguous fp32
    ``[Z,window,R,C]``: rows and columns mirrored where ``flip_r`` / ``flip_c``; ``window=3``: channel ``k`` of sample ``i`` is slice
    ``(i + k - 1) mod Z`` (the reference's 2.5-D stack), ``window=1``: the slices themselves.  The input is never written."""
    z, r, c, sz, sr, sc = _volume_view("volume_slices", view, (torch.float32, torch.float64, torch.int16, torch.uint8))
    if window not in (1, 3):
        raise ValueError("volume_slices: window is 1 or 3, got %r" % (window,))
    out = _zoom_out("volume_slices", out, (z, window, r, c), torch.float32, view.device)
    check(L.lib().pcuda_volume_slices(view.data_ptr(), _VOL_DTYPES[view.dtype], 0, sz, sr, sc, z, r, c, int(bool(flip_r)),
                                      int(bool(flip_c)), window, out.data_ptr(), _stream()), "volume_slices")
    return out


def volume_labels(view, flip_r=False, flip_c=False, num_classes=5, remap=(), onehot=False, raw=False):
    """A uint8, int16, int32, fp32 or float64 device view ``[Z,R,C]`` of any stride (``pcuda_volume_labels``): the ``(from, to)``
    pairs of ``remap`` in order, then -> ``(labels uint8 [Z,R,C], onehot uint8 [Z,K,R,C] or None, counter)``; ``counter``: int64
    ``[1]`` on the device, the number of values that are no integer in ``[0, num_classes)`` (written as background).  ``raw``:
    ``(int32 [Z,R,C] holding the values themselves, None, None)``, no remap and no range check."""
    z, r, c, sz, sr, sc = _volume_view("volume_labels", view, (torch.uint8, torch.int16, torch.int32, torch.float32, torch.float64))
    pairs = [(int(a), int(b)) for a, b in remap]
    if raw:
        if onehot or pairs:
            raise ValueError("volume_labels: raw output takes no remap and has no one-hot form")
        out = torch.empty((z, r, c), dtype=torch.int32, device=view.device)
        check(L.lib().pcuda_volume_labels(view.data_ptr(), _VOL_DTYPES[view.dtype], 0, sz, sr, sc, z, r, c, int(bool(flip_r)),
                                          int(bool(flip_c)), 0, None, 0, 1, out.data_ptr(), None, None, 0, _stream()), "volume_labels")
        return out, None, None
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 255:
        raise ValueError("volume_labels: 2..255 classes, got %r" % (num_classes,))
    if len(pairs) > 8:
        raise ValueError("volume_labels: a remap table of at most 8 (from, to) pairs, got %d" % len(pairs))
    lab = torch.empty((z, r, c), dtype=torch.uint8, device=view.device)
    hot = torch.empty((z, num_classes, r, c), dtype=torch.uint8, device=view.device) if onehot else None
    nbytes = L.lib().pcuda_volume_labels_workspace_size()
    ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=view.device)
    table = (C.c_int * max(2 * len(pairs), 1))(*[v for p in pairs for v in p])
    check(L.lib().pcuda_volume_labels(view.data_ptr(), _VOL_DTYPES[view.dtype], 0, sz, sr, sc, z, r, c, int(bool(flip_r)),
                                      int(bool(flip_c)), num_classes, C.cast(table, C.c_void_p), len(pairs), 0, lab.data_ptr(),
                                      _ptr(hot), ws.data_ptr(), nbytes, _stream()), "volume_labels")
    return lab, hot, ws[:1]


def volume_restore(pred, out_view, flip_r=False, flip_c=False, lut=None):
    """The inverse scatter (``pcuda_volume_restore``): uint8 ``pred [Z,R,C]`` into ``out_view``, a uint8 or int16 device view
    ``[Z,R,C]`` of any stride over the caller's array, through the same map, so that ``volume_labels(out_view) == pred``;
    ``lut``: an int16 ``[256]`` device table looked up first.  -> ``out_view``."""
    _req(pred, torch.uint8)
    z, r, c, sz, sr, sc = _volume_view("volume_restore", out_view, (torch.uint8, torch.int16))
    if tuple(pred.shape) != (z, r, c):
        raise ValueError("volume_restore: pred %r does not match the view %r" % (tuple(pred.shape), (z, r, c)))
    if lut is not None:
        _req(lut, torch.int16)
        if tuple(lut.shape) != (256,) or not lut.is_contiguous():
            raise ValueError("volume_restore: lut is a contiguous int16 [256] tensor")
    pred = pred.contiguous()
    check(L.lib().pcuda_volume_restore(pred.data_ptr(), z, r, c, out_view.data_ptr(), _VOL_DTYPES[out_view.dtype], 0, sz, sr, sc,
                                       int(bool(flip_r)), int(bool(flip_c)), _ptr(lut), _stream()), "volume_restore")
    return out_view


def argmax_labels(x):
    """[N,C,H,W] fp32 logits or uint8 one-hot -> uint8 label map [N,H,W]: first channel holding the maximum (a NaN in
    any channel: label 0, as the reference's np.max leaves no channel equal to it)."""
    if x.dtype not in (torch.float32, torch.uint8):
        raise TypeError("argmax_labels: fp32 logits or a uint8 one-hot mask")
    _req(x, x.dtype)
    n, c = x.shape[:2]
    hw = x.numel() // (n * c)
    if x.stride(-1) != 1 or (x.dim() == 4 and x.stride(2) != x.shape[3]):
        x = x.contiguous()
    lab = torch.empty((n,) + tuple(x.shape[2:]), dtype=torch.uint8, device=x.device)
    check(L.lib().pcuda_argmax_labels(x.data_ptr(), 1 if x.dtype == torch.uint8 else 0, x.stride(0), x.stride(1), n, c,
                                      hw, lab.data_ptr(), _stream()), "argmax_labels")
    return lab


def _out_size(name, h, w):
    for v in (h, w):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 16384:
            raise ValueError("%s: the output size (h, w) = (%r, %r) must be integers in 1..16384" % (name, h, w))


def area_resize(x, h, w):
    """``pcuda_area_resize``: fp32 planes ``[N,S_h,S_w]`` (or one plane ``[S_h,S_w]``; unit column stride, any row and plane
    stride) -> fp32 ``[N,h,w]`` by the build's INTER_AREA rule (parity with OpenCV not pinned): the area table
    where both axes shrink or stay, two taps per axis where one enlarges."""
    _out_size("area_resize", h, w)
    if not torch.is_tensor(x) or x.dim() not in (2, 3):
        raise ValueError("area_resize: fp32 planes [N,H,W] or one plane [H,W]")
    _req(x)
    v = x.unsqueeze(0) if x.dim() == 2 else x
    n, sh, sw = v.shape
    if sh < 1 or sw < 1:
        raise ValueError("area_resize: empty planes")
    if v.stride(2) != 1 or v.stride(1) < sw or v.stride(0) < 0 or (n > 1 and v.stride(0) == 0):
        v = v.contiguous()
    out = torch.empty((n, h, w), dtype=torch.float32, device=x.device)
    for i in range(0, n, 65535):
        m = min(65535, n - i)
        check(L.lib().pcuda_area_resize(v[i:i + m].data_ptr(), v.stride(0), v.stride(1), m, sh, sw, out[i:i + m].data_ptr(), h, w,
                                        _stream()), "area_resize")
    return out[0] if x.dim() == 2 else out


def reconstruct_resize_argmax(logits, h, w, crop_size=112, origin_size=256):
    """``pcuda_reconstruct_resize_argmax``: fp32 logits ``[N,C,2 crop,2 crop]`` as the network leaves them (C <= 8) -> uint8
    labels ``[N,h,w]``: ``reconstuct_volume`` into a zero ``origin_size`` canvas, ``resize_volume`` of every class plane to
    ``(h, w)`` and ``argmax`` (``evaluate_mscmrseg.py:139-145``) in one pass; neither the canvas nor the resized planes are
    written.  Ties and NaN as ``argmax_labels``."""
    _out_size("reconstruct_resize_argmax", h, w)
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise ValueError("reconstruct_resize_argmax: fp32 logits [N,C,H,W]")
    n, c, lh, lw = logits.shape
    if not 1 <= c <= 8:
        raise ValueError("reconstruct_resize_argmax: 1..8 classes, got %d" % c)
    o = int(origin_size / 2)
    if crop_size < 1 or o - crop_size < 0 or o + crop_size > origin_size:
        raise ValueError("reconstruct_resize_argmax: the window %d +- %d does not fit a canvas of %d" % (o, crop_size, origin_size))
    if (lh, lw) != (2 * crop_size, 2 * crop_size):
        raise ValueError("reconstruct_resize_argmax: logits of %dx%d, the window is %dx%d" % (lh, lw, 2 * crop_size, 2 * crop_size))
    _req(logits)
    if logits.stride(3) != 1 or logits.stride(2) < lw or min(logits.stride(0), logits.stride(1)) < 0 or \
            (c > 1 and logits.stride(1) == 0) or (n > 1 and logits.stride(0) == 0):
        logits = logits.contiguous()
    lab = torch.empty((n, h, w), dtype=torch.uint8, device=logits.device)
    for i in range(0, n, 65535):
        m = min(65535, n - i)
        check(L.lib().pcuda_reconstruct_resize_argmax(logits[i:i + m].data_ptr(), logits.stride(0), logits.stride(1), logits.stride(2),
                                                      m, c, lh, lw, crop_size, origin_size, lab[i:i + m].data_ptr(), h, w, _stream()),
              "reconstruct_resize_argmax")
    return lab


def label_dice(pred_labels, gt_labels, num_classes):
    """per-class Dice (medpy dc) of two uint8 label maps -> fp32 [num_classes] on the device"""
    _req(pred_labels, torch.uint8); _req(gt_labels, torch.uint8)
    if pred_labels.shape != gt_labels.shape:
        raise ValueError("label_dice: shapes differ")
    pred_labels, gt_labels = pred_labels.contiguous(), gt_labels.contiguous()
    ws = torch.empty(3 * num_classes, dtype=torch.int64, device=pred_labels.device)
    out = torch.empty(num_classes, dtype=torch.float32, device=pred_labels.device)
    check(L.lib().pcuda_label_dice(pred_labels.data_ptr(), gt_labels.data_ptr(), pred_labels.numel(), num_classes,
                                   out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()), "label_dice")
    return out


def _label_volume(t, name, spare=-2 ** 31):
    """a 2-D / 3-D integer label volume as the library reads it: contiguous uint8 or int32 (int64 values outside the
    int32 range, which no class value lies in, become ``spare``: an int32 value the caller matches nothing with), and
    its (ndim, z, h, w)"""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("%s: HIP device tensors only (no CPU fallback)" % name)
    if t.dim() not in (2, 3):
        raise ValueError("%s: 2-D [H,W] or 3-D [Z,H,W] label volumes (got shape %s)" % (name, tuple(t.shape)))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype not in (torch.uint8, torch.int32):
        if t.is_floating_point() or t.is_complex():
            raise TypeError("%s: integer label volumes only (got %s)" % (name, t.dtype))
        if t.dtype == torch.int64:
            t = t.masked_fill((t < -2 ** 31) | (t > 2 ** 31 - 1), spare)
        t = t.to(torch.int32)
    shp = (1,) * (3 - t.dim()) + tuple(t.shape)
    return t.contiguous(), t.dim(), shp


def _surface_args(name, pred, gt, classes, spacing):
    """the common front end of surface_metrics / surface_metrics_ext: both label volumes as the library reads them (one
    dtype), and (ndim, (z, h, w), the class values and the spacing as C arrays)"""
    cls = [int(c) for c in classes]
    if any(c < -2 ** 31 or c > 2 ** 31 - 1 for c in cls):
        raise ValueError("%s: class values must fit int32 (got %s)" % (name, cls))
    spare = next(v for v in range(-2 ** 31, -2 ** 31 + len(cls) + 1) if v not in cls)      # no class: wider labels go here
    pred, nd, shp = _label_volume(pred, name, spare)
    gt, nd_g, shp_g = _label_volume(gt, name, spare)
    if shp != shp_g or nd != nd_g:
        raise ValueError("%s: shapes differ (%s vs %s)" % (name, tuple(pred.shape), tuple(gt.shape)))
    if pred.dtype != gt.dtype:
        pred, gt = pred.to(torch.int32), gt.to(torch.int32)
    ccls = (C.c_int * max(1, len(cls)))(*cls)
    sp = None
    if spacing is not None:
        spacing = [float(v) for v in (spacing if hasattr(spacing, "__len__") else [spacing] * nd)]
        if len(spacing) != nd:
            raise ValueError("%s: %d spacing values for a %d-D volume" % (name, len(spacing), nd))
        sp = (C.c_double * nd)(*spacing)
    return pred, gt, nd, shp, ccls, len(cls), sp


def surface_metrics(pred, gt, classes, spacing=None, connectivity=1):
    """medpy's dc / hd / asd for every class value of ``classes`` (at most 8) between two label volumes of one shape
    (2-D or 3-D, uint8 or integer): fp64 ``[len(classes), 8]`` on the device, no host synchronisation.  Columns: dice,
    hd, asd(pred -> gt), asd(gt -> pred), |pred == c|, |gt == c|, |both|, flags (1: pred empty, 2: gt empty; hd and asd
    are NaN where a flag is set).  ``spacing``: per-axis voxel spacing (None = 1); ``connectivity``: 1..ndim, the
    footprint of the erosion that extracts the borders."""
    pred, gt, nd, shp, ccls, ncls, sp = _surface_args("surface_metrics", pred, gt, classes, spacing)
    lib = L.lib()
    wsb = lib.pcuda_surface_metrics_workspace_size(nd, *shp, ncls, sp)
    ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=pred.device)
    out = torch.empty((ncls, 8), dtype=torch.float64, device=pred.device)
    check(lib.pcuda_surface_metrics(pred.data_ptr(), gt.data_ptr(), 1 if pred.dtype == torch.int32 else 0, nd, *shp, ccls,
                                    ncls, int(connectivity), sp, out.data_ptr(), ws.data_ptr(), wsb, _stream()),
          "surface_metrics")
    return out


def surface_metrics_ext(pred, gt, classes, spacing=None, connectivity=1, percentile=95.0):
    """``surface_metrics`` with four more columns: fp64 ``[len(classes), 12]`` on the device, no host synchronisation.
    Columns 0..7 are those of ``surface_metrics`` (the same bits); 8: the ``percentile``-th percentile (0..100) of the
    distances of both directions pooled, as ``numpy.percentile`` (linear) gives it -- medpy's ``hd95`` at 95; 9: medpy's
    ``assd``, the mean of the two directed asd; 10, 11: the border voxel counts of pred and gt.  Columns 8 and 9 are NaN
    where a flag is set.  The percentile is an exact selection on the device: the same bits from run to run."""
    pred, gt, nd, shp, ccls, ncls, sp = _surface_args("surface_metrics_ext", pred, gt, classes, spacing)
    lib = L.lib()
    wsb = lib.pcuda_surface_metrics_ext_workspace_size(nd, *shp, ncls, sp)
    ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=pred.device)
    out = torch.empty((ncls, 12), dtype=torch.float64, device=pred.device)
    check(lib.pcuda_surface_metrics_ext(pred.data_ptr(), gt.data_ptr(), 1 if pred.dtype == torch.int32 else 0, nd, *shp,
                                        ccls, ncls, int(connectivity), sp, float(percentile), out.data_ptr(), ws.data_ptr(),
                                        wsb, _stream()), "surface_metrics_ext")
    return out


def largest_components(mask):
    """``keep_largest_connected_components`` (utils.py:43-65) of a 2-D / 3-D label volume on the device: for every label
    1..mask.shape[1] the largest face-connected component (ties: the one whose first voxel comes first in raster order),
    every other voxel 0; uint8 of the mask's shape.  Label values >= 256 in that range raise ValueError (the reference
    would wrap them in uint8)."""
    nl = int(mask.shape[1]) if mask.dim() >= 2 else 0
    if mask.is_cuda and mask.dtype not in (torch.uint8, torch.bool) and nl >= 256 and not mask.is_floating_point():
        if bool(((mask >= 256) & (mask <= nl)).any()):          # (a host synchronisation only for such masks)
            raise ValueError("largest_components: label values 256..%d do not fit the uint8 output" % nl)
    m, nd, shp = _label_volume(mask, "largest_components")
    lib = L.lib()
    wsb = lib.pcuda_largest_components_workspace_size(nd, *shp)
    ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=m.device)
    out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    check(lib.pcuda_largest_components(m.data_ptr(), 1 if m.dtype == torch.int32 else 0, nd, *shp, nl, out.data_ptr(),
                                       ws.data_ptr(), wsb, _stream()), "largest_components")
    return out


# ------------------------------------------------------------------------------------------
# dense
# ------------------------------------------------------------------------------------------
def linear_fwd(x, w, b):
    _req(x); _req(w)
    m, k = x.shape
    n = w.shape[0]
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    check(L.lib().pcuda_linear_fwd(x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), m, k, n, _stream()), "linear_fwd")
    return y


def linear_bwd_x(dy, w):
    m, n = dy.shape
    k = w.shape[1]
    dx = torch.empty((m, k), dtype=torch.float32, device=dy.device)
    check(L.lib().pcuda_linear_bwd_x(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), m, k, n, 0, _stream()), "linear_bwd_x")
    return dx


def linear_bwd_w(dy, x, dw, db, accumulate=True):
    m, n = dy.shape
    k = x.shape[1]
    lib = L.lib()
    nb = lib.pcuda_linear_bwd_w_workspace_size(m, k, n)
    ws = _workspace(nb, dy.device)
    check(lib.pcuda_linear_bwd_w(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), _ptr(db), m, k, n,
                                 1 if accumulate else 0, _ptr(ws), nb, _stream()), "linear_bwd_w")


def conv1d_fwd(x, w, b, want_stats=False):
    """torch.nn.Conv1d(cin, cout, 1) on [B,cin,L] in exact fp32 (MFMA f32): -> (y [B,cout,L], bn partials|None, ntiles)"""
    _req(x); _req(w)
    if not (x.is_contiguous() and w.is_contiguous()):
        raise ValueError("conv1d_fwd needs contiguous tensors")
    bsz, cin, l = x.shape
    cout = w.shape[0]
    lib = L.lib()
    y = torch.empty((bsz, cout, l), dtype=torch.float32, device=x.device)
    part, nt = None, 0
    if want_stats:
        nt = lib.pcuda_conv1d_k1_fwd_tiles(bsz, l)
        part = torch.empty((nt, cout, 2), dtype=torch.float32, device=x.device)
    check(lib.pcuda_conv1d_k1_fwd(x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), bsz, cin, cout, l, _ptr(part),
                                  _stream()), "conv1d_k1_fwd")
    return y, part, nt


def conv1d_dgrad(dy, w):
    _req(dy); _req(w)
    dy = dy.contiguous()
    bsz, cout, l = dy.shape
    cin = w.shape[1]
    dx = torch.empty((bsz, cin, l), dtype=torch.float32, device=dy.device)
    check(L.lib().pcuda_conv1d_k1_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), bsz, cin, cout, l, _stream()),
          "conv1d_k1_dgrad")
    return dx


def conv1d_wgrad(x, dy, dw, db, accumulate=True):
    _req(x); _req(dy)
    dy = dy.contiguous()
    bsz, cin, l = x.shape
    cout = dy.shape[1]
    lib = L.lib()
    nb = lib.pcuda_conv1d_k1_wgrad_workspace_size(bsz, cin, cout, l)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib.pcuda_conv1d_k1_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _ptr(db), bsz, cin, cout, l,
                                    1 if accumulate else 0, ws.data_ptr(), nb, _stream()), "conv1d_k1_wgrad")


def max_points_fwd(x):
    _req(x)
    b, c, l = x.shape
    y = torch.empty((b, c), dtype=torch.float32, device=x.device)
    idx = torch.empty((b, c), dtype=torch.int32, device=x.device)
    check(L.lib().pcuda_max_points_fwd(x.data_ptr(), b, c, l, y.data_ptr(), idx.data_ptr(), _stream()), "max_points_fwd")
    return y, idx


def max_points_bwd(dy, idx, l):
    b, c = dy.shape
    dx = torch.empty((b, c, l), dtype=torch.float32, device=dy.device)
    check(L.lib().pcuda_max_points_bwd(dy.data_ptr(), idx.data_ptr(), b, c, l, dx.data_ptr(), _stream()), "max_points_bwd")
    return dx


def bn_backward_maxpts(g, idx, a, st: BNState, gamma, dgamma, dbeta, post_relu=False, act_slope=1.0, accumulate=True,
                       frozen=False):
    """bn_backward(max_points_bwd(g, idx, L), a, ...) without the dense [B, C, L] gradient: (g, idx) are read in place.
    L <= 2048 (one tile of the general reduce per row); above that, and under PCUDA_PN_SMALL=0, the dense path."""
    _req(a); _req(g)
    b, c, l = a.shape
    if not (_pn_small and l <= 2048 and a.is_contiguous()):
        return bn_backward(max_points_bwd(g.contiguous(), idx, l), a, st, gamma, dgamma, dbeta, post_relu=post_relu,
                           act_slope=act_slope, accumulate=accumulate, frozen=frozen)
    g = g.contiguous()
    assert idx.is_contiguous() and idx.dtype == torch.int32 and g.shape == idx.shape == (b, c)
    lib = L.lib()
    pr = 1 if post_relu else 0

    def reduce():      # one tile per row: what pcuda_bn_bwd_reduce writes for the dense gradient, ntiles = b
        part = torch.empty((b, c, 2), dtype=torch.float32, device=a.device)
        check(lib.pcuda_bn_bwd_reduce_maxpts(g.data_ptr(), idx.data_ptr(), a.data_ptr(), st.mean.data_ptr(),
                                             st.invstd.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), pr, b, c, l,
                                             part.data_ptr(), _stream()), "bn_bwd_reduce_maxpts")
        return part, b

    def apply(coef, dz):
        check(lib.pcuda_bn_bwd_apply_maxpts(g.data_ptr(), idx.data_ptr(), a.data_ptr(), coef.data_ptr(),
                                            st.scale.data_ptr(), st.shift.data_ptr(), pr, float(act_slope), dz.data_ptr(),
                                            b, c, l, _stream()), "bn_bwd_apply_maxpts")

    return _bn_backward_chain(a, b * l, st, gamma, dgamma, dbeta, accumulate, frozen, reduce, apply)


def bmm(a, b, ta=False, tb=False):
    """C[i] = op(A[i]) op(B[i]); a: [B,m,k] (or [B,k,m] with ta), b: [B,k,n] (or [B,n,k] with tb)."""
    _req(a); _req(b)
    batch = a.shape[0]
    m, k = (a.shape[2], a.shape[1]) if ta else (a.shape[1], a.shape[2])
    n = b.shape[1] if tb else b.shape[2]
    c = torch.empty((batch, m, n), dtype=torch.float32, device=a.device)
    check(L.lib().pcuda_bmm(a.data_ptr(), b.data_ptr(), c.data_ptr(), batch, m, k, n, 1 if ta else 0, 1 if tb else 0, 0,
                            _stream()), "bmm")
    return c


# ------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------
def surface_vertices(mask_u8: torch.Tensor, max_verts: int, order: str = "lex"):
    """order "lex": this build's canonical list; "mc": marching-cubes traversal order with coincident duplicates"""
    _req(mask_u8, torch.uint8)
    b, h, w = mask_u8.shape
    verts = torch.zeros((b, max_verts, 3), dtype=torch.int32, device=mask_u8.device)
    counts = torch.empty(b, dtype=torch.int32, device=mask_u8.device)
    if order == "mc":
        check(L.lib().pcuda_surface_vertices_mc(mask_u8.data_ptr(), b, h, w, verts.data_ptr(), max_verts,
                                                counts.data_ptr(), _stream()), "surface_vertices_mc")
        return verts, counts
    if order != "lex":
        raise ValueError("order must be 'lex' or 'mc'")
    check(L.lib().pcuda_surface_vertices(mask_u8.data_ptr(), b, h, w, verts.data_ptr(), max_verts, counts.data_ptr(),
                                         None, 0, _stream()), "surface_vertices")
    return verts, counts


def fps(pts_f64: torch.Tensor, counts: torch.Tensor, first: torch.Tensor, k: int):
    _req(pts_f64, torch.float64); _req(counts, torch.int32); _req(first, torch.int32)
    b, npts_max, _ = pts_f64.shape
    idx = torch.empty((b, k), dtype=torch.int32, device=pts_f64.device)
    check(L.lib().pcuda_fps(pts_f64.data_ptr(), counts.data_ptr(), first.data_ptr(), b, npts_max, k, idx.data_ptr(),
                            _stream()), "fps")
    return idx


# ------------------------------------------------------------------------------------------
# optimiser steps
# ------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    check(L.lib().pcuda_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2,
                                  eps, weight_decay, step, grad_scale, _stream()), "adam_step")


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_t, grad_scale=1.0):
    """Adam with the step count in the int32 device tensor ``step_t`` (incremented by the call): graph-capturable."""
    check(L.lib().pcuda_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1,
                                      beta2, eps, weight_decay, step_t.data_ptr(), grad_scale, _stream()),
          "adam_step_dev")


def sgd_step(p, g, mom, lr, momentum, weight_decay, first_step, grad_scale=1.0):
    check(L.lib().pcuda_sgd_step(p.data_ptr(), g.data_ptr(), _ptr(mom), p.numel(), lr, momentum, weight_decay,
                                 1 if first_step else 0, grad_scale, _stream()), "sgd_step")


def guard_record(device):
    """A zeroed guard record (``pcuda_grad_norm``): int32 words; [0] norm and [1] coef are fp32 (``.view(torch.float32)``),
    [2] finite, [3] skipped and [4] applied (cumulative), [5] this step's decision."""
    return torch.zeros(L.GUARD_RECORD_WORDS, dtype=torch.int32, device=device)


def grad_norm(g, ranges, grad_scale, max_norm, skip_nonfinite, record, range_sumsq=None, workspace=None):
    """Global L2 norm of ``g * grad_scale`` over ``ranges`` (``(offset, numel)`` pairs in elements of the flat fp32 buffer
    ``g``) into the device ``record``, with the clip coefficient for ``max_norm`` (<= 0: none) and the skip decision; each
    range's own sum of squares goes to the float64 tensor ``range_sumsq`` when given.  Two launches, no atomics."""
    _req(g)
    _req(record, torch.int32)
    ranges = [(int(o), int(n)) for o, n in ranges]
    if record.numel() < L.GUARD_RECORD_WORDS or not record.is_contiguous() or not g.is_contiguous():
        raise ValueError("grad_norm: the record holds %d int32 words; flat contiguous buffers only" % L.GUARD_RECORD_WORDS)
    if any(o < 0 or n < 0 or o + n > g.numel() for o, n in ranges):
        raise ValueError("grad_norm: a range lies outside the buffer")
    if range_sumsq is not None:
        _req(range_sumsq, torch.float64)
        if range_sumsq.numel() < len(ranges) or not range_sumsq.is_contiguous():
            raise ValueError("grad_norm: range_sumsq holds one float64 per range")
    if workspace is None:
        workspace = torch.empty(L.GRAD_NORM_WORKSPACE_BYTES // 8, dtype=torch.float64, device=g.device)
    arr = (C.c_longlong * (2 * len(ranges)))(*[x for r in ranges for x in r])
    check(L.lib().pcuda_grad_norm(g.data_ptr(), arr, len(ranges), grad_scale, max_norm, 1 if skip_nonfinite else 0,
                                  record.data_ptr(), _ptr(range_sumsq), workspace.data_ptr(),
                                  workspace.numel() * workspace.element_size(), _stream()), "grad_norm")


def adam_step_guarded(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_t, record, skip_nonfinite, grad_scale=1.0):
    """``adam_step_dev`` with the gradient scaled by the record's clip coefficient; with ``skip_nonfinite`` and a non-finite
    norm in the record nothing is stored and ``step_t`` stays."""
    check(L.lib().pcuda_adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1,
                                          beta2, eps, weight_decay, step_t.data_ptr(), grad_scale, record.data_ptr(),
                                          1 if skip_nonfinite else 0, _stream()), "adam_step_guarded")


def sgd_step_guarded(p, g, mom, lr, momentum, weight_decay, init_t, mark_init, record, skip_nonfinite, grad_scale=1.0):
    """``sgd_step`` with the clip coefficient of the record and "momentum buffer initialised" in the int32 device tensor
    ``init_t`` (set behind the update when ``mark_init`` and the step is applied)."""
    check(L.lib().pcuda_sgd_step_guarded(p.data_ptr(), g.data_ptr(), _ptr(mom), p.numel(), lr, momentum, weight_decay,
                                         _ptr(init_t), 1 if mark_init else 0, grad_scale, record.data_ptr(),
                                         1 if skip_nonfinite else 0, _stream()), "sgd_step_guarded")


# ------------------------------------------------------------------------------------------
# profiling
# ------------------------------------------------------------------------------------------
def prof_enable(on: bool):
    check(L.lib().pcuda_prof_enable(1 if on else 0))


def prof_reset():
    check(L.lib().pcuda_prof_reset())


def prof_read(family: int):
    ms, work, n = C.c_double(0), C.c_double(0), C.c_longlong(0)
    check(L.lib().pcuda_prof_read(family, C.byref(ms), C.byref(work), C.byref(n)), "prof_read")
    return ms.value, work.value, n.value


def launch_count(reset: bool = False) -> int:
    """kernel launches issued by the library since the last reset (host-side counter)"""
    return int(L.lib().pcuda_launch_count(1 if reset else 0))


def last_kernel() -> str:
    """"<shape tag> | <kernel>" of this thread's most recent convolution launch (``pcuda_last_kernel``): kernel-level tests
    assert the dispatch with it"""
    v = L.lib().pcuda_last_kernel()
    return v.decode() if v else ""


def clock_ghz_under_load(dev, iters: int = 8192, reps: int = 3) -> float:
    """shader clock (GHz) while every SIMD of the chip issues MFMAs back to back (``pcuda_clock_probe``): the last of ``reps``
    ~3-ms launches, so that the power state has settled"""
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    sink = torch.zeros(1, dtype=torch.float32, device=dev)
    ghz = 0.0
    for _ in range(reps):
        check(L.lib().pcuda_clock_probe(out.data_ptr(), sink.data_ptr(), int(iters), _stream()), "clock_probe")
        c, r = (int(v) for v in out.tolist())
        ghz = 0.1 * c / max(r, 1)
    return ghz


def fallback_count() -> int:
    return int(L.lib().pcuda_fallback_count())


def prof_dump(path: str):
    check(L.lib().pcuda_prof_dump(path.encode()), "prof_dump")
