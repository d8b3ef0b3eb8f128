"""The variant sweep's child process: ``python conv_variant_child.py <table> <records.jsonl>``.

Runs every case of one table through ``kernels.ConvOp`` in both precisions, compares every result with the operand-exact
reference (tests/conv_exact_ref.py) and writes one JSON line per operation: case, operation, precision, the (family, key) pairs
the operation was the FIRST of this process to dispatch (``PCUDA_VARIANT_LOG``, re-read after each operation), ``last_kernel()``,
the error, ``e32`` and the bound.  The library reads ``PCUDA_VARIANT_LOG`` and its A/B switches once per process, which is why
this is a process of its own (tests/test_conv_variants_gpu.py starts it).  Stops at the first HIP error and exits non-zero.

The tables were picked greedily (fewest cases first, then fewest multiply-adds) from a dispatch-only search over ~50 000
geometries x {aligned, off by one float} x {one source, two sources}, restricted to cin >= 32 -- at least one FULL 32-channel
chunk, mostly a second ragged one (40 = 32 + 8), so that an error in any channel of a chunk is seen -- and cout >= 24.  A case:
(n, cin, cout, h, w, k, stride, pad, dil, in_up, mis, xs): h, w the logical input size; mis = 1: activations and gradients are
views one float behind a 256-byte boundary; xs > 0: the weight gradient reads its input from two tensors, xs + (cin - xs)
channels (the zero-copy concat; xs no multiple of 32 sends it down the unpipelined path).
"""
import json
import os
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

# which operations a table runs
CONV_OPS, WGRAD_OPS = "conv", "wgrad"

TABLES = {
    # four-wave pipelined forward / dgrad kernel: > 320 (tile, co-tile) items or a 32-row co-tile on 128-pixel tiles
    "pipe": (CONV_OPS, {}, [
        (16, 32, 32, 20, 24, 1, 1, 0, 1, 0, 0, 0),
        (1, 32, 32, 8, 8, 1, 1, 0, 1, 0, 0, 0),
        (1, 40, 24, 17, 17, 3, 2, 1, 1, 0, 0, 0),
        (48, 32, 512, 6, 6, 1, 1, 0, 1, 0, 0, 0),
        (12, 40, 24, 57, 57, 1, 1, 0, 1, 0, 0, 0),
        (1, 40, 24, 4, 4, 1, 1, 0, 1, 0, 0, 0),
        (1, 40, 24, 8, 8, 1, 1, 0, 1, 1, 0, 0),
        (48, 32, 512, 8, 8, 1, 1, 0, 1, 0, 0, 0),
        (24, 40, 24, 56, 56, 1, 1, 0, 1, 0, 0, 0),
        (16, 40, 24, 21, 19, 3, 1, 1, 1, 0, 0, 0),
        (16, 40, 24, 20, 24, 3, 1, 1, 1, 1, 0, 0),
        (12, 32, 256, 28, 28, 1, 1, 0, 1, 1, 0, 0),
        (12, 256, 32, 28, 28, 1, 1, 0, 1, 0, 0, 0),
        (24, 40, 24, 65, 65, 1, 1, 0, 1, 0, 0, 0),
        (24, 32, 64, 56, 56, 1, 1, 0, 1, 0, 0, 0),
        (12, 40, 24, 57, 57, 3, 1, 4, 4, 0, 0, 0),
        (24, 512, 32, 8, 8, 2, 2, 0, 1, 0, 0, 0),
        (12, 40, 24, 128, 128, 4, 2, 2, 1, 0, 0, 0),
        (24, 32, 48, 56, 56, 3, 1, 1, 1, 1, 0, 0),
    ]),
    # eight-wave kernel: <= 320 items or an LDS tile above 80 KiB
    "ig8": (CONV_OPS, {}, [
        (1, 32, 64, 57, 57, 2, 2, 0, 1, 0, 0, 0),
        (1, 40, 24, 12, 16, 3, 1, 2, 2, 0, 0, 0),
        (1, 48, 64, 1, 300, 3, 2, 1, 1, 0, 0, 0),
        (1, 48, 64, 8, 64, 6, 1, 0, 1, 0, 0, 0),
        (1, 32, 64, 4, 4, 2, 2, 0, 1, 0, 0, 0),
        (1, 32, 64, 12, 16, 1, 1, 0, 1, 0, 0, 0),
        (1, 32, 64, 28, 28, 3, 2, 1, 1, 0, 0, 0),
        (1, 40, 24, 12, 16, 1, 1, 0, 1, 0, 0, 0),
        (1, 32, 64, 16, 16, 2, 2, 0, 1, 0, 0, 0),
        (1, 32, 64, 17, 17, 3, 2, 1, 1, 0, 0, 0),
        (1, 40, 24, 14, 14, 3, 1, 2, 2, 0, 0, 0),
        (1, 40, 24, 20, 24, 3, 1, 4, 4, 0, 0, 0),
    ]),
    "wgrad": (WGRAD_OPS, {}, [
        (1, 32, 64, 4, 4, 2, 2, 0, 1, 0, 0, 0),
        (1, 40, 24, 8, 8, 4, 2, 1, 1, 0, 0, 0),
        (1, 32, 64, 16, 16, 2, 2, 0, 1, 0, 0, 0),
        (1, 32, 64, 17, 17, 2, 2, 0, 1, 0, 0, 0),
        (1, 32, 64, 1, 300, 1, 1, 0, 1, 0, 0, 0),
        (1, 32, 64, 8, 64, 2, 2, 0, 1, 0, 0, 0),
        (1, 32, 64, 16, 16, 3, 2, 1, 1, 0, 0, 0),
        (1, 40, 24, 21, 19, 4, 2, 1, 1, 0, 0, 0),
        (1, 32, 64, 21, 19, 4, 2, 1, 1, 0, 0, 0),
        (1, 32, 64, 16, 24, 4, 2, 1, 1, 0, 0, 0),
        (1, 48, 48, 21, 19, 4, 2, 1, 1, 0, 0, 24),
        (1, 32, 64, 12, 16, 3, 1, 1, 1, 0, 0, 0),
        (1, 40, 24, 8, 64, 3, 1, 1, 1, 0, 0, 0),
        (1, 32, 64, 20, 24, 3, 1, 1, 1, 0, 0, 0),
        (1, 32, 64, 8, 64, 3, 1, 1, 1, 0, 0, 0),
        (1, 40, 24, 56, 56, 3, 1, 1, 1, 1, 0, 0),
        (1, 40, 24, 4, 4, 1, 1, 0, 1, 1, 0, 0),
        (1, 32, 64, 4, 4, 1, 1, 0, 1, 1, 0, 0),
        (1, 40, 24, 8, 8, 1, 1, 0, 1, 1, 0, 0),
        (1, 40, 24, 16, 16, 2, 2, 0, 1, 0, 0, 0),
        (1, 40, 24, 1, 300, 1, 1, 0, 1, 0, 0, 0),
        (1, 32, 64, 4, 4, 3, 1, 1, 1, 0, 0, 0),
        (1, 40, 24, 8, 64, 1, 1, 0, 1, 1, 0, 0),
        (1, 40, 24, 8, 64, 2, 2, 0, 1, 0, 0, 0),
        (1, 32, 64, 8, 8, 4, 2, 1, 1, 0, 0, 0),
        (1, 40, 24, 12, 16, 3, 1, 1, 1, 0, 0, 0),
        (1, 40, 24, 20, 24, 3, 1, 1, 1, 0, 0, 0),
        (1, 32, 64, 17, 17, 3, 1, 8, 8, 0, 0, 0),
        (1, 32, 64, 65, 65, 2, 2, 0, 1, 0, 0, 0),
        (1, 40, 24, 4, 4, 1, 1, 0, 1, 0, 1, 0),
        (1, 32, 64, 56, 56, 3, 1, 1, 1, 1, 0, 0),
    ]),
    # the 1x1 / stride-1 kernel (csrc/conv_wgrad1.hip) takes these shapes in front of the keyed kernels: its documented A/B switch
    "wgrad_no_wgrad1": (WGRAD_OPS, {"PCUDA_NO_WGRAD1": "1"}, [
        (1, 40, 24, 8, 64, 1, 1, 0, 1, 0, 0, 0),
        (1, 32, 64, 8, 64, 1, 1, 0, 1, 0, 0, 0),
    ]),
}
SLOPE = 0.2


class Log:
    def __init__(self, path):
        self.path, self.pos = path, 0

    def new_keys(self):
        if not os.path.exists(self.path):
            return []
        with open(self.path) as fh:
            fh.seek(self.pos)
            txt = fh.read()
            self.pos = fh.tell()
        return [[ln.split()[0], int(ln.split()[1])] for ln in txt.splitlines() if ln.strip()]


def _dev(t, dev, mis=0):
    """a device copy; mis: as a view ``mis`` floats behind an aligned allocation"""
    if not mis:
        return t.to(dev)
    flat = torch.empty(t.numel() + 64 + mis, dtype=t.dtype, device=dev)
    v = flat[mis:mis + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _empty(shape, dev, mis=0, fill=None):
    n = int(np.prod(shape))
    flat = torch.empty(n + 64 + mis, dtype=torch.float32, device=dev)
    v = flat[mis:mis + n].view(shape)
    if fill is not None:
        v.fill_(fill)
    return v


def _check(what, got, fn, old_ref, prec, axis=1, old_tol=None):
    """one tensor against its operand-exact reference: error, e32, bound = FACTOR x e32, and the project's old bound"""
    e32, ref = R.e32_of(fn, axis=axis)
    err = R.chan_err(got, ref, axis=axis)
    old_err = R.rel_err(got, old_ref)
    return dict(what=what, err=err, e32=e32, bound=R.bound_of(e32, prec), old_err=old_err, old_bound=old_tol or R.OLD_TOL[prec])


def _check_sums(what, got, fn, old_pair, old_tol, prec):
    """per-channel sums; fn(dtype) -> (sum, scale = sum of |terms|); old_pair = the unrounded (sum, scale); prec None: a sum of
    fp32 values no MFMA produced (the bias gradient)"""
    s64, a64 = fn(torch.float64)
    s32, _ = fn(torch.float32)
    e32 = R.sum_err(s32, s64, a64)
    err = R.sum_err(got, s64, a64)
    old_err = R.rel_err(got, old_pair[0])      # (the project's measure for these sums: whole vector)
    return dict(what=what, err=err, e32=e32, bound=R.bound_of(e32, prec), old_err=old_err, old_bound=old_tol)


class Case:
    def __init__(self, idx, case, dev):
        self.case = case
        n, cin, cout, h, w, k, s, p, d, up, self.mis, self.xs = case
        self.g = g = R.Geom(n, cin, cout, h, w, k, s, p, d, up)
        rng = np.random.default_rng(1000 + idx)
        t = lambda *sh, sd=1.0, mu=0.0: torch.from_numpy(rng.normal(mu, sd, sh).astype(np.float32))
        sh, sw = (h // 2, w // 2) if up else (h, w)
        self.x, self.w, self.b = t(n, cin, sh, sw), t(cout, cin, k, k, sd=0.1), t(cout, sd=0.1)
        self.dz = t(n, cout, g.oh, g.ow)
        self.base = t(n, cin, h, w)                      # what an accumulating dgrad adds to
        self.a = t(n, cin, h, w)                         # saved activation (LeakyReLU mask, BatchNorm reduce)
        self.a_half = t(n, cin, sh, sw)
        self.mean = t(cin, sd=0.3)
        self.invstd = torch.from_numpy(rng.uniform(0.5, 2.0, (cin,)).astype(np.float32))
        self.base_w, self.base_b = t(cout, cin, k, k), t(cout)
        self.dev = dev
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]


def conv_ops(c, prec, K):
    """yields (operation name, thunk -> list of checks)"""
    g, dev, mis = c.g, c.dev, c.mis
    op = K.ConvOp(g.cin, g.cout, g.k, stride=g.stride, pad=g.pad, dil=g.dil, in_up=g.in_up)
    xd, wd, bd, dzd = _dev(c.x, dev, mis), c.w.to(dev), c.b.to(dev), _dev(c.dz, dev, mis)
    fw = {}

    def fwd(dt):      # (shared by the forward operations)
        if dt not in fw:
            fw[dt] = R.forward_ref(g, c.x, c.w, c.b, SLOPE, prec, dt)
        return fw[dt]
    fwd_old = c.memo("fwd_old", lambda: R.forward_ref(g, c.x, c.w, c.b, SLOPE, None))
    dg_old = c.memo("dg_old", lambda: R.dgrad_ref(g, c.dz, c.w, None))
    dg = {dt: R.dgrad_ref(g, c.dz, c.w, prec, dt) for dt in (torch.float64, torch.float32)}      # shared by the dgrad operations
    st = K.BNState()
    st.mean, st.invstd = c.mean.to(dev), c.invstd.to(dev)

    def sums_of(red):
        part, nt = red
        return part[:nt].double().sum(0).cpu()

    def f_fwd():
        out = _empty((g.n, g.cout, g.oh, g.ow), dev, mis, float("nan"))
        y, _, _ = op.forward(xd, wd, bd, SLOPE, g.h, g.w, out=out)
        return [_check("y", y, fwd, fwd_old, prec)]
    yield "fwd", f_fwd

    def f_fwd_stats():
        out = _empty((g.n, g.cout, g.oh, g.ow), dev, mis, float("nan"))
        y, part, nt = op.forward(xd, wd, bd, SLOPE, g.h, g.w, out=out, want_stats=True)
        got = sums_of((part, nt))
        old = R.bn_fwd_sums(fwd_old)
        tol = max(R.OLD_TOL[prec], 1e-4) * 10
        return [_check("y", y, fwd, fwd_old, prec),
                _check_sums("sum y", got[:, 0], lambda dt: R.bn_fwd_sums(fwd(dt), dt)[0], old[0], tol, prec),
                _check_sums("sum y^2", got[:, 1], lambda dt: R.bn_fwd_sums(fwd(dt), dt)[1], old[1], tol, prec)]
    yield "fwd_stats", f_fwd_stats

    def f_dgrad():
        dx = _empty((g.n, g.cin, g.h, g.w), dev, mis, float("nan"))
        op.dgrad(dzd, wd, g.h, g.w, dx=dx)
        return [_check("dx", dx, lambda dt: dg[dt], dg_old, prec)]
    yield "dgrad", f_dgrad

    def f_dgrad_acc():
        dx = _dev(c.base, dev, mis)
        op.dgrad(dzd, wd, g.h, g.w, dx=dx, accumulate=True)
        return [_check("dx", dx, lambda dt: dg[dt] + c.base.to(dt), dg_old + c.base.double(), prec)]
    yield "dgrad_acc", f_dgrad_acc

    if g.cin >= 16:
        def f_dgrad_split():
            c1 = max(8, (g.cin // 2) // 8 * 8)
            d1 = _empty((g.n, c1, g.h, g.w), dev, mis, float("nan"))
            d2 = _empty((g.n, g.cin - c1, g.h, g.w), dev, mis, float("nan"))
            op.dgrad(dzd, wd, g.h, g.w, dx=d1, dx2=d2)
            return [_check("dx", torch.cat([d1, d2], 1), lambda dt: dg[dt], dg_old, prec)]
        yield "dgrad_split", f_dgrad_split

    if g.stride == 1 and not g.in_up:
        def f_dgrad_bnred():
            dx = _empty((g.n, g.cin, g.h, g.w), dev, mis, float("nan"))
            dx, red = op.dgrad(dzd, wd, g.h, g.w, dx=dx, bnred=(c.a.to(dev), st))
            out = [_check("dx", dx, lambda dt: dg[dt], dg_old, prec)]
            if red is not None:
                got = sums_of(red)
                old = R.bnred_sums(dg_old, c.a, c.mean, c.invstd)
                for i, nm in enumerate(("sum g", "sum g a_hat")):
                    out.append(_check_sums(nm, got[:, i], lambda dt, i=i: R.bnred_sums(dg[dt], c.a, c.mean, c.invstd, dt)[i],
                                           old[i], max(R.OLD_TOL[prec], 1e-4) * 10, prec))
            return out
        yield "dgrad_bnred", f_dgrad_bnred

    if g.k > 1 and not g.in_up:
        def f_dgrad_lrelu():
            dx = op.dgrad_lrelu(dzd, wd, g.h, g.w, c.a.to(dev), SLOPE)
            return [_check("dx", dx, lambda dt: R.dgrad_ref(g, c.dz, c.w, prec, dt, mask=(c.a, SLOPE)),
                           R.dgrad_ref(g, c.dz, c.w, None, mask=(c.a, SLOPE)), prec)]
        yield "dgrad_lrelu", f_dgrad_lrelu

    if g.in_up:
        def f_dgrad_fold(bn):
            r = op.dgrad_fold(dzd, wd, g.h, g.w, bnred=(c.a_half.to(dev), st) if bn else None)
            dx, red = r if bn else (r, None)
            old_f = R.fold2(dg_old)
            out = [_check("dx", dx, lambda dt: R.fold2(dg[dt]), old_f, prec)]
            if red is not None:
                got = sums_of(red)
                old = R.bnred_sums(old_f, c.a_half, c.mean, c.invstd)
                for i, nm in enumerate(("sum g", "sum g a_hat")):
                    out.append(_check_sums(nm, got[:, i],
                                           lambda dt, i=i: R.bnred_sums(R.fold2(dg[dt]), c.a_half, c.mean, c.invstd, dt)[i],
                                           old[i], max(R.OLD_TOL[prec], 1e-4) * 10, prec))
            return out
        yield "dgrad_fold", lambda: f_dgrad_fold(False)
        yield "dgrad_fold_bnred", lambda: f_dgrad_fold(True)


def wgrad_ops(c, prec, K):
    g, dev, mis, xs = c.g, c.dev, c.mis, c.xs
    op = K.ConvOp(g.cin, g.cout, g.k, stride=g.stride, pad=g.pad, dil=g.dil, in_up=g.in_up)
    dzd = _dev(c.dz, dev, mis)
    if xs:
        x1, x2 = _dev(c.x[:, :xs].contiguous(), dev, mis), _dev(c.x[:, xs:].contiguous(), dev, mis)
    else:
        x1, x2 = _dev(c.x, dev, mis), None
    wg = {dt: R.wgrad_ref(g, c.x, c.dz, prec, dt) for dt in (torch.float64, torch.float32)}
    wg_old = c.memo("wg_old", lambda: R.wgrad_ref(g, c.x, c.dz, None))
    db = lambda dt: R.chan_sums(c.dz, dt)
    db_old = R.chan_sums(c.dz)
    nan = float("nan")

    def f_wgrad():
        dw = torch.full(c.w.shape, nan, device=dev)
        op.wgrad(x1, dzd, dw, None, g.h, g.w, x2=x2, accumulate=False)
        return [_check("dw", dw, lambda dt: wg[dt], wg_old, prec, axis=0)]
    yield "wgrad", f_wgrad

    def f_wgrad_db():
        dw, dbias = torch.full(c.w.shape, nan, device=dev), torch.full((g.cout,), nan, device=dev)
        op.wgrad(x1, dzd, dw, dbias, g.h, g.w, x2=x2, accumulate=False)
        return [_check("dw", dw, lambda dt: wg[dt], wg_old, prec, axis=0), _check_sums("db", dbias, db, db_old, 1e-4, None)]
    yield "wgrad_db", f_wgrad_db

    def f_wgrad_acc():
        dw, dbias = c.base_w.to(dev), c.base_b.to(dev)
        op.wgrad(x1, dzd, dw, dbias, g.h, g.w, x2=x2, accumulate=True)
        dbs = lambda dt: (db(dt)[0] + c.base_b.to(dt), db(dt)[1] + c.base_b.abs().double())
        return [_check("dw", dw, lambda dt: wg[dt] + c.base_w.to(dt), wg_old + c.base_w.double(), prec, axis=0),
                _check_sums("db", dbias, dbs, dbs(torch.float64), 1e-4, None)]
    yield "wgrad_acc", f_wgrad_acc


def main(table, out_path):
    from pointcloududa_amd import kernels as K
    kind, _env, cases = TABLES[table]
    dev = torch.device("cuda", 0)
    log = Log(os.environ["PCUDA_VARIANT_LOG"])
    t_start = time.time()
    with open(out_path, "w") as out:
        for idx, case in enumerate(cases):
            c = Case(idx, case, dev)
            for prec in ("bf16x3", "bf16"):
                K.set_precision(prec)
                for name, thunk in (conv_ops if kind == CONV_OPS else wgrad_ops)(c, prec, K):
                    t0 = time.time()
                    checks = thunk()
                    torch.cuda.synchronize()          # a HIP error of this operation surfaces here: nothing runs after it
                    keys = log.new_keys()
                    worst = max(checks, key=lambda q: (q["err"] / q["e32"]) if q["e32"] > 0 else (0.0 if q["err"] == 0 else float("inf")))
                    ok = all(q["err"] <= q["bound"] and q["old_err"] < q["old_bound"] for q in checks)
                    rec = dict(table=table, case=list(case), op=name, prec=prec, keys=keys, last_kernel=K.last_kernel(), err=worst["err"],
                               e32=worst["e32"], bound=worst["bound"], ok=ok, checks=checks, macs=c.g.macs, seconds=round(time.time() - t0, 4))
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
