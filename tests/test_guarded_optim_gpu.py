"""Guarded optimiser steps at kernel level: the device-side gradient norm (csrc/optim.hip, ``pcuda_grad_norm``) and the update
kernels that take "clip by how much" and "skip this step" from the record it leaves in device memory.

The rule, restated here in numpy:

  x_i   = float32(g_i * grad_scale)                      the very product the update kernels form
  total = sum(float64(x_i) ** 2)                         in double, in a fixed order, no atomics
  norm  = float32(sqrt(total))
  coef  = min(1, max_norm / (norm + 1e-6))  in float32   (max_norm <= 0: 1; a NaN norm gives a NaN coefficient, as
                                                          torch.clamp(max=1) does in clip_grad_norm_)
  finite = isfinite(norm)                                a sum that overflows float32 counts as non-finite
  gi    = (g_i * grad_scale) * coef                      two rounded float32 products; coef == 1 changes no bit

Bounds.  norm: one float32 ulp of the float64 restatement -- derived, not measured: a sum of n non-negative doubles in any
order is within (n - 1) * 2^-53 relative of exact (~2^-32 at n = 2^21), far below half a float32 ulp, so the two roundings to
float32 can differ only at a rounding boundary.  coef / finite: bit for bit from the device's own norm.  Per-range sums: 1e-12
relative.  Updates: bit for bit against the unguarded kernels fed the pre-multiplied gradient; 1e-6 against float64
torch.optim behind clip_grad_norm_ (M_NUMEL1 for Adam's first moment at numel 1: test_pointwise_edges_gpu.py).

Sizes: 1, 257, 5000 and 2097152 + 3.  The last passes both grid caps: 8192 workgroups of one element per lane in the update
kernels, 2048 workgroups of four elements per lane in the norm's first pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err

gpu = pytest.mark.gpu

NUMELS = [1, 257, 5000, 2097152 + 3]
M_NUMEL1 = 4 * 1.49e-6          # test_pointwise_edges_gpu.py: Adam's first moment at numel 1
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8)
WD_ADAM, LR_SGD, WD_SGD = 0.01, 2.5e-2, 0.0005


# ------------------------------------------------------------------------------------------------ the rule in numpy
def ref_sumsq(g, scale, ranges):
    """float64 sums of squares of float32(g * scale), one per range"""
    x = (np.asarray(g, dtype=np.float32) * np.float32(scale)).astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.array([np.sum(x[o:o + n] ** 2) for o, n in ranges], dtype=np.float64)


def ref_norm(g, scale, ranges):
    with np.errstate(all="ignore"):
        return np.float32(np.sqrt(ref_sumsq(g, scale, ranges).sum()))


def ref_coef(norm32, max_norm):
    if max_norm <= 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
        return np.minimum(np.float32(1.0), c)          # propagates NaN


def same_bits(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def read(rec):
    """the device record -> dict"""
    w = rec.cpu().numpy()
    f = w[:2].view(np.float32)
    return dict(norm=f[0], coef=f[1], finite=int(w[2]), skipped=int(w[3]), applied=int(w[4]), skip=int(w[5]))


def check_record(r, g, scale, ranges, max_norm):
    want = ref_norm(g, scale, ranges)
    if np.isfinite(want):
        assert abs(np.float64(r["norm"]) - np.float64(want)) <= np.spacing(want), (r["norm"], want)
    else:
        assert same_bits(r["norm"], want), (r["norm"], want)
    assert same_bits(r["coef"], ref_coef(r["norm"], max_norm)), (r["coef"], ref_coef(r["norm"], max_norm))
    assert r["finite"] == int(np.isfinite(r["norm"]))


@functools.lru_cache(maxsize=None)
def _inputs(numel):
    rng = np.random.default_rng(1701)
    mk = lambda: torch.from_numpy(rng.normal(0, 1, numel).astype(np.float32))
    return mk(), tuple(mk() for _ in range(3))


def _max_norm_between(grads, k):
    """a max_norm that clips the largest of the three gradients (x k) and neither of the others"""
    n = sorted(float(ref_norm(g.numpy(), k, [(0, g.numel())])) for g in grads)
    assert n[1] < n[2]
    return float(np.sqrt(n[1] * n[2]))


# ------------------------------------------------------------------------------------------------ 1. norm against float64
@gpu
@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("scale", [1.0, 0.25, 1.0 / 3.0])
def test_norm_against_float64(dev, numel, scale):
    from pointcloududa_amd import kernels as K
    _, grads = _inputs(numel)
    g = grads[0]
    full = [(0, numel)]
    n0 = float(ref_norm(g.numpy(), scale, full))
    gd = g.to(dev)
    for max_norm in (0.0, 0.5 * n0, 2.0 * n0):        # none, clipping, not clipping
        rec = K.guard_record(dev)
        K.grad_norm(gd, full, scale, max_norm, False, rec)
        r = read(rec)
        print("numel %d scale %.3g max_norm %.3g: norm %.9g (float64 %.9g) coef %.9g" % (numel, scale, max_norm, r["norm"], n0, r["coef"]))
        check_record(r, g.numpy(), scale, full, max_norm)
        assert r["finite"] == 1 and r["applied"] == 1 and r["skipped"] == 0 and r["skip"] == 0
    assert read(rec)["coef"] == 1.0
    K.grad_norm(gd, full, scale, 0.5 * n0, False, rec)
    assert 0.49 < read(rec)["coef"] < 0.51 and read(rec)["applied"] == 2


# ------------------------------------------------------------------------------------------------ 2. ranges
# three ranges with gaps, starting 1, 2 and 3 elements past a 16-byte boundary, with scalar tails of 1, 2 and 3 elements;
# "small": one or two workgroups per range; "capped": more work than the capped grid holds, shared out by size
RANGE_SETS = {
    "small": (3700, [(1, 3 + 4 * 500 + 1), (2010, 2 + 4 * 300 + 2), (3219, 1 + 4 * 100 + 3)]),
    "capped": (2120100, [(1, 3 + 4 * 400000 + 1), (1600010, 2 + 4 * 100000 + 2), (2000019, 1 + 4 * 30000 + 3)]),
    "tiny": (64, [(1, 1), (6, 2), (11, 3)]),           # heads only: no range reaches a 16-byte boundary with 4 elements left
}


@gpu
@pytest.mark.parametrize("name", list(RANGE_SETS))
def test_ranges_with_gaps_of_nan_and_inf(dev, name):
    from pointcloududa_amd import kernels as K
    total, ranges = RANGE_SETS[name]
    for (o, n), off, tail in zip(ranges, (1, 2, 3), (1, 2, 3)):
        assert o % 4 == off and (name == "tiny" or (n - (4 - off)) % 4 == tail)
    rng = np.random.default_rng(5)
    vals = rng.normal(0, 1, total).astype(np.float32)
    g = np.where(np.arange(total) % 2 == 0, np.float32(np.nan), np.float32(np.inf)).astype(np.float32)
    for o, n in ranges:
        g[o:o + n] = vals[o:o + n]
    gd = torch.from_numpy(g).to(dev)
    assert gd.data_ptr() % 16 == 0
    rec, sums = K.guard_record(dev), torch.zeros(3, dtype=torch.float64, device=dev)
    K.grad_norm(gd, ranges, 0.5, 1.0, True, rec, sums)
    r = read(rec)
    assert r["finite"] == 1 and r["skip"] == 0 and np.isfinite(r["norm"])
    check_record(r, g, 0.5, ranges, 1.0)
    want = ref_sumsq(g, 0.5, ranges)
    got = sums.cpu().numpy()
    print(name, "range sums, relative to float64:", np.abs(got - want) / want)
    assert np.all(np.abs(got - want) <= 1e-12 * want)
    assert np.float32(np.sqrt(got.sum())).tobytes() == np.float32(r["norm"]).tobytes()      # the total is the ranges' sum


# ------------------------------------------------------------------------------------------------ 3. same bits from run to run
@gpu
def test_two_calls_give_the_same_bits(dev):
    from pointcloududa_amd import kernels as K
    total, ranges = RANGE_SETS["capped"]
    gd = torch.from_numpy(np.random.default_rng(6).normal(0, 1, total).astype(np.float32)).to(dev)
    out = []
    rec = K.guard_record(dev)
    for _ in range(2):
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        K.grad_norm(gd, ranges, 1.0, 3.0, False, rec, sums)
        out.append((rec.cpu().numpy().copy(), sums.cpu().numpy().tobytes()))
    (w0, s0), (w1, s1) = out
    assert s0 == s1 and w0[[0, 1, 2, 5]].tobytes() == w1[[0, 1, 2, 5]].tobytes()
    assert (w0[3], w0[4], w1[3], w1[4]) == (0, 1, 0, 2)              # the counters are cumulative


# ------------------------------------------------------------------------------------------------ 4. clipped update
def _torch_ref(kind, p0, momentum, wd):
    """float64 torch.optim on the hyper-parameters the kernels receive: float32 values (as tests/fp64_refs.py takes them;
    1 - 0.99 differs from 1 - float32(0.99) by 9.5e-7 of itself)"""
    f = lambda x: float(np.float32(x))
    pr = p0.double().clone().requires_grad_(True)
    if kind == "adam":
        return pr, torch.optim.Adam([pr], lr=f(ADAM["lr"]), betas=(f(ADAM["beta1"]), f(ADAM["beta2"])), eps=f(ADAM["eps"]),
                                    weight_decay=f(wd))
    return pr, torch.optim.SGD([pr], lr=f(LR_SGD), momentum=f(momentum), weight_decay=f(wd))


CASES = [("adam_wd", "adam", 0.0, 1.0), ("sgd_momentum", "sgd", 0.99, 1.0), ("sgd_momentum0", "sgd", 0.0, 1.0),
         ("adam_scale", "adam", 0.0, 0.25), ("sgd_scale", "sgd", 0.99, 0.25)]


@gpu
@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("tag,kind,momentum,scale", CASES, ids=[c[0] for c in CASES])
def test_clipped_update_bit_for_bit(dev, numel, tag, kind, momentum, scale):
    from pointcloududa_amd import kernels as K
    p0, grads = _inputs(numel)
    grads = [g * (1.0 / scale) for g in grads]          # summed gradients of 1 / scale ranks
    max_norm = _max_norm_between(grads, scale)
    wd = WD_ADAM if kind == "adam" else WD_SGD
    z = lambda: torch.zeros(numel, device=dev)
    # guarded | the unguarded kernels on copies, fed (g * scale) * coef
    p, m, v, buf = p0.to(dev), z(), z(), (z() if momentum else None)
    pc, mc, vc, bufc = p0.to(dev), z(), z(), (z() if momentum else None)
    step_t, step_c = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    init_t = torch.zeros(1, dtype=torch.int32, device=dev)
    rec = K.guard_record(dev)
    pr, topt = _torch_ref(kind, p0, momentum, wd)
    coefs = []
    for i, g in enumerate(grads):
        gd = g.to(dev)
        K.grad_norm(gd, [(0, numel)], scale, max_norm, False, rec)
        coef_t = rec[1:2].view(torch.float32)
        pre = (gd * scale) * coef_t
        if kind == "adam":
            K.adam_step_guarded(p, gd, m, v, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], wd, step_t, rec, False, scale)
            K.adam_step_dev(pc, pre, mc, vc, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], wd, step_c)
            assert torch.equal(m, mc) and torch.equal(v, vc) and int(step_t) == i + 1
        else:
            K.sgd_step_guarded(p, gd, buf, LR_SGD, momentum, wd, init_t if momentum else None, True, rec, False, scale)
            K.sgd_step(pc, pre, bufc, LR_SGD, momentum, wd, i == 0)
            if momentum:
                assert torch.equal(buf, bufc) and int(init_t) == 1
        assert torch.equal(p, pc)
        r = read(rec)
        check_record(r, g.numpy(), scale, [(0, numel)], max_norm)
        coefs.append(float(r["coef"]))
        # float64 torch: clip_grad_norm_ + the optimiser's step on the same data
        pr.grad = (g.double() * scale)
        torch.nn.utils.clip_grad_norm_([pr], float(np.float32(max_norm)))
        topt.step()
        errs = {"p": rel_err(p, pr.detach())}
        if kind == "adam":
            st = topt.state[pr]
            errs["m"], errs["v"] = rel_err(m, st["exp_avg"]), rel_err(v, st["exp_avg_sq"])
        elif momentum:
            errs["buf"] = rel_err(buf, topt.state[pr]["momentum_buffer"])
        print("%s numel %d step %d coef %.6f: %s" % (tag, numel, i + 1, r["coef"], {k: "%.3g" % e for k, e in errs.items()}))
        for k, e in errs.items():
            assert e < (M_NUMEL1 if (k == "m" and numel == 1) else 1e-6), (k, e)
    assert sum(c < 1.0 for c in coefs) == 1 and sum(c == 1.0 for c in coefs) == 2, coefs


# ------------------------------------------------------------------------------------------------ 5. no clipping is no change
@gpu
@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("max_norm", [0.0, 1e30])
def test_no_clipping_changes_no_bit(dev, numel, max_norm):
    from pointcloududa_amd import kernels as K
    p0, grads = _inputs(numel)
    z = lambda: torch.zeros(numel, device=dev)
    pa, ma, va, pau, mau, vau = p0.to(dev), z(), z(), p0.to(dev), z(), z()
    ps, bs, psu, bsu = p0.to(dev), z(), p0.to(dev), z()
    step_t, step_u, init_t = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3))
    rec = K.guard_record(dev)
    for i, g in enumerate(grads):
        gd = g.to(dev)
        K.grad_norm(gd, [(0, numel)], 0.25, max_norm, True, rec)
        K.adam_step_guarded(pa, gd, ma, va, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], WD_ADAM, step_t, rec, True, 0.25)
        K.adam_step_dev(pau, gd, mau, vau, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], WD_ADAM, step_u, 0.25)
        K.sgd_step_guarded(ps, gd, bs, LR_SGD, 0.99, WD_SGD, init_t, True, rec, True, 0.25)
        K.sgd_step(psu, gd, bsu, LR_SGD, 0.99, WD_SGD, i == 0, 0.25)
        assert read(rec)["coef"] == 1.0
        assert torch.equal(pa, pau) and torch.equal(ma, mau) and torch.equal(va, vau) and int(step_t) == int(step_u) == i + 1
        assert torch.equal(ps, psu) and torch.equal(bs, bsu)


# ------------------------------------------------------------------------------------------------ 6. non-finite
# a 5003-element buffer; range 0 starts 1 past a 16-byte boundary (head 3, tail 3), range 1 starts 2 past one (head 2, tail 1)
NF_TOTAL, NF_RANGES = 5003, [(1, 2002), (2006, 2803)]
NF_SPAN = (1, 2006 + 2803)
PLACEMENTS = {
    "inf_last_of_last_range": ([2006 + 2803 - 1], np.inf),
    "nan_first": ([1], np.nan),
    "nan_in_scalar_tail": ([1 + 2002 - 2], np.nan),
    "overflow_of_finite_values": ([100, 101, 102, 103], 3e38),       # every element finite, the float32 norm is not
}


def _nf_grad(where=None, value=None, seed=7):
    g = np.random.default_rng(seed).normal(0, 1, NF_TOTAL).astype(np.float32)
    g[:NF_RANGES[0][0]] = 0
    g[NF_RANGES[0][0] + NF_RANGES[0][1]:NF_RANGES[1][0]] = 0          # (the gap: zero, so that one span can be updated)
    g[NF_SPAN[1]:] = 0
    if where is not None:
        g[where] = value
    return g


@gpu
@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_nonfinite_gradient_is_skipped(dev, place):
    from pointcloududa_amd import kernels as K
    where, value = PLACEMENTS[place]
    bad, good = torch.from_numpy(_nf_grad(where, value)).to(dev), torch.from_numpy(_nf_grad()).to(dev)
    lo, hi = NF_SPAN
    rng = np.random.default_rng(8)
    mk = lambda: torch.from_numpy(rng.normal(0, 1, NF_TOTAL).astype(np.float32)).to(dev)
    # Adam: state from "earlier steps" (count 5); SGD: a momentum buffer of junk that only the initialising step may overwrite
    p, m, v, ps, buf = mk(), mk(), mk().abs(), mk(), mk()
    step_t = torch.full((1,), 5, dtype=torch.int32, device=dev)
    init_t = torch.zeros(1, dtype=torch.int32, device=dev)
    rec = K.guard_record(dev)
    before = [t.clone() for t in (p, m, v, ps, buf)]

    def both(g):
        K.grad_norm(g, NF_RANGES, 1.0, 1.0, True, rec)
        K.adam_step_guarded(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], WD_ADAM,
                            step_t, rec, True)
        for i, (o, n) in enumerate(NF_RANGES):
            K.sgd_step_guarded(ps[o:o + n], g[o:o + n], buf[o:o + n], LR_SGD, 0.99, WD_SGD, init_t, i == len(NF_RANGES) - 1, rec, True)

    both(bad)
    r = read(rec)
    print(place, r)
    assert r["finite"] == 0 and not np.isfinite(r["norm"])
    check_record(r, bad.cpu().numpy(), 1.0, NF_RANGES, 1.0)
    for t, t0 in zip((p, m, v, ps, buf), before):
        assert torch.equal(t, t0)
    assert int(step_t) == 5 and int(init_t) == 0
    assert (r["skipped"], r["applied"], r["skip"]) == (1, 0, 1)
    # the next finite step applies; SGD initialises its momentum buffer on it
    pc, mc, vc, psc, bufc = [t.clone() for t in before]
    step_c = torch.full((1,), 5, dtype=torch.int32, device=dev)
    both(good)
    r = read(rec)
    assert (r["skipped"], r["applied"], r["skip"], r["finite"]) == (1, 1, 0, 1) and r["coef"] < 1.0
    pre = good * rec[1:2].view(torch.float32)
    K.adam_step_dev(pc[lo:hi], pre[lo:hi], mc[lo:hi], vc[lo:hi], ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], WD_ADAM, step_c)
    for o, n in NF_RANGES:
        K.sgd_step(psc[o:o + n], pre[o:o + n], bufc[o:o + n], LR_SGD, 0.99, WD_SGD, True)       # first_step: buf = gradient
    assert int(step_t) == 6 and int(init_t) == 1
    for t, tc in zip((p, m, v, ps, buf), (pc, mc, vc, psc, bufc)):
        assert torch.equal(t, tc)
    assert not torch.equal(p, before[0]) and not torch.equal(buf, before[4])


def _same_nan_and_values(got, want, what):
    got, want = got.double().cpu().numpy(), want.double().cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(np.isinf(got), np.isinf(want)), what
    ok = np.isfinite(want)
    if ok.any():
        err = np.abs(got[ok] - want[ok]).max() / max(1e-30, np.abs(want[ok]).max())
        assert err < 1e-6, (what, err)


@gpu
@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_nonfinite_gradient_propagates_as_in_torch_without_the_switch(dev, place):
    """skip_nonfinite off: nothing is special-cased -- clip_grad_norm_(error_if_nonfinite=False) followed by the step, in
    float32 on the CPU (where a sum of squares overflows as it does here), gives the same NaN positions and finite values"""
    from pointcloududa_amd import kernels as K
    where, value = PLACEMENTS[place]
    g = torch.from_numpy(_nf_grad(where, value))
    lo, hi = NF_SPAN
    rng = np.random.default_rng(9)
    p0 = torch.from_numpy(rng.normal(0, 1, NF_TOTAL).astype(np.float32))
    gd, rec = g.to(dev), K.guard_record(dev)
    for kind in ("adam", "sgd"):
        p, a, b = p0.to(dev), torch.zeros(NF_TOTAL, device=dev), torch.zeros(NF_TOTAL, device=dev)
        step_t, init_t = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
        K.grad_norm(gd, NF_RANGES, 1.0, 1.0, False, rec)
        assert read(rec)["skip"] == 0 and read(rec)["finite"] == 0
        pr = p0[lo:hi].clone().requires_grad_(True)
        pr.grad = g[lo:hi].clone()
        torch.nn.utils.clip_grad_norm_([pr], 1.0)
        if kind == "adam":
            K.adam_step_guarded(p[lo:hi], gd[lo:hi], a[lo:hi], b[lo:hi], ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], 0.0,
                                step_t, rec, False)
            topt = torch.optim.Adam([pr], lr=ADAM["lr"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["eps"])
            topt.step()
            assert int(step_t) == 1
            _same_nan_and_values(a[lo:hi], topt.state[pr]["exp_avg"], (kind, "m"))
            _same_nan_and_values(b[lo:hi], topt.state[pr]["exp_avg_sq"], (kind, "v"))
        else:
            K.sgd_step_guarded(p[lo:hi], gd[lo:hi], a[lo:hi], LR_SGD, 0.99, WD_SGD, init_t, True, rec, False)
            topt = torch.optim.SGD([pr], lr=LR_SGD, momentum=0.99, weight_decay=WD_SGD)
            topt.step()
            assert int(init_t) == 1
            _same_nan_and_values(a[lo:hi], topt.state[pr]["momentum_buffer"], (kind, "buf"))
        _same_nan_and_values(p[lo:hi], pr.detach(), (kind, "p"))
        assert torch.equal(p[:lo].cpu(), p0[:lo]) and torch.equal(p[hi:].cpu(), p0[hi:])
    assert read(rec)["applied"] == 2 and read(rec)["skipped"] == 0


# ------------------------------------------------------------------------------------------------ 7. graph replay
def _disc(dev, seed):
    from pointcloududa_amd.networks import UncertaintyDiscriminator
    torch.manual_seed(seed)
    return UncertaintyDiscriminator(in_channel=2).to(dev).train()


def _opt_state(opt):
    return [t for t in (opt.p, getattr(opt, "m", None), getattr(opt, "v", None), getattr(opt, "buf", None),
                        getattr(opt, "step_t", None), getattr(opt, "init_t", None), opt.guard) if t is not None]


@gpu
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_guarded_step_replays_from_a_captured_graph(dev, kind):
    """one guarded step() captured once (a linear chain of launches), replayed three times over a rewritten gradient buffer:
    the decision is taken from device memory at every replay.  Adam: clipped, unclipped, inf; SGD: inf FIRST (a skipped
    first step must not consume the momentum buffer's initialisation), then clipped, then unclipped."""
    from pointcloududa_amd.optim import FusedAdam, FusedSGD
    mk = (lambda m: FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, skip_nonfinite=True)) if kind == "adam" else \
         (lambda m: FusedSGD(m, lr=2.5e-2, momentum=0.99, weight_decay=0.0005, max_grad_norm=1.0, skip_nonfinite=True))
    og, oe = mk(_disc(dev, 11)), mk(_disc(dev, 11))
    assert torch.equal(og.p, oe.p) and og.guard is not None
    n = og.g.numel()
    gen = torch.Generator().manual_seed(12)
    base = torch.randn(n, generator=gen)
    clipped = (base * (4.0 / float(base.norm()))).to(dev)                 # norm 4: coef 0.25
    unclipped = (torch.randn(n, generator=gen) * (0.5 / n ** 0.5)).to(dev)     # norm ~0.5
    bad = unclipped.clone()
    bad[n - 1] = float("inf")
    seq = [clipped, unclipped, bad] if kind == "adam" else [bad, clipped, unclipped]
    # warm-up outside the capture (every lazily created object exists afterwards), then the state is put back
    saved = [t.clone() for t in _opt_state(og)]
    og.g.copy_(unclipped)
    og.step()
    torch.cuda.synchronize()
    for t, s in zip(_opt_state(og), saved):
        t.copy_(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    for t, s in zip(_opt_state(og), saved):      # (capture executes nothing; this only states it)
        assert torch.equal(t, s)
    coefs = []
    for g in seq:
        og.g.copy_(g)
        graph.replay()
        oe.g.copy_(g)
        oe.step()
        coefs.append(float(og.clip_coef))
        for a, b in zip(_opt_state(og), _opt_state(oe)):
            assert torch.equal(a, b)
    print(kind, "coefficients over the replays:", coefs)
    assert int(og.skipped) == 1 and read(og.guard)["applied"] == 2
    if kind == "adam":
        assert int(og.step_t) == 2 and coefs[0] < 0.26 and coefs[1] == 1.0
    else:
        assert int(og.init_t) == 1 and coefs[1] < 0.26 and coefs[2] == 1.0
        # the first applied step initialised the buffer: buf = gradient + weight decay, not momentum * 0 + ...; and the
        # exported state holds it
        assert len(og.torch_state_dict()["state"]) > 0


@gpu
def test_sgd_state_export_reads_the_device_flag(dev):
    """a guarded FusedSGD whose only steps were skipped exports no momentum buffer (torch.optim.SGD holds none before its
    first step); grad_norms() returns the named groups' sums from the same launch"""
    from pointcloududa_amd.optim import FusedSGD
    opt = FusedSGD(_disc(dev, 13), skip_nonfinite=True)
    opt.g.fill_(float("nan"))
    opt.step()
    assert int(opt.skipped) == 1 and opt.torch_state_dict()["state"] == {}
    opt.g.normal_()
    opt.step()
    assert len(opt.torch_state_dict()["state"]) == len(list(opt.module.parameters()))
    sums = opt.grad_norms(["conv1.", "conv5.", "conv"]).cpu().numpy()
    g = opt.g.double().cpu().numpy()
    sl = dict(zip([k for k, _ in opt.module.named_parameters()], opt._slices()))
    want = lambda pre: sum(float((g[o:o + n] ** 2).sum()) for k, (o, n, _) in sl.items() if k.startswith(pre))
    for got, pre in zip(sums, ("conv1.", "conv5.", "conv")):
        assert abs(got - want(pre)) <= 1e-12 * want(pre), (pre, got, want(pre))
    assert abs(float(opt.grad_norm) - want("conv") ** 0.5) <= 2e-7 * want("conv") ** 0.5
    with pytest.raises(ValueError):
        opt.grad_norms(["conv1.weight"])


# ------------------------------------------------------------------------------------------------ 8. argument checks (CPU)
def test_argument_checks_return_before_any_launch():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    fake = 0x10000                                                       # never dereferenced: every check is on the host
    launches = lib.pcuda_launch_count(0)
    ranges = (ctypes.c_longlong * 34)(*([0, 8] * 17))
    ws = _lib.GRAD_NORM_WORKSPACE_BYTES
    norm = lambda g, rg, n, rec, w, wb=ws: lib.pcuda_grad_norm(g, rg, n, 1.0, 1.0, 1, rec, None, w, wb, None)
    assert norm(None, ranges, 1, fake, fake) == -1 and b"grad_norm" in lib.pcuda_last_error()
    assert norm(fake, None, 1, fake, fake) == -1
    assert norm(fake, ranges, 1, None, fake) == -1
    assert norm(fake, ranges, 1, fake, None) == -1
    assert norm(fake, ranges, 0, fake, fake) == -1
    assert norm(fake, ranges, 17, fake, fake) == -1                       # more than 16 ranges
    neg = (ctypes.c_longlong * 4)(0, 8, 8, -1)
    assert norm(fake, neg, 2, fake, fake) == -1                           # negative numel
    neg = (ctypes.c_longlong * 2)(-4, 8)
    assert norm(fake, neg, 1, fake, fake) == -1                           # negative offset
    assert norm(fake, ranges, 1, fake, fake, ws - 8) == -4                # workspace too small
    assert norm(fake + 2, ranges, 1, fake, fake) == -4                    # misaligned gradient
    a = lambda p, g, m, v, n, st, rec: lib.pcuda_adam_step_guarded(p, g, m, v, n, 1e-3, 0.9, 0.99, 1e-8, 0.0, st, 1.0, rec, 1, None)
    for bad in ((None, fake, fake, fake, 8, fake, fake), (fake, None, fake, fake, 8, fake, fake), (fake, fake, None, fake, 8, fake, fake),
                (fake, fake, fake, None, 8, fake, fake), (fake, fake, fake, fake, 0, fake, fake), (fake, fake, fake, fake, -8, fake, fake),
                (fake, fake, fake, fake, 8, None, fake), (fake, fake, fake, fake, 8, fake, None)):
        assert a(*bad) == -1 and b"adam_step_guarded" in lib.pcuda_last_error()
    s = lambda p, g, mom, n, momentum, init, rec: lib.pcuda_sgd_step_guarded(p, g, mom, n, 1e-3, momentum, 0.0, init, 1, 1.0, rec, 1, None)
    for bad in ((None, fake, fake, 8, 0.9, fake, fake), (fake, None, fake, 8, 0.9, fake, fake), (fake, fake, None, 8, 0.9, fake, fake),
                (fake, fake, fake, 8, 0.9, None, fake), (fake, fake, fake, 8, 0.9, fake, None), (fake, fake, fake, -1, 0.9, fake, fake),
                (fake, fake, None, 8, 0.0, None, None)):
        assert s(*bad) == -1 and b"sgd_step_guarded" in lib.pcuda_last_error()
    assert lib.pcuda_launch_count(0) == launches
    assert lib.pcuda_version() == _lib.PCUDA_ABI_VERSION == 5            # the three entry points are an additive change
