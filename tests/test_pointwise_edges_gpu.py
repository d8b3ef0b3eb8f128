"""pointwise.hip and optim.hip at the branches test_pointwise_gpu.py never takes, against the float64 statements of
tests/fp64_refs.py (which tests/test_fp64_refs.py checks against torch autograd on the CPU).

case -> branch
  bn (1800,2,5)                 tile_pair_sum: 1800 tiles, lanes 0..7 take the 8-deep unrolled trip, the rest the tail; scalar kernels
  bn (3900,1,4)                 tile_pair_sum: two unrolled trips (lanes 0..59) + tail; float4 kernels
  bn (1,3,2048|2049|2052)       a plane that ends at a PCH = 2048 tile, one element past it (scalar), four past it (float4)
  bn (2,3,4100)                 three tiles per plane, ragged last tile, float4
  bn (2,1,1), (1,1,1)           count 2 and count 1 (var = 0, unbiased = var)
  bn (3,5,33,33)                odd plane, scalar kernels
  ... x post_relu x dy2 x accumulate    the `+=` of dgamma / dbeta (bn_bwd_finalize_kernel), the second gradient source
  layout slice64 / slice30      channel slice of a larger tensor: float4 kernels with foreign strides / scalar kernels
  layout pad65                  hw % 4 == 0 but plane strides 65: vec_ok refuses the strides -> scalar kernels
  layout off4                   hw % 4 == 0, base pointer 4 bytes past 16-byte alignment -> scalar kernels
  frozen                        count < 0 in bn_bwd_finalize_kernel (fixed affine), bn_backward and bn_backward_pooled
  bn_apply fma on/off           bn_apply_kernel<VEC, FMA>, bit patterns; relu on/off; float4 and scalar
  pooled (1,1,2,2) (2,3,6,4)    pool_load<4>; (2,3,6,6) and the odd-stride g: pool_load<1>
  maxpool grid                  ties in every window position, negative scales, pooled planes of 2047 / 2048 / 2049 elements
  *_bwd accumulate=1            pcuda_maxpool2_bwd / pcuda_upsample2_bwd `+=` (C ABI only)
  upsample2_bwd bnred           upsample2_bwd_kernel<true> partials, one and two tiles, fed to bn_backward(red=...)
  channel_sum accumulate        channel_sum_final_kernel `+=` at the tile borders
  add_n / mul 1048576 + 3       grid-stride loop past the 4096-block cap
  optimisers 2097152 + 3        grid-stride loop past the 8192-block cap; weight decay; adam_step_dev; momentum 0; grad_scale

Sign decisions (a > 0, a * scale + shift > 0): inputs whose float64 gate lies within 1e-3 of zero are moved to +-1e-2 before
either side sees them (fp64_refs.clear_gates), so every element is compared.

Bounds (against float64): 2e-5 BatchNorm forward, 5e-5 BatchNorm backward, 1e-5 running statistics / channel sums, 1e-6
element-wise operations and optimiser steps, copies / selections / max values bit-exact.

count 1: the variance of one value is 0, so y = beta and dz = 0 exactly; the kernels state that by construction
(scale = 0, shift = beta; zero backward coefficients) and the case is held to the same bounds as every other.

count 2: the input gradient of a training BatchNorm is eps / (var + eps) ~ 1e-5 times the terms it is the difference of,
which float32 does not resolve to 5e-5 of the result in general.  At (2,1,1) without the relu the kernel still does; with it
it does not, and there the bound on dz is four times the error of float32 F.batch_norm on the CPU against float64 on the same inputs (DZ_COUNT2, both
figures beside it).  y, the statistics, dgamma, dbeta, and dz without the relu keep the bounds above.

Adam's first moment with ONE element: beta1 * m + (1 - beta1) * g cancels at the second step of the numel = 1 case, and
nothing else sets the scale of max |ref|.  Its bound there is four times the error of float32 torch.optim.Adam (M_NUMEL1,
both figures beside it); every other numel, and every other quantity at numel = 1, keeps 1e-6.
"""
import functools

import numpy as np
import pytest
import torch

import fp64_refs as R
from conftest import rel_err
from layout_helpers import place_view as _place

pytestmark = pytest.mark.gpu

SLOPE = 0.2
BN_SHAPES = [(1800, 2, 5), (3900, 1, 4), (1, 3, 2048), (1, 3, 2049), (1, 3, 2052), (2, 3, 4100), (2, 1, 1), (1, 1, 1),
             (3, 5, 33, 33)]


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


def _rand(rng, *shape, scale=1.0, loc=0.0):
    return torch.from_numpy(rng.normal(loc, scale, shape).astype(np.float32))


def _params(rng, c):
    gamma = _rand(rng, c) * 0.2 + 1
    beta = torch.from_numpy(((0.05 + 0.2 * np.abs(rng.normal(0, 1, c))) * rng.choice([-1.0, 1.0], c)).astype(np.float32))
    return gamma, beta, _rand(rng, c) * 0.1, torch.rand(c, generator=torch.Generator().manual_seed(c)) + 0.5


def _prefill(c, lo=0.5):
    return torch.tensor([(lo + 0.25 * i) * (-1) ** i for i in range(c)], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _bn_case(shape, post_relu):
    """inputs (gates cleared) and the float64 forward of one BatchNorm case"""
    rng = np.random.default_rng(100 * len(shape) + sum(shape) + int(post_relu))
    c = shape[1]
    gamma, beta, rm0, rv0 = _params(rng, c)
    a = _rand(rng, *shape, loc=0.3)
    a = R.clear_gates(a, R.gate_bn(gamma, beta) if post_relu else R.gate_identity)
    gy, gy2 = _rand(rng, *shape), _rand(rng, *shape)
    fwd = R.bn_train_forward(a, gamma, beta, rm0, rv0, relu=post_relu)
    return dict(a=a, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, gy=gy, gy2=gy2, fwd=fwd)


@functools.lru_cache(maxsize=None)
def _bn_bwd_ref(shape, post_relu, two):
    cs = _bn_case(shape, post_relu)
    g = cs["gy"].double() + cs["gy2"].double() if two else cs["gy"]
    f = cs["fwd"]
    dz, dg, db = R.bn_backward(cs["a"], g, cs["gamma"], f["mean"], f["invstd"], cs["beta"], post_relu, SLOPE)
    return dz, dg, db


# (2,1,1): dz = eps / (var + eps) ~ 1e-5 of its terms (module docstring).  Error of dz against float64, float32
# F.batch_norm (+ relu) with autograd on the CPU next to the kernel, per (post_relu, two gradient sources):
#                     float32 CPU    kernel
#   (False, False)    7.28e-5        3.84e-5      within the 5e-5 of every other shape: kept
#   (False, True)     8.79e-5        4.63e-5      likewise
#   (True, False)     3.52e-3        4.86e-3      bound = 4 x the float32 CPU figure
#   (True, True)      7.34e-3        8.67e-3      bound = 4 x the float32 CPU figure
DZ_COUNT2 = {(False, False): 5e-5, (False, True): 5e-5, (True, False): 4 * 3.52e-3, (True, True): 4 * 7.34e-3}


def _run_bn(K, dev, cs, post_relu, two, accumulate, layout="dense"):
    c = cs["a"].shape[1]
    a = _place(cs["a"], dev, layout)
    gamma, beta = cs["gamma"].to(dev), cs["beta"].to(dev)
    rm, rv = cs["rm0"].to(dev), cs["rv0"].to(dev)
    part, nt, cnt = K.bn_stats(a)
    st = K.bn_finalize(part, nt, cnt, gamma, beta, rm, rv)
    y = K.bn_apply(a, st, relu=post_relu)
    pre_g, pre_b = _prefill(c), _prefill(c, 0.75)
    dg, db = (pre_g.to(dev), pre_b.to(dev)) if accumulate else (torch.zeros(c, device=dev), torch.zeros(c, device=dev))
    dz = K.bn_backward(_place(cs["gy"], dev, layout), a, st, gamma, dg, db, dy2=_place(cs["gy2"], dev, layout) if two else None,
                       post_relu=post_relu, act_slope=SLOPE, accumulate=accumulate)
    return dict(nt=nt, cnt=cnt, st=st, y=y, rm=rm, rv=rv, dz=dz, dg=dg, db=db, pre_g=pre_g if accumulate else 0.0,
                pre_b=pre_b if accumulate else 0.0)


def _check_bn(out, cs, ref_bwd, dz_bound=5e-5):
    f = cs["fwd"]
    dz, dg, db = ref_bwd
    assert out["cnt"] == f["count"]
    print("bn: mean %.3g invstd %.3g y %.3g rm %.3g rv %.3g dz %.3g dg %.3g db %.3g" % (
        rel_err(out["st"].mean, f["mean"]), rel_err(out["st"].invstd, f["invstd"]), rel_err(out["y"], f["y"]),
        rel_err(out["rm"], f["running_mean"]), rel_err(out["rv"], f["running_var"]), rel_err(out["dz"], dz),
        rel_err(out["dg"], dg + out["pre_g"]), rel_err(out["db"], db + out["pre_b"])))
    assert rel_err(out["st"].mean, f["mean"]) < 1e-5 and rel_err(out["st"].invstd, f["invstd"]) < 1e-5
    assert rel_err(out["y"], f["y"]) < 2e-5
    assert rel_err(out["rm"], f["running_mean"]) < 1e-5 and rel_err(out["rv"], f["running_var"]) < 1e-5
    assert rel_err(out["dz"], dz) < dz_bound
    assert rel_err(out["dg"], dg + out["pre_g"]) < 5e-5 and rel_err(out["db"], db + out["pre_b"]) < 5e-5


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("post_relu", [False, True])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=_ids(BN_SHAPES))
def test_batchnorm_against_float64(dev, shape, post_relu, two, accumulate):
    from pointcloududa_amd import kernels as K
    cs = _bn_case(shape, post_relu)
    out = _run_bn(K, dev, cs, post_relu, two, accumulate)
    hw = int(np.prod(shape[2:]))
    assert out["nt"] == shape[0] * ((hw + 2047) // 2048)           # (1800 and 3900 tiles for the first two shapes)
    _check_bn(out, cs, _bn_bwd_ref(shape, post_relu, two), DZ_COUNT2[post_relu, two] if shape == (2, 1, 1) else 5e-5)


LAYOUTS = [("slice", (3, 4, 64)), ("slice", (3, 4, 5, 6)), ("pad", (3, 4, 64)), ("off4", (3, 4, 8, 8))]


@pytest.mark.parametrize("post_relu", [False, True])
@pytest.mark.parametrize("layout,shape", LAYOUTS, ids=["slice64", "slice30", "pad65", "off4"])
def test_batchnorm_on_strided_and_misaligned_inputs(dev, layout, shape, post_relu):
    from pointcloududa_amd import kernels as K
    cs = _bn_case(shape, post_relu)
    out = _run_bn(K, dev, cs, post_relu, True, True, layout)
    _check_bn(out, cs, _bn_bwd_ref(shape, post_relu, True))


def _hand_state(K, dev, gamma, beta, rm, rv, count):
    """BNState of an eval-mode BatchNorm: the running statistics (float32 values; the reference reads the same ones)"""
    invstd = (1.0 / torch.sqrt(rv.double() + R.f32(1e-5))).float()
    scale = (gamma.double() * invstd.double()).float()
    shift = (beta.double() - rm.double() * scale.double()).float()
    st = K.BNState()
    st.mean, st.invstd, st.scale, st.shift, st.count = rm.to(dev), invstd.to(dev), scale.to(dev), shift.to(dev), count
    return st, invstd, scale, shift


@pytest.mark.parametrize("post_relu", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (2, 3, 5, 7), (1, 2, 2049)], ids=_ids([(2, 3, 8, 8), (2, 3, 5, 7), (1, 2, 2049)]))
def test_frozen_batchnorm_backward(dev, shape, post_relu):
    """eval-mode BatchNorm: dz = gamma * invstd * g (times the activation's slope), dgamma / dbeta the same sums"""
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(7 + sum(shape))
    c = shape[1]
    gamma, beta, rm, rv = _params(rng, c)
    st, invstd, scale, shift = _hand_state(K, dev, gamma, beta, rm, rv, shape[0] * int(np.prod(shape[2:])))
    a = R.clear_gates(_rand(rng, *shape, loc=0.3), R.gate_affine(scale, shift) if post_relu else R.gate_identity)
    gy, gy2 = _rand(rng, *shape), _rand(rng, *shape)
    # (the gate of the kernel is a * scale + shift with the float32 scale / shift: the reference's beta is the one they imply)
    beta_eff = shift.double() + rm.double() * scale.double()
    dz_r, dg_r, db_r = R.bn_backward(a, gy.double() + gy2.double(), gamma, rm, invstd, beta_eff, post_relu, SLOPE, frozen=True)
    pre_g, pre_b = _prefill(c), _prefill(c, 0.75)
    dg, db = pre_g.to(dev), pre_b.to(dev)
    dz = K.bn_backward(gy.to(dev), a.to(dev), st, gamma.to(dev), dg, db, dy2=gy2.to(dev), post_relu=post_relu, act_slope=SLOPE,
                       accumulate=True, frozen=True)
    print("frozen: dz %.3g dg %.3g db %.3g" % (rel_err(dz, dz_r), rel_err(dg, dg_r + pre_g), rel_err(db, db_r + pre_b)))
    assert rel_err(dz, dz_r) < 5e-5
    assert rel_err(dg, dg_r + pre_g) < 5e-5 and rel_err(db, db_r + pre_b) < 5e-5


def _pooled_inputs(rng, dev, shape, two, skip, odd_g=False):
    n, c, h, w = shape
    a = R.clear_gates(_rand(rng, *shape, loc=0.3), R.gate_identity)
    idx = torch.from_numpy(rng.integers(0, 4, (n, c, h // 2, w // 2)).astype(np.uint8))
    g = _rand(rng, n, c, h // 2, w // 2)
    g2 = _rand(rng, n, c, h // 2, w // 2) if two else None
    dy = _rand(rng, *shape) if skip else None
    if odd_g:        # planes of (h/2)*(w/2) elements, plane stride one more: odd when the plane is even
        gd = _place(g.view(n, c, -1), dev, "pad").unflatten(2, (h // 2, w // 2))
        assert c == 1 or gd.stride(1) == (h // 2) * (w // 2) + 1
    else:
        gd = g.to(dev)
    full = R.maxpool2_scatter(g.double() + g2.double() if two else g, idx, h, w)
    if skip:
        full = full + dy.double()
    return a, idx, g, g2, dy, gd, full


POOLED = [(1, 1, 2, 2), (2, 3, 6, 4), (2, 3, 6, 6)]


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("two,skip,odd_g", [(False, False, False), (True, False, False), (False, True, False), (True, True, False),
                                            (True, True, True)])
@pytest.mark.parametrize("shape", POOLED, ids=_ids(POOLED))
def test_pooled_gradient_source_against_the_definition(dev, shape, two, skip, odd_g, frozen):
    """bn_backward_pooled / lrelu_bwd_pooled == the float64 backward fed with the max-pool's scatter (+ the full-resolution
    share); training and frozen statistics"""
    from pointcloududa_amd import kernels as K
    n, c, h, w = shape
    rng = np.random.default_rng(11 + h * w + 2 * two + skip)
    a, idx, g, g2, dy, gd, full = _pooled_inputs(rng, dev, shape, two, skip, odd_g)
    gamma, beta, rm, rv = _params(rng, c)
    ad = a.to(dev)
    g2d, dyd = (None if g2 is None else g2.to(dev)), (None if dy is None else dy.to(dev))
    got = K.lrelu_bwd_pooled(gd, idx.to(dev), ad, SLOPE, g2=g2d, dy=dyd)
    want = full * torch.where(a > 0, 1.0, R.f32(SLOPE)).double()
    assert rel_err(got, want) < 1e-6
    if frozen:
        st, invstd, _, _ = _hand_state(K, dev, gamma, beta, rm, rv, n * h * w)
        mean = rm
    else:
        part, nt, cnt = K.bn_stats(ad)
        st = K.bn_finalize(part, nt, cnt, gamma.to(dev), beta.to(dev), None, None)
        f = R.bn_train_forward(a, gamma, beta, rm, rv)
        mean, invstd = f["mean"], f["invstd"]
    dz_r, dg_r, db_r = R.bn_backward(a, full, gamma, mean, invstd, None, False, SLOPE, frozen=frozen)
    pre_g, pre_b = _prefill(c), _prefill(c, 0.75)
    dg, db = pre_g.to(dev), pre_b.to(dev)
    dz = K.bn_backward_pooled(gd, idx.to(dev), ad, st, gamma.to(dev), dg, db, g2=g2d, dy=dyd, act_slope=SLOPE, accumulate=True,
                              frozen=frozen)
    print("pooled: dz %.3g dg %.3g db %.3g" % (rel_err(dz, dz_r), rel_err(dg, dg_r + pre_g), rel_err(db, db_r + pre_b)))
    assert rel_err(dz, dz_r) < 5e-5
    assert rel_err(dg, dg_r + pre_g) < 5e-5 and rel_err(db, db_r + pre_b) < 5e-5


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 4100), (1, 3, 2049)], ids=["float4", "scalar"])
def test_bn_apply_rounds_twice_without_fma_and_once_with(dev, shape, relu):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(21 + shape[2])
    c = shape[1]
    a = _rand(rng, *shape)
    st = K.BNState()
    sc, sf = _rand(rng, c) * 0.5 + 1, _rand(rng, c)
    st.scale, st.shift, st.mean, st.invstd, st.count = sc.to(dev), sf.to(dev), None, None, 0
    an, scn, sfn = a.numpy(), sc.numpy()[None, :, None], sf.numpy()[None, :, None]
    two = (an * scn).astype(np.float32) + sfn                                   # float32(float32(a * sc) + sf)
    assert two.dtype == np.float32
    one = (an.astype(np.float64) * scn.astype(np.float64) + sfn.astype(np.float64)).astype(np.float32)
    if relu:
        two, one = np.where(two > 0, two, np.float32(0)), np.where(one > 0, one, np.float32(0))
    y_mul = K.bn_apply(a.to(dev), st, relu=relu, fma=False).cpu().numpy()
    y_fma = K.bn_apply(a.to(dev), st, relu=relu, fma=True).cpu().numpy()
    assert np.array_equal(_bits(y_mul), _bits(two))
    share = lambda y: float(np.mean(_bits(y) != _bits(one)))
    print("bn_apply: fma differs from the once-rounded value in %.3g, multiply-add in %.3g of the elements" % (share(y_fma), share(y_mul)))
    assert share(y_fma) <= 1e-4                  # (the float64 sum is itself rounded: double rounding)
    assert share(y_mul) > 1e-4                   # the two paths cannot be swapped unnoticed


def _grid_input(rng, n, c, h, w):
    """x in multiples of 1/8 within +-64, scale in {-2, -.5, .5, 1, 2}, shift in multiples of .25: x * scale + shift is exact
    in float32.  Windows (0, 0..10) of every plane carry a tie over every subset of >= 2 window positions."""
    x = rng.integers(-512, 513, (n, c, h, w)).astype(np.float32) / 8
    scale = np.array([-2.0, -0.5, 0.5, 1.0, 2.0], dtype=np.float32)[np.arange(c) % 5]
    shift = (rng.integers(-16, 17, c) * 0.25).astype(np.float32)
    subsets = [s for s in range(1, 16) if bin(s).count("1") >= 2]
    for j, s in enumerate(subsets):
        for ch in range(c):
            for k in range(4):
                x[:, ch, k >> 1, 2 * j + (k & 1)] = 3.0 if (s >> k) & 1 else 3.0 - 8.0 * np.sign(scale[ch])
    return torch.from_numpy(x), torch.from_numpy(scale), torch.from_numpy(shift), subsets


PLANES = [(46, 178), (64, 128), (6, 1366)]          # pooled planes of 23*89 = 2047, 32*64 = 2048, 3*683 = 2049 elements


@pytest.mark.parametrize("h,w", PLANES, ids=["2047", "2048", "2049"])
def test_maxpool_values_indices_and_scatter_are_exact(dev, h, w):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.kernels import TA
    rng = np.random.default_rng(31 + h)
    n, c = 2, 5
    x, scale, shift, subsets = _grid_input(rng, n, c, h, w)
    y_r, idx_r = R.maxpool2(x, scale, shift)
    for j, s in enumerate(subsets):              # the plant: the first tied position wins
        assert bool((idx_r[:, :, 0, j] == min(k for k in range(4) if (s >> k) & 1)).all())
    y, idx = K.maxpool2_fwd(TA(x.to(dev), scale.to(dev), shift.to(dev)))
    assert torch.equal(y.cpu().double(), y_r) and torch.equal(idx.cpu(), idx_r)
    y0, idx0 = K.maxpool2_fwd(x.to(dev))                                         # no affine
    y0_r, idx0_r = R.maxpool2(x)
    assert torch.equal(y0.cpu().double(), y0_r) and torch.equal(idx0.cpu(), idx0_r)
    g1, g2 = _rand(rng, n, c, h // 2, w // 2), _rand(rng, n, c, h // 2, w // 2)
    dx = K.maxpool2_bwd(g1.to(dev), idx, h, w)
    assert torch.equal(dx.cpu().double(), R.maxpool2_scatter(g1, idx_r, h, w))   # a selection: exact
    # accumulate = 1 (C ABI only) onto a pre-filled dx, two gradient sources
    pre = _rand(rng, n, c, h, w)
    dxa, g1d, g2d = pre.to(dev), g1.to(dev), g2.to(dev)
    L.check(L.lib().pcuda_maxpool2_bwd(g1d.data_ptr(), g1d.stride(0), g1d.stride(1), g2d.data_ptr(), g2d.stride(0), g2d.stride(1),
                                       idx.data_ptr(), dxa.data_ptr(), dxa.stride(0), dxa.stride(1), 1, n, c, h, w,
                                       K._stream()), "maxpool2_bwd")
    assert rel_err(dxa, pre.double() + R.maxpool2_scatter(g1.double() + g2.double(), idx_r, h, w)) < 1e-6


@pytest.mark.parametrize("h,w", [(23, 89), (32, 64), (3, 683)], ids=["2047", "2048", "2049"])
def test_upsample_fold_accumulates(dev, h, w):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(41 + h)
    n, c = 2, 3
    dy, pre = _rand(rng, n, c, 2 * h, 2 * w), _rand(rng, n, c, h, w)
    assert rel_err(K.upsample2_bwd(dy.to(dev)), R.fold2(dy)) < 1e-6
    dyd, dx = dy.to(dev), pre.to(dev)
    L.check(L.lib().pcuda_upsample2_bwd(dyd.data_ptr(), dyd.stride(0), dyd.stride(1), dx.data_ptr(), dx.stride(0), dx.stride(1), 1,
                                        n, c, h, w, K._stream()), "upsample2_bwd")
    assert rel_err(dx, pre.double() + R.fold2(dy)) < 1e-6


@pytest.mark.parametrize("shape", [(2, 3, 8, 10), (1, 2, 46, 46)], ids=_ids([(2, 3, 8, 10), (1, 2, 46, 46)]))
def test_upsample_fold_carries_the_batchnorm_reduce(dev, shape):
    from pointcloududa_amd import kernels as K
    n, c, h, w = shape
    rng = np.random.default_rng(51 + h)
    a = R.clear_gates(_rand(rng, *shape, loc=0.3), R.gate_identity)
    dy = _rand(rng, n, c, 2 * h, 2 * w)
    gamma, beta, rm, rv = _params(rng, c)
    ad = a.to(dev)
    part, nt, cnt = K.bn_stats(ad)
    st = K.bn_finalize(part, nt, cnt, gamma.to(dev), beta.to(dev), None, None)
    dx, red = K.upsample2_bwd(dy.to(dev), bnred=(ad, st))
    assert red is not None and red[1] == n * ((h * w + 2047) // 2048) and red[0].shape == (red[1], c, 2)
    g = R.fold2(dy)
    assert rel_err(dx, g) < 1e-6
    xhat = (a.double() - st.mean.double().cpu().view(1, -1, 1, 1)) * st.invstd.double().cpu().view(1, -1, 1, 1)
    sums = red[0].double().sum(0).cpu()
    print("bnred: S1 %.3g S2 %.3g" % (rel_err(sums[:, 0], g.sum((0, 2, 3))), rel_err(sums[:, 1], (g * xhat).sum((0, 2, 3)))))
    assert rel_err(sums[:, 0], g.sum((0, 2, 3))) < 5e-5 and rel_err(sums[:, 1], (g * xhat).sum((0, 2, 3))) < 5e-5
    f = R.bn_train_forward(a, gamma, beta, rm, rv)
    dz_r, dg_r, db_r = R.bn_backward(a, g, gamma, f["mean"], f["invstd"], None, False, SLOPE)
    dg, db = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    dz = K.bn_backward(dx, ad, st, gamma.to(dev), dg, db, act_slope=SLOPE, accumulate=False, red=red)
    assert rel_err(dz, dz_r) < 5e-5 and rel_err(dg, dg_r) < 5e-5 and rel_err(db, db_r) < 5e-5


TILE_BORDERS = [(1, 3, 2048), (1, 3, 2049), (1, 3, 2052), (2, 3, 4100)]


@pytest.mark.parametrize("shape", TILE_BORDERS, ids=_ids(TILE_BORDERS))
def test_channel_sum_accumulates(dev, shape):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(61 + shape[2])
    x, pre = _rand(rng, *shape), _prefill(shape[1])
    db = pre.to(dev)
    K.channel_sum(x.to(dev), db)                                  # accumulate=True is the default
    assert rel_err(db, pre.double() + R.channel_sum(x)) < 1e-5
    K.channel_sum(x.to(dev), db, accumulate=False)
    assert rel_err(db, R.channel_sum(x)) < 1e-5


@pytest.mark.parametrize("numel", [1, 255, 257, 1048576 + 3])
def test_add_and_mul(dev, numel):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(71)
    ts = [_rand(rng, numel) for _ in range(4)]
    td = [t.to(dev) for t in ts]
    for k in (2, 3, 4):
        assert rel_err(K.add_n(td[:k]), sum(t.double() for t in ts[:k])) < 1e-6
    assert rel_err(K.mul(td[0], td[1]), ts[0].double() * ts[1].double()) < 1e-6


NUMELS = [1, 257, 5000, 2097152 + 3]


# numel 1, Adam's first moment: beta1 * m + (1 - beta1) * g cancels at the second step (module docstring).  Largest error
# over the three steps against float64: float32 torch.optim.Adam on the CPU 1.49e-6, the kernel 1.54e-6; the bound is four
# times the former.
M_NUMEL1 = 4 * 1.49e-6


ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8)


@functools.lru_cache(maxsize=None)
def _opt_inputs(numel):
    rng = np.random.default_rng(81)
    return _rand(rng, numel), tuple(_rand(rng, numel) for _ in range(3))


@pytest.mark.parametrize("numel", NUMELS)
def test_adam_with_weight_decay_and_device_step_count(dev, numel):
    from pointcloududa_amd import kernels as K
    p0, grads = _opt_inputs(numel)
    wd = 0.01
    z = lambda: torch.zeros(numel, device=dev)
    p, m, v = p0.to(dev), z(), z()
    pd, md, vd, step_t = p0.to(dev), z(), z(), torch.zeros(1, dtype=torch.int32, device=dev)
    pr, mr, vr = p0, torch.zeros(numel), torch.zeros(numel)
    for i, g in enumerate(grads):
        K.adam_step(p, g.to(dev), m, v, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], wd, i + 1)
        K.adam_step_dev(pd, g.to(dev), md, vd, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], wd, step_t)
        pr, mr, vr = R.adam_step(pr, g, mr, vr, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], wd, i + 1)
        print("adam step %d: p %.3g m %.3g v %.3g" % (i + 1, rel_err(p, pr), rel_err(m, mr), rel_err(v, vr)))
        assert rel_err(p, pr) < 1e-6 and rel_err(m, mr) < (M_NUMEL1 if numel == 1 else 1e-6) and rel_err(v, vr) < 1e-6
        assert torch.equal(pd, p) and torch.equal(md, m) and torch.equal(vd, v)
        assert rel_err(pd, pr) < 1e-6
    assert int(step_t) == 3


@pytest.mark.parametrize("numel", NUMELS)
def test_sgd_without_momentum_and_with_grad_scale(dev, numel):
    from pointcloududa_amd import kernels as K
    p0, grads = _opt_inputs(numel)
    lr, wd = 2.5e-2, 0.0005
    p, pr = p0.to(dev), p0
    for i, g in enumerate(grads):                      # momentum 0: no buffer at all
        K.sgd_step(p, g.to(dev), None, lr, 0.0, wd, i == 0)
        pr, _ = R.sgd_step(pr, g, None, lr, 0.0, wd, i == 0)
        assert rel_err(p, pr) < 1e-6
    p, buf, pr, bufr = p0.to(dev), torch.zeros(numel, device=dev), p0, None
    for i, g in enumerate(grads):                      # grad_scale = 1 / world on summed gradients
        K.sgd_step(p, (g * 4).to(dev), buf, lr, 0.99, wd, i == 0, grad_scale=0.25)
        pr, bufr = R.sgd_step(pr, g * 4, bufr, lr, 0.99, wd, i == 0, grad_scale=0.25)
        print("sgd step %d: p %.3g buf %.3g" % (i + 1, rel_err(p, pr), rel_err(buf, bufr)))
        assert rel_err(p, pr) < 1e-6 and rel_err(buf, bufr) < 1e-6
    with pytest.raises(RuntimeError):
        K.sgd_step(p, grads[0].to(dev), None, lr, 0.99, wd, True)   # momentum without a buffer


def test_argument_checks_return_before_any_launch(dev):
    from pointcloududa_amd import kernels as K
    with pytest.raises(RuntimeError):
        K.maxpool2_fwd(torch.zeros(1, 2, 5, 8, device=dev))                        # odd height
    off = torch.zeros(2 * 4 * 8 + 1, device=dev)[1:].view(1, 2, 4, 8)
    assert off.data_ptr() % 8 == 4
    with pytest.raises(RuntimeError):
        K.maxpool2_fwd(off)                                                        # float2 loads need 8-byte alignment
    part, nt, cnt = K.bn_stats(torch.ones(2, 3, 8, device=dev))
    with pytest.raises(RuntimeError):
        K.bn_finalize(part, nt, 0, None, None, None, None)                         # count = 0
