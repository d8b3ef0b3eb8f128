"""BatchNorm1d on [B, C] in one launch per direction (csrc/pointnet_small.hip: pcuda_bn1d_fwd, pcuda_bn1d_bwd) against the
three launches it replaces, called through the C ABI: pcuda_bn_stats -> pcuda_bn_finalize -> pcuda_bn_apply forward,
pcuda_bn_bwd_reduce -> pcuda_bn_bwd_finalize -> pcuda_bn_bwd_apply backward.  Every comparison is ``torch.equal``: the fused
kernels keep the association of every sum (one sample per tile, tile t in slot t % 256, the 256-slot fp64 tree).

(B, C): (2, 5) two samples, fewer channels than a workgroup's 16; (32, 512) and (64, 256) the production shapes, 32 and 16
workgroups; (257, 3) sample 256 is the second one of slot 0 (tile_pair_sum's second trip).  Channel 0 holds -0.0 only
(the partial is 0.f + a = +0.0; variance 0), channel 1 a constant.  x ReLU x affine present / absent x accumulate.
K.bn_backward with a second gradient share (dy2) or frozen statistics must take the three launches (no fused form): same
bits, and the launch count says which path ran.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5), (32, 512), (64, 256), (257, 3)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(b, c):
    rng = np.random.default_rng(11 * b + c)
    t = lambda *sh, mu=0.0: torch.from_numpy(rng.normal(mu, 1.0, sh).astype(np.float32))
    a = t(b, c, mu=0.3)
    a[:, 0] = -0.0
    a[:, 1] = 1.7
    return dict(a=a, dy=t(b, c), gamma=t(c, mu=1.0), beta=t(c), rm=t(c), rv=t(c).abs() + 0.5, dgamma=t(c), dbeta=t(c))


def _ref_forward(K, L, a, gamma, beta, rm, rv, relu):
    """the general path, raw entry points"""
    lib = L.lib()
    b, c = a.shape
    nt = C.c_int(0)
    L.check(lib.pcuda_bn_stats(None, a.stride(0), a.stride(1), b, c, 1, None, C.byref(nt), K._stream()), "q")
    assert nt.value == b
    part = torch.empty((b, c, 2), dtype=torch.float32, device=a.device)
    L.check(lib.pcuda_bn_stats(a.data_ptr(), a.stride(0), a.stride(1), b, c, 1, part.data_ptr(), C.byref(nt), K._stream()), "stats")
    st = K.bn_finalize(part, b, b, gamma, beta, rm, rv)
    y = torch.empty_like(a)
    L.check(lib.pcuda_bn_apply(a.data_ptr(), a.stride(0), a.stride(1), st.scale.data_ptr(), st.shift.data_ptr(), 1 if relu else 0,
                               y.data_ptr(), y.stride(0), y.stride(1), b, c, 1, K._stream()), "apply")
    return st, y


def _ref_backward(K, L, dy, a, st, gamma, dgamma, dbeta, post_relu, slope, accumulate, dy2=None, count=None):
    lib = L.lib()
    b, c = a.shape
    p = lambda t: None if t is None else t.data_ptr()
    d2 = (p(dy2), dy2.stride(0), dy2.stride(1)) if dy2 is not None else (None, 0, 0)
    nt = C.c_int(0)
    red = torch.empty((b, c, 2), dtype=torch.float32, device=a.device)
    L.check(lib.pcuda_bn_bwd_reduce(dy.data_ptr(), dy.stride(0), dy.stride(1), *d2, a.data_ptr(), a.stride(0), a.stride(1),
                                    st.mean.data_ptr(), st.invstd.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(),
                                    1 if post_relu else 0, b, c, 1, red.data_ptr(), C.byref(nt), K._stream()), "reduce")
    assert nt.value == b
    coef = torch.empty((c, 3), dtype=torch.float32, device=a.device)
    L.check(lib.pcuda_bn_bwd_finalize(red.data_ptr(), b, c, b if count is None else count, p(gamma), st.invstd.data_ptr(),
                                      st.mean.data_ptr(), p(dgamma), p(dbeta), 1 if accumulate else 0, coef.data_ptr(),
                                      K._stream()), "finalize")
    dz = torch.empty_like(a)
    L.check(lib.pcuda_bn_bwd_apply(dy.data_ptr(), dy.stride(0), dy.stride(1), *d2, a.data_ptr(), a.stride(0), a.stride(1),
                                   coef.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), 1 if post_relu else 0, float(slope),
                                   dz.data_ptr(), dz.stride(0), dz.stride(1), b, c, 1, K._stream()), "apply")
    return dz


def _eq(got, ref, what):
    assert torch.equal(got, ref), "%s differs: %d of %d elements, max |d| %g" % (
        what, int((got != ref).sum()), ref.numel(), float((got.double() - ref.double()).abs().max()))


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("b,c", SHAPES, ids=IDS)
def test_forward_is_bit_equal_to_the_three_launches(dev, b, c, relu, affine):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    cs = {k: v.to(dev) for k, v in _case(b, c).items()}
    gamma, beta = (cs["gamma"], cs["beta"]) if affine else (None, None)
    rm_r, rv_r, rm_g, rv_g = cs["rm"].clone(), cs["rv"].clone(), cs["rm"].clone(), cs["rv"].clone()
    st_r, y_r = _ref_forward(K, L, cs["a"], gamma, beta, rm_r, rv_r, relu)
    n0 = K.launch_count()
    fused = K.bn1d_forward(cs["a"], gamma, beta, rm_g, rv_g, relu=relu)
    assert fused is not None and K.launch_count() - n0 == 1
    st_g, y_g = fused
    assert st_g.count == b
    _eq(y_g, y_r, "y")
    for nm in ("mean", "invstd", "scale", "shift"):
        _eq(getattr(st_g, nm), getattr(st_r, nm), nm)
    _eq(rm_g, rm_r, "running_mean")
    _eq(rv_g, rv_r, "running_var")
    assert float(st_g.mean[0]) == 0.0 and not np.signbit(float(st_g.mean[0]))      # the -0.0 channel: partials are +0.0


@pytest.mark.parametrize("accumulate", [False, True], ids=["set", "acc"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("relu", [False, True], ids=["lrelu", "postrelu"])
@pytest.mark.parametrize("b,c", SHAPES, ids=IDS)
def test_backward_is_bit_equal_to_the_three_launches(dev, b, c, relu, affine, accumulate):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    cs = {k: v.to(dev) for k, v in _case(b, c).items()}
    gamma, beta = (cs["gamma"], cs["beta"]) if affine else (None, None)
    st, _ = _ref_forward(K, L, cs["a"], gamma, beta, None, None, relu)
    slope = 1.0 if relu else 0.2
    dg_r, db_r, dg_g, db_g = cs["dgamma"].clone(), cs["dbeta"].clone(), cs["dgamma"].clone(), cs["dbeta"].clone()
    dz_r = _ref_backward(K, L, cs["dy"], cs["a"], st, gamma, dg_r, db_r, relu, slope, accumulate)
    n0 = K.launch_count()
    dz_g = K.bn_backward(cs["dy"], cs["a"], st, gamma, dg_g, db_g, post_relu=relu, act_slope=slope, accumulate=accumulate)
    assert K.launch_count() - n0 == 1
    _eq(dz_g, dz_r, "dz")
    _eq(dg_g, dg_r, "dgamma")
    _eq(db_g, db_r, "dbeta")


def test_backward_without_parameter_gradients_and_one_sample(dev):
    """dgamma = dbeta = NULL (the adversarial pass); count == 1: dz is exactly 0 * ... as the three launches leave it"""
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    for b, c in ((32, 512), (1, 20)):
        cs = {k: v[:b].to(dev) if v.dim() == 2 else v.to(dev) for k, v in _case(32, 512).items()}
        cs = {k: (v[:, :c].contiguous() if v.dim() == 2 else v[:c].contiguous()) for k, v in cs.items()}
        st, y_r = _ref_forward(K, L, cs["a"], cs["gamma"], cs["beta"], None, None, True)
        st_g, y_g = K.bn1d_forward(cs["a"], cs["gamma"], cs["beta"], None, None, relu=True)
        _eq(y_g, y_r, "y")
        _eq(st_g.scale, st.scale, "scale")
        dz_r = _ref_backward(K, L, cs["dy"], cs["a"], st, cs["gamma"], None, None, True, 1.0, True)
        dz_g = K.bn_backward(cs["dy"], cs["a"], st, cs["gamma"], None, None, post_relu=True)
        _eq(dz_g, dz_r, "dz")


@pytest.mark.parametrize("which", ["dy2", "frozen", "b1025"])
def test_cases_without_a_fused_form_take_the_three_launches(dev, which):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    b, c = (1025, 3) if which == "b1025" else (32, 512)
    rng = np.random.default_rng(5)
    t = lambda *sh: torch.from_numpy(rng.normal(0, 1.0, sh).astype(np.float32)).to(dev)
    a, dy, dy2, gamma, beta = t(b, c), t(b, c), t(b, c), t(c), t(c)
    st, _ = _ref_forward(K, L, a, gamma, beta, None, None, False)
    if which == "b1025":
        assert K.bn1d_forward(a, gamma, beta, None, None) is None
    dg_r, db_r = t(c), t(c)
    dg_g, db_g = dg_r.clone(), db_r.clone()
    kw = dict(dy2=dy2) if which == "dy2" else {}
    dz_r = _ref_backward(K, L, dy, a, st, gamma, dg_r, db_r, False, 0.2, True, count=-b if which == "frozen" else None, **kw)
    n0 = K.launch_count()
    dz_g = K.bn_backward(dy, a, st, gamma, dg_g, db_g, act_slope=0.2, frozen=which == "frozen", **kw)
    assert K.launch_count() - n0 == 3
    _eq(dz_g, dz_r, "dz")
    _eq(dg_g, dg_r, "dgamma")
    _eq(db_g, db_r, "dbeta")
