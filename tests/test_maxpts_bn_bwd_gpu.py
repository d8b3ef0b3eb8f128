"""BatchNorm backward behind the max over points with the gradient read in place (csrc/pointnet_small.hip:
pcuda_bn_bwd_reduce_maxpts, pcuda_bn_bwd_apply_maxpts) against today's sequence through the C ABI: K.max_points_bwd writes the
dense [B, C, L] gradient, then pcuda_bn_bwd_reduce -> pcuda_bn_bwd_finalize -> pcuda_bn_bwd_apply.  ``torch.equal`` on dz, dgamma
and dbeta: a row's tile holds one non-zero, so its partial is (0.f + g, 0.f + g * xhat) exactly.

(B, C, L): (2, 5, 1) one point; (3, 7, 37) odd everything, scalar path; (3, 8, 300) the vector path with rows that straddle the
4096-element chunks of the apply kernel; (32, 16, 300) more than one workgroup of the gather; (2, 3, 2052) above the one-tile
limit: K.bn_backward_maxpts takes the dense path itself.  x post_relu (BN -> ReLU, the T-Nets) or not (PointNetfeat's bn3).
g[0][0] = -0.0; channel 1 sits below the ReLU everywhere, so that the mask of the post_relu form is exercised.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 1), (3, 7, 37), (3, 8, 300), (32, 16, 300), (2, 3, 2052)]


@functools.lru_cache(maxsize=None)
def _case(b, c, l):
    rng = np.random.default_rng(b + 10 * c + 1000 * l)
    t = lambda *sh, mu=0.0: torch.from_numpy(rng.normal(mu, 1.0, sh).astype(np.float32))
    g = t(b, c)
    g[0, 0] = -0.0
    beta = t(c)
    beta[1] = -50.0      # with the ReLU, channel 1 is 0 everywhere: its maxima are masked (gg = 0), idx = 0
    return dict(a=t(b, c, l, mu=0.2), g=g, gamma=t(c, mu=1.0), beta=beta, dgamma=t(c), dbeta=t(c))


def _dense_reference(K, L, g, idx, a, st, gamma, dgamma, dbeta, post_relu):
    lib = L.lib()
    b, c, l = a.shape
    dy = K.max_points_bwd(g, idx, l)
    nt = C.c_int(0)
    L.check(lib.pcuda_bn_bwd_reduce(None, 0, 0, None, 0, 0, None, 0, 0, None, None, None, None, 0, b, c, l, None, C.byref(nt),
                                    K._stream()), "query")
    red = torch.empty((nt.value, c, 2), dtype=torch.float32, device=a.device)
    L.check(lib.pcuda_bn_bwd_reduce(dy.data_ptr(), c * l, l, None, 0, 0, a.data_ptr(), c * l, l, st.mean.data_ptr(),
                                    st.invstd.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), post_relu, b, c, l,
                                    red.data_ptr(), C.byref(nt), K._stream()), "reduce")
    coef = torch.empty((c, 3), dtype=torch.float32, device=a.device)
    L.check(lib.pcuda_bn_bwd_finalize(red.data_ptr(), nt.value, c, b * l, gamma.data_ptr(), st.invstd.data_ptr(), st.mean.data_ptr(),
                                      dgamma.data_ptr(), dbeta.data_ptr(), 1, coef.data_ptr(), K._stream()), "finalize")
    dz = torch.empty_like(a)
    L.check(lib.pcuda_bn_bwd_apply(dy.data_ptr(), c * l, l, None, 0, 0, a.data_ptr(), c * l, l, coef.data_ptr(),
                                   st.scale.data_ptr(), st.shift.data_ptr(), post_relu, 1.0, dz.data_ptr(), c * l, l, b, c, l,
                                   K._stream()), "apply")
    return dz


@pytest.mark.parametrize("post_relu", [0, 1], ids=["lin", "postrelu"])
@pytest.mark.parametrize("b,c,l", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_in_place_gradient_is_bit_equal_to_the_dense_one(dev, b, c, l, post_relu):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    cs = {k: v.to(dev) for k, v in _case(b, c, l).items()}
    a, g, gamma = cs["a"], cs["g"], cs["gamma"]
    part, nt, cnt = K.bn_stats(a)
    st = K.bn_finalize(part, nt, cnt, gamma, cs["beta"], None, None)
    y = K.bn_apply(a, st, relu=bool(post_relu))
    _, idx = K.max_points_fwd(y)
    dg_r, db_r, dg_g, db_g = cs["dgamma"].clone(), cs["dbeta"].clone(), cs["dgamma"].clone(), cs["dbeta"].clone()
    dz_r = _dense_reference(K, L, g, idx, a, st, gamma, dg_r, db_r, post_relu)
    n0 = K.launch_count()
    dz_g = K.bn_backward_maxpts(g, idx, a, st, gamma, dg_g, db_g, post_relu=bool(post_relu))
    assert K.launch_count() - n0 == (3 if l <= 2048 else 4)      # gather, finalize, apply | scatter + the three dense ones
    for nm, got, ref in (("dz", dz_g, dz_r), ("dgamma", dg_g, dg_r), ("dbeta", db_g, db_r)):
        assert torch.equal(got, ref), "%s differs in %d of %d elements" % (nm, int((got != ref).sum()), ref.numel())
    if post_relu:      # (the mask was live in channel 1 and idle elsewhere)
        assert bool((y[:, 1] == 0).all()) and int((y.amax(2) > 0).sum()) > 0
