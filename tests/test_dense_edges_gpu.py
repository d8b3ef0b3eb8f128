"""dense.hip at its dispatch borders, against the float64 statements of tests/fp64_refs.py.  Bound 1e-5 (the project's
bound for the dense operations, here against float64); max values, indices and scatters bit-exact.

(m, k, n) of y = x w^T + b -> branch.  launch_gemm takes the skinny kernel for `rows <= 64 && depth >= 64` of the GEMM at
hand: forward rows = m, depth = k; bwd_x rows = m, depth = n; bwd_w rows = n, depth = m (or the slice of m).
  (64, 64, 8)       forward: skinny at both borders (wave 15 owns k = 60..63); bwd_w skinny (n = 8, m = 64)
  (65, 64, 9)       forward: m one past the skinny limit -> tiled kernel
  (64, 63, 7)       forward: k one below the skinny limit -> tiled kernel
  (1, 1000, 10)     a single row (lanes 1..63 clamp to row 0); bwd_w depth 1 -> tiled
  (40, 70, 65)      skinny with k = 70 over 16 waves: 5 each, waves 14 and 15 idle; colsum with n = 65: two workgroups of 64
  (2048, 121, 3)    bwd_w split-K: 8 slices of 256 rows, no tail
  (2050, 121, 3)    bwd_w split-K: 7 batched slices of 257 rows + a tail of 251 rows on the skinny kernel
  (9600, 121, 3)    the production shape: 37 slices
  (16700, 9, 3)     slice count capped at 64 (63 batched slices of 261 rows + a tail of 257)
  (2048, 256, 256)  n * k = 65536 exactly: still splits
  (2048, 257, 256)  one over: one tiled launch, no workspace
  ... x accumulate  the `+=` of dw (splitk_reduce_kernel or the GEMM epilogue), db (colsum_kernel), dx (C ABI only)
  bmm (33, 31, 65), (1, 1, 1) x ta x tb x accumulate    no multiple of the 32-tile; both transposes; `+=` (C ABI only)
  max_points l = 1, 37, 64, 65, 300 with 21 rows        fewer than 64 points, 64, one more; rows no multiple of 4;
                                                        ties inside a lane (5, 69) and across lanes (70 in lane 6, 7 in lane 7)
"""
import functools

import numpy as np
import pytest
import torch

import fp64_refs as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

LINEAR = [(64, 64, 8), (65, 64, 9), (64, 63, 7), (1, 1000, 10), (40, 70, 65), (2048, 121, 3), (2050, 121, 3), (9600, 121, 3),
          (16700, 9, 3), (2048, 256, 256), (2048, 257, 256)]
SPLITS = {(2048, 121, 3): 8, (2050, 121, 3): 8, (9600, 121, 3): 37, (16700, 9, 3): 64, (2048, 256, 256): 8}


def _rand(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.normal(0, scale, shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _linear_case(m, k, n):
    rng = np.random.default_rng(m + 3 * k + 7 * n)
    x, w, b, g = _rand(rng, m, k), _rand(rng, n, k, scale=0.1), _rand(rng, n), _rand(rng, m, n)
    pre = dict(dx=_rand(rng, m, k), dw=_rand(rng, n, k), db=_rand(rng, n))
    return x, w, b, g, pre, R.linear(x, w, b), R.linear_backward(g, x, w)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("m,k,n", LINEAR, ids=["x".join(map(str, s)) for s in LINEAR])
def test_linear_against_float64(dev, m, k, n, accumulate):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    x, w, b, g, pre, y_r, (dx_r, dw_r, db_r) = _linear_case(m, k, n)
    xd, wd, bd, gd = x.to(dev), w.to(dev), b.to(dev), g.to(dev)
    # the split the table above promises: workspace for (slices + 1) partial results, or none
    want_ws = (SPLITS[(m, k, n)] + 1) * n * k * 4 if (m, k, n) in SPLITS else 0
    assert L.lib().pcuda_linear_bwd_w_workspace_size(m, k, n) == want_ws
    errs = [rel_err(K.linear_fwd(xd, wd, bd), y_r)]
    if accumulate:
        dx, dw, db = pre["dx"].to(dev), pre["dw"].to(dev), pre["db"].to(dev)
        L.check(L.lib().pcuda_linear_bwd_x(gd.data_ptr(), wd.data_ptr(), dx.data_ptr(), m, k, n, 1, K._stream()), "linear_bwd_x")
        K.linear_bwd_w(gd, xd, dw, db)                           # accumulate=True is the default
        dx_r, dw_r, db_r = dx_r + pre["dx"].double(), dw_r + pre["dw"].double(), db_r + pre["db"].double()
    else:
        dx = K.linear_bwd_x(gd, wd)
        dw, db = torch.full((n, k), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev)
        K.linear_bwd_w(gd, xd, dw, db, accumulate=False)
    errs += [rel_err(dx, dx_r), rel_err(dw, dw_r), rel_err(db, db_r)]
    print("linear %s acc=%d: y %.3g dx %.3g dw %.3g db %.3g" % ((m, k, n), accumulate, *errs))
    assert max(errs) < 1e-5
    if not accumulate:
        dw2 = torch.zeros(n, k, device=dev)
        K.linear_bwd_w(gd, xd, dw2, None, accumulate=False)      # no bias gradient asked for
        assert torch.equal(dw2, dw)


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("m,k,n", [(33, 31, 65), (1, 1, 1)])
def test_bmm_against_float64(dev, m, k, n, ta, tb):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(m + 2 * ta + tb)
    batch = 3
    a, b = _rand(rng, batch, *((k, m) if ta else (m, k))), _rand(rng, batch, *((n, k) if tb else (k, n)))
    ref = R.bmm(a, b, ta, tb)
    ad, bd = a.to(dev), b.to(dev)
    assert rel_err(K.bmm(ad, bd, ta=ta, tb=tb), ref) < 1e-5
    pre = _rand(rng, batch, m, n)
    c = pre.to(dev)
    L.check(L.lib().pcuda_bmm(ad.data_ptr(), bd.data_ptr(), c.data_ptr(), batch, m, k, n, int(ta), int(tb), 1, K._stream()), "bmm")
    assert rel_err(c, ref + pre.double()) < 1e-5


@pytest.mark.parametrize("l", [1, 37, 64, 65, 300])
def test_max_points_ties_and_short_rows(dev, l):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(l)
    b, c = 3, 7                                                    # 21 rows: the last workgroup has one live wave
    h = _rand(rng, b, c, l)
    want = {}
    if l == 300:
        h[0, 0, 5] = h[0, 0, 69] = 9.0                             # one lane sees both: the first stays
        h[0, 1, 70] = h[0, 1, 7] = 9.0                             # lane 6 holds 70, lane 7 holds 7: the smaller index wins
        want = {(0, 0): 5, (0, 1): 7}
    elif l == 65:
        h[0, 0, 0] = h[0, 0, 64] = 9.0                             # lane 0's first and only second element
        want = {(0, 0): 0}
    elif l > 1:
        h[0, 0, 3] = h[0, 0, l - 1] = 9.0                          # two lanes, the rest of the wave idle or full
        want = {(0, 0): 3}
    v_r, i_r = R.max_points(h)
    for (bi, ci), i in want.items():
        assert int(i_r[bi, ci]) == i
    v, idx = K.max_points_fwd(h.to(dev))
    assert torch.equal(v.cpu().double(), v_r)
    assert torch.equal(idx.cpu().long(), i_r)
    g = _rand(rng, b, c)
    ref = torch.zeros(b, c, l, dtype=torch.float64).scatter_(2, i_r[..., None], g.double()[..., None])
    assert torch.equal(K.max_points_bwd(g.to(dev), idx, l).cpu().double(), ref)
