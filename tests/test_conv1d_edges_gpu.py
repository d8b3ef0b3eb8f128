"""conv1d_f32.hip at its dispatch borders, against the float64 statements of tests/fp64_refs.py.  Every case asserts the
instantiation that ran (K.last_kernel(), written out per case below, not computed) and that no fallback was counted.

(b, cin, cout, l) -> branch.  c1d_gemm_kernel<MB, TA, VEC>: 64 columns (points) x 64 * MB rows per workgroup; MB = 2 when
rows > 64 and ceil(b*l / 64) * ceil(rows / 128) >= 512 (rows = cout forward, cin dgrad); TA = dgrad; VEC = cin, cout, l
multiples of 4 and 16-byte aligned tensors (32-deep stages, else 16-deep).  c1d_wgrad_kernel<MB>: MB = 2 for cout > 64;
32 columns per step, ksplit slices of ceil(steps / ksplit) steps each.
  (16, 8, 1024, 256)   forward 64 x 8 = 512 workgroups: exactly at the switch -> mb2 vec; dgrad 8 rows -> mb1 vec
  (16, 8, 1024, 252)   63 x 8 = 504: one tile column below the switch -> mb1 vec
  (14, 36, 1020, 300)  forward mb2 vec: last row tile has 124 rows, K = 32 + 4 (the second stage holds 2 k-pairs); wgrad mb2
  (14, 33, 1021, 301)  forward mb2 scalar: K = 16 + 16 + 1 (odd tail), batch borders inside column tiles; dgrad mb1 scalar
  (14, 1020, 36, 300)  dgrad mb2 vec; wgrad mb1, ksplit 48, 3 steps per slice, 132 steps -> slices 44..47 own no step
  (14, 1021, 33, 301)  dgrad mb2 scalar
  (1, 4, 4, 288)       9 steps, ksplit 4 of 3 steps -> the last slice is empty
  (1, 64, 64, 64)      exactly one tile on every axis; wgrad mb1
  (1, 65, 65, 65)      one past it on every axis; wgrad mb2
  (1, 1, 1, 1)         a single element
  (2, 128, 129, 4)     4 columns in a 64-column tile; cout no multiple of 4 -> scalar
  (3, 8, 64, 300)      the aligned twin of the misaligned cases: x / w / dy in turn one float into its storage -> the
                       GEMMs that read it take the scalar loaders, results bit-identical (the fma chain is k-ordered in both)

Bounds.  rel_err (max error over the tensor's largest entry) against float64: y, dx 2e-6; dw, db 4e-6; statistics 1e-5, as
tests/test_conv1d_gpu.py.  Element-wise, because rel_err misses a dropped term in a small output: a length-n fp32 fma chain
plus one more rounding (bias, `+=`) is within (n + 2) * 2^-24 * sum |terms| of the exact sum, so
  y, dx:  |got - ref| <= (K + 2) 2^-24 (sum_k |a_k b_k| + |bias|),  K = cin forward, cout dgrad
  dw, db: |got - ref| <= (b*l + ksplit + 2) 2^-24 (sum |dy x| + |previous value|)   (db: sum |dy|)
with the sums of absolute values computed in float64 (the same statements on |inputs|)."""
import functools

import numpy as np
import pytest
import torch

import fp64_refs as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
G = "c1d_gemm "
CASES = [  # (b, cin, cout, l), forward, dgrad, wgrad, ksplit
    ((16, 8, 1024, 256), G + "mb2 ta0 vec1", G + "mb1 ta1 vec1", "c1d_wgrad mb2", 64),
    ((16, 8, 1024, 252), G + "mb1 ta0 vec1", G + "mb1 ta1 vec1", "c1d_wgrad mb2", 63),
    ((14, 36, 1020, 300), G + "mb2 ta0 vec1", G + "mb1 ta1 vec1", "c1d_wgrad mb2", 66),
    ((14, 33, 1021, 301), G + "mb2 ta0 vec0", G + "mb1 ta1 vec0", "c1d_wgrad mb2", 66),
    ((14, 1020, 36, 300), G + "mb1 ta0 vec1", G + "mb2 ta1 vec1", "c1d_wgrad mb1", 48),
    ((14, 1021, 33, 301), G + "mb1 ta0 vec0", G + "mb2 ta1 vec0", "c1d_wgrad mb1", 48),
    ((1, 4, 4, 288), G + "mb1 ta0 vec1", G + "mb1 ta1 vec1", "c1d_wgrad mb1", 4),
    ((1, 64, 64, 64), G + "mb1 ta0 vec1", G + "mb1 ta1 vec1", "c1d_wgrad mb1", 1),
    ((1, 65, 65, 65), G + "mb1 ta0 vec0", G + "mb1 ta1 vec0", "c1d_wgrad mb2", 1),
    ((1, 1, 1, 1), G + "mb1 ta0 vec0", G + "mb1 ta1 vec0", "c1d_wgrad mb1", 1),
    ((2, 128, 129, 4), G + "mb1 ta0 vec0", G + "mb1 ta1 vec0", "c1d_wgrad mb2", 1),
    ((3, 8, 64, 300), G + "mb1 ta0 vec1", G + "mb1 ta1 vec1", "c1d_wgrad mb1", 14),
]
MISALIGNED = [  # which tensor starts one float into its storage -> forward (reads x, w), dgrad (reads dy, w)
    ("x", G + "mb1 ta0 vec0", G + "mb1 ta1 vec1"),
    ("w", G + "mb1 ta0 vec0", G + "mb1 ta1 vec0"),
    ("dy", G + "mb1 ta0 vec1", G + "mb1 ta1 vec0"),
]


def _rand(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=2)
def _case(b, cin, cout, l):
    """inputs, previous dw / db for the `+=`, float64 results, and the float64 sums of absolute values of the bounds"""
    rng = np.random.default_rng(b * 1000 + cin + cout + l)
    x, w, bias, dy = _rand(rng, b, cin, l), _rand(rng, cout, cin, scale=cin ** -0.5), _rand(rng, cout), _rand(rng, b, cout, l)
    pre_dw, pre_db = _rand(rng, cout, cin), _rand(rng, cout)
    ref = dict(zip(("y", "s1", "s2"), R.conv1d_k1(x, w, bias)))
    ref.update(zip(("y0", "s1_0", "s2_0"), R.conv1d_k1(x, w, None)))
    ref.update(zip(("dx", "dw", "db"), R.conv1d_k1_backward(dy, x, w)))
    mag = dict(y=R.conv1d_k1(x.abs(), w.abs(), bias.abs())[0], y0=R.conv1d_k1(x.abs(), w.abs(), None)[0])
    mag.update(zip(("dx", "dw", "db"), R.conv1d_k1_backward(dy.abs(), x.abs(), w.abs())))
    return dict(x=x, w=w, bias=bias, dy=dy, pre_dw=pre_dw, pre_db=pre_db), ref, mag


def _run(K, shape, t, want=None):
    """every entry point once on the device tensors ``t``: outputs, and the kernel each GEMM ran on"""
    b, cin, cout, l = shape
    dev = t["x"].device
    out, ran = {}, {}
    out["y"], out["part"], nt = K.conv1d_fwd(t["x"], t["w"], t["bias"], want_stats=True)
    ran["fwd"] = K.last_kernel()
    assert out["part"].shape == (nt, cout, 2) and nt == (b * l + 63) // 64
    out["y0"], out["part0"], _ = K.conv1d_fwd(t["x"], t["w"], None, want_stats=True)
    ran["fwd0"] = K.last_kernel()
    y_plain, none, _ = K.conv1d_fwd(t["x"], t["w"], t["bias"])          # the epilogue without statistics: same y
    assert none is None and torch.equal(y_plain, out["y"])
    out["dx"] = K.conv1d_dgrad(t["dy"], t["w"])
    ran["dgrad"] = K.last_kernel()
    out["dw"] = torch.full((cout, cin), float("nan"), device=dev)
    out["db"] = torch.full((cout,), float("nan"), device=dev)
    K.conv1d_wgrad(t["x"], t["dy"], out["dw"], out["db"], accumulate=False)
    ran["wgrad"] = K.last_kernel()
    out["dw_nodb"] = torch.full((cout, cin), float("nan"), device=dev)
    K.conv1d_wgrad(t["x"], t["dy"], out["dw_nodb"], None, accumulate=False)
    out["dw_acc"], out["db_acc"] = t["pre_dw"].clone(), t["pre_db"].clone()
    K.conv1d_wgrad(t["x"], t["dy"], out["dw_acc"], out["db_acc"], accumulate=True)
    ran["wgrad_acc"] = K.last_kernel()
    if want is not None:
        fwd, dgrad, wgrad, ksplit = want
        dims = "n%d cin%d cout%d l%d" % shape
        assert ran["fwd"] == "conv1d f32 fwd %s | %s" % (dims, fwd), ran["fwd"]
        assert ran["fwd0"] == ran["fwd"]
        assert ran["dgrad"] == "conv1d f32 dgrad %s | %s" % (dims, dgrad), ran["dgrad"]
        assert ran["wgrad"] == "conv1d f32 wgrad %s ksplit%d | %s" % (dims, ksplit, wgrad), ran["wgrad"]
        assert ran["wgrad_acc"] == ran["wgrad"]
    return out


def _check(name, got, ref, mag, n, tol):
    """the rel_err bound ``tol`` and the element-wise bound n * 2^-24 * mag; -> the two figures"""
    r = rel_err(got, ref)
    err = (got.detach().double().cpu() - ref).abs()
    bound = n * U * mag
    worst = float((err / bound.clamp(min=1e-300)).max())             # (no element has a zero magnitude: normal inputs)
    print("  %-7s rel_err %.3g (bound %.1g)   element-wise: worst error / bound %.3g" % (name, r, tol, worst))
    assert bool((err <= bound).all()), (name, worst)
    assert r < tol, (name, r)
    return r, worst


@pytest.mark.parametrize("shape,fwd,dgrad,wgrad,ksplit", CASES, ids=["x".join(map(str, c[0])) for c in CASES])
def test_conv1d_against_float64(dev, shape, fwd, dgrad, wgrad, ksplit):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    b, cin, cout, l = shape
    host, ref, mag = _case(*shape)
    t = {k: v.to(dev) for k, v in host.items()}
    # the split of the table: the workspace holds ksplit slabs of dw and of db
    assert L.lib().pcuda_conv1d_k1_wgrad_workspace_size(b, cin, cout, l) == ksplit * cout * (cin + 1) * 4 + 256
    fb = K.fallback_count()
    out = _run(K, shape, t, (fwd, dgrad, wgrad, ksplit))
    print("conv1d %s" % (shape,))
    _check("y", out["y"], ref["y"], mag["y"], cin + 2, 2e-6)
    _check("y0", out["y0"], ref["y0"], mag["y0"], cin + 2, 2e-6)
    for part, s1, s2 in ((out["part"], ref["s1"], ref["s2"]), (out["part0"], ref["s1_0"], ref["s2_0"])):
        tot = part.double().sum(0).cpu()
        e1, e2 = rel_err(tot[:, 0], s1), rel_err(tot[:, 1], s2)
        print("  stats   sum %.3g  sum of squares %.3g (bound 1e-05)" % (e1, e2))
        assert e1 < 1e-5 and e2 < 1e-5
    _check("dx", out["dx"], ref["dx"], mag["dx"], cout + 2, 2e-6)
    nw = b * l + ksplit + 2
    _check("dw", out["dw"], ref["dw"], mag["dw"], nw, 4e-6)
    _check("db", out["db"], ref["db"], mag["db"], nw, 4e-6)
    assert torch.equal(out["dw_nodb"], out["dw"])
    pw, pb = host["pre_dw"].double(), host["pre_db"].double()
    _check("dw +=", out["dw_acc"], ref["dw"] + pw, mag["dw"] + pw.abs(), nw, 4e-6)
    _check("db +=", out["db_acc"], ref["db"] + pb, mag["db"] + pb.abs(), nw, 4e-6)
    # deterministic: fixed-order split-K, no atomics anywhere
    again = _run(K, shape, t)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    assert K.fallback_count() == fb


def _one_float_in(t):
    """a contiguous copy of ``t`` that starts one float into its storage: 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("which,fwd,dgrad", MISALIGNED, ids=[m[0] for m in MISALIGNED])
def test_conv1d_misaligned_operand_takes_the_scalar_loaders(dev, which, fwd, dgrad):
    from pointcloududa_amd import kernels as K
    shape = (3, 8, 64, 300)
    host, ref, _ = _case(*shape)
    t = {k: v.to(dev) for k, v in host.items()}
    fb = K.fallback_count()
    aligned = _run(K, shape, t, CASES[-1][1:])                          # (against float64 in the test above)
    assert CASES[-1][0] == shape and all(v.data_ptr() % 16 == 0 for v in t.values())
    t[which] = _one_float_in(t[which])
    got = _run(K, shape, t, (fwd, dgrad, "c1d_wgrad mb1", 14))
    for k in aligned:
        assert torch.equal(got[k], aligned[k]), k
    assert rel_err(got["y"], ref["y"]) < 2e-6 and rel_err(got["dx"], ref["dx"]) < 2e-6 and rel_err(got["dw"], ref["dw"]) < 4e-6
    assert K.fallback_count() == fb


def _small(dev):
    b, cin, cout, l = 2, 8, 8, 16
    rng = np.random.default_rng(0)
    x, w, dy = _rand(rng, b, cin, l).to(dev), _rand(rng, cout, cin).to(dev), _rand(rng, b, cout, l).to(dev)
    return (b, cin, cout, l), x, w, dy


def test_workspace_one_byte_short_is_refused_before_any_launch(dev):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    (b, cin, cout, l), x, _, dy = _small(dev)
    lib = L.lib()
    nb = lib.pcuda_conv1d_k1_wgrad_workspace_size(b, cin, cout, l)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    dw, db = torch.full((cout, cin), float("nan"), device=dev), torch.full((cout,), float("nan"), device=dev)
    launches = K.launch_count()
    rc = lib.pcuda_conv1d_k1_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), b, cin, cout, l, 0,
                                   ws.data_ptr(), nb - 1, K._stream())
    assert rc == -4                                                    # PCUDA_E_WORKSPACE (include/pcuda_hip.h)
    assert b"workspace too small" in lib.pcuda_last_error()
    assert K.launch_count() == launches
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())
    # the full size is accepted
    L.check(lib.pcuda_conv1d_k1_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), b, cin, cout, l, 0,
                                      ws.data_ptr(), nb, K._stream()), "conv1d_k1_wgrad")
    assert rel_err(dw, R.conv1d_k1_backward(dy, x, torch.zeros(cout, cin))[1]) < 4e-6


def test_empty_batch_is_a_bad_argument_before_any_launch(dev):
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    (_, cin, cout, l), x, w, dy = _small(dev)
    lib = L.lib()
    y, dx = torch.full_like(dy, float("nan")), torch.full_like(x, float("nan"))
    dw = torch.full((cout, cin), float("nan"), device=dev)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    assert lib.pcuda_conv1d_k1_wgrad_workspace_size(0, cin, cout, l) == 0 and lib.pcuda_conv1d_k1_fwd_tiles(0, l) == 0
    launches = K.launch_count()
    s = K._stream()
    bad = -1                                                           # PCUDA_E_BADARG (include/pcuda_hip.h)
    assert lib.pcuda_conv1d_k1_fwd(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), 0, cin, cout, l, None, s) == bad
    assert b"conv1d_k1_fwd: bad arguments" in lib.pcuda_last_error()
    assert lib.pcuda_conv1d_k1_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), 0, cin, cout, l, s) == bad
    assert b"conv1d_k1_dgrad: bad arguments" in lib.pcuda_last_error()
    assert lib.pcuda_conv1d_k1_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), None, 0, cin, cout, l, 0, ws.data_ptr(), 4096,
                                     s) == bad
    assert b"conv1d_k1_wgrad: bad arguments" in lib.pcuda_last_error()
    assert K.launch_count() == launches
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(dx).all()) and bool(torch.isnan(dw).all())
