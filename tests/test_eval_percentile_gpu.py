"""surface_metrics_ext (eval_metrics.hip: the key-storing last axis pass, the radix select, the 12-column final kernel) and
what is built on it (metric.hd95 / metric.assd, class_metrics_ext, evaluate_volume(extended=True)) against the brute
force of tests/eval_percentile_ref.py; tests/test_eval_percentile.py shows without a GPU that this brute force, scipy's
distance transform and numpy.percentile agree on the same cases.

case -> what it reaches
  surface_cases() of eval_shapes, the           every path of the axis passes with keys stored beside the reductions; 2-D
  degenerate sweep x connectivity x spacing     volumes (a key buffer of their own), lines of length 1, Z = 1 in 3-D
  far_voxels                                    n = 2: lo = 0, hi = 1, both keys 1058846
  n21, n101                                     t = 0 at q = 95: the rank is an integer, hi's key must not leak in
  straddle (and _aniso, _long)                  lo on a key 1 and hi on the far key, t = 0.5: the two queries part at the
                                                second 8-bit digit of the int32 key, at the first of the fp64 key and of
                                                the int32 key 5 + 5000^2 >= 2^24
  big_8x96x96 (and _aniso)                      thousands of keys per class over 256 histogram workgroups
  q = 95, 50, 99.9, 0, 100                      both branches of the interpolation, the ends: column 1 and the minimum
  8 classes, one-sided classes, dtypes          NaN and flags as for hd; border counts where a flag is set

Bounds, no element excused: columns 0..7 the bits of surface_metrics; column 8 bit-equal to the reference at unit
spacing, |got - ref| <= 1e-12 * hd of the class with spacing (each order statistic keeps the 1e-12 relative error of
its distance, and the result lies between two of them); column 9 rtol 1e-12; columns 10, 11 exact.  Every device result
is computed twice and must agree bit for bit.

Self-check (run once on a scratch copy, not committed; wrong values only: no index or loop bound changes):
  1. the select given rank hi for both queries (em_sel_narrow_kernel: rank = hi).  65 of the 75 tests failed: every
     case of the list but speckle_5x33x35, speckle_33x67 (and _aniso), both diagonals, far_voxels and full_vs_itself,
     where s[lo] == s[hi] at all five percentiles (tied distances), and likewise the wrapper test's two volumes; n21 /
     n101 (t = 0, s[lo] < s[hi]) and the three straddle cases are the ones built to catch it.
  2. the second direction's keys dropped from the histograms (em_sel_hist_kernel: d < 1).  71 of 75 failed: all but
     far_voxels and full_vs_itself (both directions hold the same keys, and half of them select the same values), the
     raw entry point test (it compares the entry point with the binding) and class_metrics_ext's argument order.

Wall time on the MI355X: 5.0 s for the file (75 tests); the slowest test 0.54 s (big_8x96x96_aniso, its brute-force
reference included).
"""
import ctypes

import numpy as np
import pytest
import torch

import eval_percentile_ref as R
import eval_shapes as S

G = R.G
pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in R.cases()]
E_WORKSPACE = -4                             # include/pcuda_hip.h: PCUDA_E_WORKSPACE


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _dev(a, dev):
    return a if torch.is_tensor(a) else torch.from_numpy(np.array(a)).to(dev)            # (a copy: the cases are read-only)


def _ext(dev, pred, gt, cls, sp=None, conn=1, q=95.0):
    """K.surface_metrics_ext on the host, computed twice: the same bits"""
    from pointcloududa_amd import kernels as K
    tp, tg = _dev(pred, dev), _dev(gt, dev)
    out = K.surface_metrics_ext(tp, tg, cls, sp, conn, q)
    assert out.dtype == torch.float64 and out.is_cuda and out.shape == (len(cls), 12)
    got = out.cpu().numpy()
    again = K.surface_metrics_ext(tp, tg, cls, sp, conn, q).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(again)), ("run to run", got, again)
    return got


def _plain(dev, pred, gt, cls, sp=None, conn=1):
    from pointcloududa_amd import kernels as K
    return K.surface_metrics(_dev(pred, dev), _dev(gt, dev), cls, sp, conn).cpu().numpy()


def _check(got, plain, sets, q, unit, what):
    """one call's 12 columns against surface_metrics' rows and the reference's distance sets"""
    assert np.array_equal(_bits(got[:, :8]), _bits(plain)), (what, got[:, :8], plain)
    exp = R.ext_columns(sets, q)
    print(what, "q", q, "got", got[:, 8:].tolist(), "exp", exp.tolist())
    assert np.array_equal(got[:, 10:], exp[:, 2:]), (what, got[:, 10:], exp[:, 2:])
    for k, (ab, ba, _, _, flags) in enumerate(sets):
        assert got[k, 7] == flags, (what, k)
        if flags:
            assert np.isnan(got[k, 8]) and np.isnan(got[k, 9]), (what, k, got[k])
            continue
        pooled = np.hstack((ab, ba))
        hd = pooled.max()
        if unit:
            assert got[k, 8] == exp[k, 0], (what, k, q, got[k, 8], exp[k, 0])
            if q == 0.0:
                assert got[k, 8] == pooled.min(), (what, k)
        else:
            assert abs(got[k, 8] - exp[k, 0]) <= 1e-12 * hd, (what, k, q, got[k, 8], exp[k, 0], hd)
            if q == 0.0 and pooled.min() == 0.0:
                assert got[k, 8] == 0.0, (what, k)
        if q == 100.0:
            assert _bits(got[k, 8:9]) == _bits(got[k, 1:2]), (what, k, got[k, 8], got[k, 1])
        assert abs(got[k, 9] - exp[k, 1]) <= 1e-12 * abs(exp[k, 1]), (what, k, got[k, 9], exp[k, 1])


# ------------------------------------------------------------------------------------------------ the case list
@pytest.mark.parametrize("name", NAMES)
def test_ext_rows_on_every_case(dev, name):
    pred, gt, cls, sp, conn = R.case(name)
    sets = R.case_sets(name)
    plain = _plain(dev, pred, gt, cls, sp, conn)
    for q in R.QS:
        _check(_ext(dev, pred, gt, cls, sp, conn, q), plain, sets, q, sp is None, name)
    if name in ("straddle", "far_voxels"):
        got = _ext(dev, pred, gt, cls, sp, conn, 95.0)[0, 8]
        far = np.sqrt(float(R.FAR_KEY))
        assert got == (far - (far - 1.0) * 0.5 if name == "straddle" else far)


def test_hd95_is_not_hd_on_these_shapes(dev):
    """the figures that tell the percentile from the maximum and from a neighbouring rank"""
    pred, gt, cls, sp, conn = R.case("full_vs_voxel")
    got = _ext(dev, pred, gt, cls, sp, conn)
    assert abs(got[0, 8] - 13.601) < 1e-3 and abs(got[0, 1] - 15.843) < 1e-3
    pred, gt = S.degenerate_pair(G.blobs, (65, 3))
    got = _ext(dev, pred, gt, [1, 2, 3])
    assert abs(got[0, 8] - 1.4435) < 1e-4 and got[0, 1] == 21.0


# ------------------------------------------------------------------------------------------------ classes and dtypes
def test_eight_classes_one_sided_classes_and_dtypes(dev):
    from pointcloududa_amd import kernels as K
    shape = (7, 20, 22)
    pred, gt = G.blobs(shape, 321, [1, 2, 4, 5], n=8), G.blobs(shape, 321, [1, 2, 4, 5], n=8, shift=2)
    pred, gt = pred.copy(), gt.copy()
    pred[pred == 4] = 0                                                  # 4: only in gt; 5: only in pred
    gt[gt == 5] = 0
    cls = [1, 2, 1, 0, 4, 5, 7, 2]                                       # duplicates, background, one-sided, absent
    for sp, conn in ((None, 1), (S.ANISO, 3)):
        sets = R.class_sets(pred, gt, cls, sp, conn)
        assert [s[4] for s in sets] == [0, 0, 0, 0, 1, 2, 3, 0]
        assert sets[4][3] > 0 and sets[5][2] > 0 and sets[4][2] == sets[5][3] == 0           # a border on one side only
        plain = _plain(dev, pred, gt, cls, sp, conn)
        for q in (95.0, 50.0):
            got = _ext(dev, pred, gt, cls, sp, conn, q)
            _check(got, plain, sets, q, sp is None, ("8 classes", sp))
            assert np.array_equal(_bits(got[0]), _bits(got[2])) and np.array_equal(_bits(got[1]), _bits(got[7]))
    base = _ext(dev, pred, gt, cls)
    p8, g8, p32, g32 = pred.astype(np.uint8), gt.astype(np.uint8), pred.astype(np.int32), gt.astype(np.int32)
    for a, b in ((p8, g8), (p32, g32), (p8, g32), (p32, g8), (pred.astype(np.int64), gt.astype(np.int16))):
        assert np.array_equal(_bits(_ext(dev, a, b, cls)), _bits(base)), (a.dtype, b.dtype)
    with pytest.raises(ValueError, match="int32"):
        K.surface_metrics_ext(_dev(p32, dev), _dev(g32, dev), [1, 2 ** 32 + 1])
    with pytest.raises(ValueError, match="shapes differ"):
        K.surface_metrics_ext(_dev(p32, dev), _dev(g32[1:], dev), [1])
    with pytest.raises(RuntimeError, match="percentile"):
        K.surface_metrics_ext(_dev(p8, dev), _dev(g8, dev), [1], percentile=101.0)
    # a strided view: the result of its contiguous copy
    big = torch.zeros((9, 24, 44), dtype=torch.int32, device=dev)
    view = big[1:8, 2:22, 0:44:2]
    view.copy_(_dev(p32, dev))
    assert not view.is_contiguous()
    assert np.array_equal(_bits(_ext(dev, view, g32, cls)), _bits(base))


def test_raw_entry_point_and_a_short_workspace_on_the_device(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd import kernels as K
    lib = _lib.lib()
    pred, gt = (torch.from_numpy(a.astype(np.uint8)).to(dev) for a in S.degenerate_pair(G.blobs, (9, 17, 19)))
    cls = (ctypes.c_int * 3)(1, 2, 3)
    out = torch.full((3, 12), -5.0, dtype=torch.float64, device=dev)
    for sp in (None, (ctypes.c_double * 3)(*S.ANISO)):
        need = lib.pcuda_surface_metrics_ext_workspace_size(3, 9, 17, 19, 3, sp)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        before = K.launch_count()
        rc = lib.pcuda_surface_metrics_ext(pred.data_ptr(), gt.data_ptr(), 0, 3, 9, 17, 19, cls, 3, 1, sp, 95.0,
                                           out.data_ptr(), ws.data_ptr(), need - 1, K._stream())
        assert rc == E_WORKSPACE and b"workspace" in lib.pcuda_last_error()
        assert K.launch_count() == before
        torch.cuda.synchronize()
        assert bool((out == -5.0).all())                                 # nothing written
        # the documented launch count: border, three axis passes, two per select pass (4 int / 8 fp64), final
        rc = lib.pcuda_surface_metrics_ext(pred.data_ptr(), gt.data_ptr(), 0, 3, 9, 17, 19, cls, 3, 1, sp, 95.0,
                                           out.data_ptr(), ws.data_ptr(), need, K._stream())
        assert rc == 0
        assert K.launch_count() - before == (13 if sp is None else 21)
        torch.cuda.synchronize()
        exp = K.surface_metrics_ext(pred, gt, [1, 2, 3], None if sp is None else S.ANISO).cpu().numpy()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(exp))
        out.fill_(-5.0)


# ------------------------------------------------------------------------------------------------ medpy's names
def test_hd95_and_assd_wrappers(dev):
    from pointcloududa_amd.utils import metric as M
    pred, gt = S.degenerate_pair(G.blobs, (9, 17, 19))
    a, b = pred == 1, gt == 1
    for sp, conn in ((None, 1), (S.ANISO, 2)):
        (ab, ba, _, _, _), = R.class_sets(a, b, [1], sp, conn)
        hd = max(ab.max(), ba.max())
        ref95 = R.hd95_ref(a, b, sp, conn, sd=R.sd_brute)
        refas = R.assd_ref(a, b, sp, conn, sd=R.sd_brute)
        assert ref95 == R.percentile_linear(np.hstack((ab, ba)), 95.0) and ref95 < hd
        got95, gotas = M.hd95(a, b, sp, conn), M.assd(a, b, sp, conn)
        assert isinstance(got95, float) and isinstance(gotas, float)
        print("wrappers", sp, got95, ref95, gotas, refas)
        assert got95 == ref95 if sp is None else abs(got95 - ref95) <= 1e-12 * hd
        assert abs(gotas - refas) <= 1e-12 * refas
        assert M.hd95(b, a, sp, conn) == got95 and M.assd(b, a, sp, conn) == gotas          # symmetric, bit for bit
        assert M.hd95(torch.from_numpy(pred).to(dev) == 1, gt == 1, sp, conn) == got95       # tensors and numpy alike
    assert M.hd95(pred, gt) == M.hd95(pred != 0, gt != 0)                                    # any non-zero is the object
    empty = np.zeros_like(pred)
    for fn in (M.hd95, M.assd):
        with pytest.raises(RuntimeError, match="first supplied array"):
            fn(empty, gt)
        with pytest.raises(RuntimeError, match="second supplied array"):
            fn(pred, empty)
        with pytest.raises(RuntimeError, match="first supplied array"):
            fn(empty, empty)
    assert M.EMPTY_FIRST == "The first supplied array does not contain any binary object."
    assert M.EMPTY_SECOND == "The second supplied array does not contain any binary object."


def test_class_metrics_ext_argument_order(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import metric as M
    pred, gt = S.degenerate_pair(G.blobs, (9, 17, 19))
    got = M.class_metrics_ext(gt, pred, [1, 2, 3], percentile=50.0)
    assert got.is_cuda and got.shape == (3, 12)
    exp = K.surface_metrics_ext(_dev(gt, dev), _dev(pred, dev), [1, 2, 3], percentile=50.0)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(exp.cpu().numpy()))
    assert np.array_equal(_bits(got[:, :8].cpu().numpy()), _bits(M.class_metrics(gt, pred, [1, 2, 3]).cpu().numpy()))


# ------------------------------------------------------------------------------------------------ evaluate_volume
def _stub_model(dev, n_class):
    """a 'segmenter' whose logits put every pixel in the class of its intensity band (tests/test_eval_metrics_gpu.py)"""
    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, x):
            centres = torch.linspace(0, 1, n_class, device=x.device).view(1, -1, 1, 1)
            return (-(x[:, :1] - centres) ** 2 * self.w).contiguous(), None, None
    return Stub().to(dev)


@pytest.mark.parametrize("variant", ["mmwhs", "mscmrseg"])
def test_evaluate_volume_extended(dev, variant):
    from pointcloududa_amd import validate as V
    from pointcloududa_amd.utils import metric as M
    from pointcloududa_amd.utils import utils as U
    n_class = 5 if variant == "mmwhs" else 4
    labels = [1, 2, 3, 4][:n_class - 1]
    model = _stub_model(dev, n_class)
    rng = np.random.default_rng(100)
    x = np.stack([G.blobs((40, 40), 100 + j, labels, n=10) for j in range(10)])
    x = (x / (n_class - 1) + rng.normal(0, 0.08, x.shape)).astype(np.float32)[:, None]
    gt = np.stack([G.blobs((40, 40), 100 + j, labels, n=10, shift=2) for j in range(10)])
    with torch.no_grad():
        pred = U.keep_largest_connected_components(M.argmax_labels(model(torch.from_numpy(x).to(dev))[0])).cpu().numpy()
    if variant == "mscmrseg":
        lut = np.array([0, 200, 500, 600]); pred, gt = lut[pred], lut[gt]
        cls = [500, 600, 200]
    else:
        cls = [1, 2, 3, 4]
    plain = V.evaluate_volume(model, x, gt, bs=4, variant=variant)
    ext = V.evaluate_volume(model, x, gt, bs=4, variant=variant, extended=True)
    assert len(plain) == 3 * len(cls) and len(ext) == 5 * len(cls)
    sets = R.class_sets(gt, pred, cls)                                   # (gt, pred): the scripts' argument order
    assert not any(s[4] for s in sets)
    exp = R.ext_columns(sets, 95.0)
    print(variant, "ext", ext, "exp", exp.tolist())
    for k in range(len(cls)):
        assert [float(v).hex() for v in ext[5 * k:5 * k + 3]] == [float(v).hex() for v in plain[3 * k:3 * k + 3]], k
        assert ext[5 * k + 3] == exp[k, 0], (k, ext[5 * k + 3], exp[k, 0])                   # unit spacing: bit-equal
        assert abs(ext[5 * k + 4] - exp[k, 1]) <= 1e-12 * exp[k, 1], (k, ext[5 * k + 4], exp[k, 1])
    only_hd = V.evaluate_volume(model, x, gt, bs=4, variant=variant, ifasd=False, extended=True)
    assert [only_hd[5 * k + j] for k in range(len(cls)) for j in (2, 4)] == [-1] * (2 * len(cls))
    assert [only_hd[5 * k + 3] for k in range(len(cls))] == [ext[5 * k + 3] for k in range(len(cls))]
