"""eval_metrics.hip where the blob fixture (tests/golden/eval_metrics.npz) never takes it, against the numpy brute-force
restatement of scripts/make_eval_golden.py (surface_brute, largest_components_brute) on the shapes of
tests/eval_shapes.py.  tests/test_eval_metrics.py checks the same brute force against scipy on the same cases.

case -> what it reaches
  snake 129x131, comb 40x129                    one component through 67 / 21 workgroups: em_find over long parent
                                                chains while other blocks hook them
  hanging / lying comb                          junction voxels hooked from two sides at once, each hook the only link
                                                of its side: em_unite's re-link after a lost atomicMin
  two / joined snakes [3, 33, 35]               equal sizes: the raster-first root wins; one voxel joins them across planes
  rings 63, checker (5, 6, 7)                   nested components of one label; every voxel a root
  all ones [9, 33, 31]                          9207 voxels: no multiple of EM_CCL_RUN = 16 or of the 256-thread block
  [1, 13], [4, 1]                               degenerate dimensions
  int32 / int16 / int64 / bool, negatives,      _label_volume's conversions, int64 beyond int32, em_label's range check,
  2^32 + 1, uint8 254 / 255, strided views      nl = 255
  ten thin shapes x connectivity x spacing      lines of length 1, line counts off the 64-lane block, Z = 1 in 3-D
  speckle, diagonals                            deep envelope stacks; pop runs of many parabolas per line
  far voxels [2, 3, 1030]                       d^2 = 1058846 exactly, hd = asd = sqrt of it
  pred == gt, full volumes                      max key left at its memset 0; borders only on the volume's faces
  spacing (1, 1, 1) / 1.0                       the integer path and its workspace size
  swap / permute / flip                         relations that hold whatever the reference says
  8 classes (duplicate, 0, negative), mixed     EM_MAXCLS masks, em_eq_bits in 64-bit, the uint8 / int32 readers;
  dtypes, int64 beyond int32                    classes INT32_MIN / INT32_MAX beside labels that a clamp would move there
  workspace one byte short, on the device       PCUDA_E_WORKSPACE and no launch

Bounds (those of test_eval_metrics_gpu._check_rows, no element excused): Dice, counts and flags exact; hd exact under
unit spacing, rtol 1e-12 with spacing; asd rtol 1e-12; hd and asd NaN where a flag is set; components np.array_equal.
Every device result is computed twice and must agree bit for bit.

Self-check (run once on a scratch copy, not committed): em_unite cut down to its first atomicMin, no re-link after a
lost one (wrong values only: every loop still ends, no index leaves its range).  Failed then: hanging_comb (41 of
2664 voxels kept in one run, 822 in the next), lying_comb, and four of the five snake cases (3937 .. 5014 of 8579 in
their first run, all 8579 in their second: which hook loses is a matter of timing, hence runs=8 on these shapes).
comb and rings passed: the upright comb hooks every voxel from one side only, so no atomicMin is ever lost there, and
the 129x131 snake has just 32 voxels that are hooked from two sides (the right-hand ends of rows 2, 6, ..); the two
flipped combs, with 64 / 20 such junctions that every tooth hangs on, were added for that reason.
test_largest_components_against_the_fixture caught it as well, on labels_above_shape1.

Wall time on the MI355X: 3.4 s for the file (48 cases); the slowest case 0.24 s (snake as int64).
"""
import ctypes
import functools
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import eval_shapes as S
from conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_eval_golden", os.path.join(ROOT, "scripts", "make_eval_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

pytestmark = pytest.mark.gpu

CCL = {name: (m, kept) for name, m, kept in S.ccl_cases()}
SURF = {c[0]: c[1:] for c in S.surface_cases()}
E_WORKSPACE = -4                             # include/pcuda_hip.h: PCUDA_E_WORKSPACE


# ------------------------------------------------------------------------------------------------ helpers
def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check_rows(got, exp, name, exact_hd):
    assert np.array_equal(got[:, [0, 4, 5, 6, 7]], exp[:, [0, 4, 5, 6, 7]]), (name, got, exp)     # dice and counts: exact
    empty = exp[:, 7] != 0
    assert np.isnan(got[empty, 1:4]).all(), name
    if exact_hd:
        assert np.array_equal(got[~empty, 1], exp[~empty, 1]), (name, got[:, 1], exp[:, 1])
    else:
        assert np.allclose(got[~empty, 1], exp[~empty, 1], rtol=1e-12, atol=0), (name, got[:, 1], exp[:, 1])
    assert np.allclose(got[~empty, 2:4], exp[~empty, 2:4], rtol=1e-12, atol=0), (name, got[:, 2:4], exp[:, 2:4])


def _unit(sp):
    return sp is None or all(float(v) == 1.0 for v in (sp if hasattr(sp, "__len__") else [sp]))


def _dev(a, dev):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _surface(dev, pred, gt, cls, sp=None, conn=1):
    """K.surface_metrics on the host, computed twice: the same bits"""
    from pointcloududa_amd import kernels as K
    tp, tg = _dev(pred, dev), _dev(gt, dev)
    out = K.surface_metrics(tp, tg, cls, sp, conn)
    assert out.dtype == torch.float64 and out.is_cuda and out.shape == (len(cls), 8)
    got = out.cpu().numpy()
    again = K.surface_metrics(tp, tg, cls, sp, conn).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(again)), ("run to run", got, again)
    return got


def _components(dev, mask, runs=2):
    """K.largest_components on the host, computed ``runs`` times: the same bytes (which hook loses its atomicMin is a
    matter of timing, so the contended shapes are run more often)"""
    from pointcloududa_amd import kernels as K
    tm = _dev(mask, dev)
    out = K.largest_components(tm)
    assert out.dtype == torch.uint8 and out.is_cuda and out.shape == tm.shape
    got = out.cpu().numpy()
    for r in range(1, runs):
        again = K.largest_components(tm).cpu().numpy()
        assert np.array_equal(got, again), ("run to run", r, int(np.count_nonzero(got)), int(np.count_nonzero(again)))
    return got


@functools.lru_cache(maxsize=None)
def _ccl_ref(name, as_bool=False):
    m = CCL[name][0]
    ref = G.largest_components_brute(m.astype(bool) if as_bool else m)
    ref.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------ largest components
@pytest.mark.parametrize("name", list(CCL))
def test_largest_components_on_contended_and_thin_shapes(dev, name):
    m, kept = CCL[name]
    ref = _ccl_ref(name)
    if kept is not None:
        assert int(np.count_nonzero(ref)) == kept                       # the reference itself: the closed form
    if name == "checker":
        assert np.flatnonzero(ref).tolist() == [0, 1]
    if name == "two_snakes":
        assert ref[0].any() and not ref[2].any()                        # equal sizes: the raster-first one
    got = _components(dev, m, runs=8)
    assert np.array_equal(got, ref), (name, int(np.count_nonzero(got)), int(np.count_nonzero(ref)))


@pytest.mark.parametrize("dtype", ["int32", "int16", "int64", "bool"])
@pytest.mark.parametrize("name", ["snake", "rings"])
def test_largest_components_dtypes(dev, name, dtype):
    m = CCL[name][0]
    ref = _ccl_ref(name, as_bool=dtype == "bool")                       # bool: every ring is label 1, one component
    if dtype == "bool" and name == "rings":
        assert ref.all()
    assert np.array_equal(_components(dev, m.astype(dtype)), ref), (name, dtype)


def test_largest_components_label_range(dev):
    snake = CCL["snake"][0]
    neg = snake.astype(np.int32)
    neg[neg == 0] = -1                                                  # a connected negative background: ignored
    neg[1, :5] = -7
    neg[5, 60:70] = -2 ** 31
    assert np.array_equal(_components(dev, neg), _ccl_ref("snake"))
    wide = CCL["rings"][0].astype(np.int64)
    wide[wide == 2] = 2 ** 32 + 1                                       # not label 1 (its low 32 bits), not any label
    wide[31, 31] = -2 ** 40
    ref = G.largest_components_brute(wide)
    assert int(np.count_nonzero(ref)) == 248 and ref.max() == 1
    assert np.array_equal(_components(dev, wide), ref)
    top = np.zeros((2, 255, 3), np.uint8)                               # nl = shape[1] = 255: the whole uint8 range
    top[0, :100, 0] = 255; top[1, 200:, 2] = 255; top[0, 10:40, 2] = 254; top[1, 10:41, 1] = 254; top[0, 254, 1] = 1
    ref = G.largest_components_brute(top)
    assert sorted(np.unique(ref).tolist()) == [0, 1, 254, 255] and int((ref == 255).sum()) == 100 and int((ref == 254).sum()) == 31
    assert np.array_equal(_components(dev, top), ref)


def test_largest_components_strided_views(dev):
    from pointcloududa_amd import kernels as K
    two = CCL["two_snakes"][0]
    big = np.zeros((5, 40, 70), np.uint8)
    big[:] = S.checker(big.shape) + 2                                   # what a reader that ignored the strides would see
    big[1:4, 3:36, 1:70:2] = two
    view = torch.from_numpy(big).to(dev)[1:4, 3:36, 1:70:2]
    assert not view.is_contiguous() and tuple(view.shape) == two.shape
    got = K.largest_components(view)
    assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), _ccl_ref("two_snakes"))
    comb = CCL["comb"][0]
    tview = torch.from_numpy(np.ascontiguousarray(comb.T)).to(dev).t()  # transposed: [40, 129] with strides (1, 40)
    assert not tview.is_contiguous()
    assert np.array_equal(K.largest_components(tview).cpu().numpy(), _ccl_ref("comb"))
    assert np.array_equal(K.largest_components(tview).cpu().numpy(), K.largest_components(tview.contiguous()).cpu().numpy())


# ------------------------------------------------------------------------------------------------ surface metrics
@pytest.mark.parametrize("shape", S.DEGENERATE_SHAPES, ids=["x".join(map(str, s)) for s in S.DEGENERATE_SHAPES])
def test_surface_metrics_on_degenerate_shapes(dev, shape):
    pred, gt = S.degenerate_pair(G.blobs, shape)
    n = 0
    for conn in range(1, len(shape) + 1):
        for sp in (None, S.ANISO[-len(shape):]):
            exp = G.surface_brute(pred, gt, S.DEGENERATE_CLASSES, sp, conn)
            assert exp[3, 7] == 3 and exp[3, 0] == 0
            got = _surface(dev, pred, gt, S.DEGENERATE_CLASSES, sp, conn)
            _check_rows(got, exp, (shape, conn, sp), exact_hd=_unit(sp))
            n += 1
    assert n == 2 * len(shape)


@pytest.mark.parametrize("name", list(SURF))
def test_surface_metrics_on_deep_envelopes_and_long_distances(dev, name):
    pred, gt, cls, sp, conn = SURF[name]
    exp = G.surface_brute(pred, gt, cls, sp, conn)
    if name == "far_voxels":
        assert exp[0, 1] == exp[0, 2] == exp[0, 3] == np.sqrt(1.0 + 4.0 + 1029.0 ** 2)
    if name == "full_vs_itself":
        assert exp[0, 0] == 1.0 and (exp[0, 1:4] == 0.0).all() and exp[1, 7] == 3
    got = _surface(dev, pred, gt, cls, sp, conn)
    _check_rows(got, exp, name, exact_hd=_unit(sp))
    if name == "far_voxels":
        assert got[0, 1] == got[0, 2] == got[0, 3] == np.sqrt(1.0 + 4.0 + 1029.0 ** 2)


@pytest.mark.parametrize("sp", [None, S.ANISO], ids=["unit", "aniso"])
def test_surface_metrics_of_a_volume_with_itself(dev, sp):
    vol = G.blobs((9, 17, 19), 311, [1, 2, 3], n=6)
    cls = [1, 2, 3]
    for conn in (1, 3):
        got = _surface(dev, vol, vol, cls, sp, conn)
        assert (got[:, 7] == 0).all() and (got[:, 0] == 1.0).all()
        assert np.array_equal(_bits(got[:, 1:4]), np.zeros((3, 3), np.int64)), got     # +0.0 exactly
        _check_rows(got, G.surface_brute(vol, vol, cls, sp, conn), ("self", conn, sp), exact_hd=True)


def test_explicit_unit_spacing_takes_the_integer_path(dev):
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    for shape in ((9, 17, 19), (33, 67)):
        pred, gt = S.degenerate_pair(G.blobs, shape)
        base = _surface(dev, pred, gt, [1, 2, 3], None, 1)
        _check_rows(base, G.surface_brute(pred, gt, [1, 2, 3]), shape, exact_hd=True)
        for sp in ((1.0,) * len(shape), 1.0, 1, np.ones(len(shape))):
            assert np.array_equal(_bits(_surface(dev, pred, gt, [1, 2, 3], sp, 1)), _bits(base)), sp
        nd, shp = len(shape), (1,) * (3 - len(shape)) + shape
        ones = (ctypes.c_double * nd)(*[1.0] * nd)
        size = lib.pcuda_surface_metrics_workspace_size(nd, *shp, 3, None)
        assert size > 0 and lib.pcuda_surface_metrics_workspace_size(nd, *shp, 3, ones) == size
        off = (ctypes.c_double * nd)(*([1.0] * (nd - 1) + [1.0 + 2.0 ** -52]))
        assert lib.pcuda_surface_metrics_workspace_size(nd, *shp, 3, off) > size           # any other value: fp64 fields


def _swapped(rows):
    out = rows[:, [0, 1, 3, 2, 5, 4, 6, 7]].copy()
    f = rows[:, 7].astype(np.int64)
    out[:, 7] = ((f & 1) << 1) | ((f & 2) >> 1)
    return out


def _same_up_to_order_of_summation(a, b, exact_hd, what):
    assert np.array_equal(a[:, [0, 4, 5, 6, 7]], b[:, [0, 4, 5, 6, 7]]), what
    ok = a[:, 7] == 0
    assert np.isnan(a[~ok, 1:4]).all() and np.isnan(b[~ok, 1:4]).all(), what
    if exact_hd:
        assert np.array_equal(a[ok, 1], b[ok, 1]), (what, a[:, 1], b[:, 1])
    else:
        assert np.allclose(a[ok, 1], b[ok, 1], rtol=1e-12, atol=0), (what, a[:, 1], b[:, 1])
    assert np.allclose(a[ok, 2:4], b[ok, 2:4], rtol=1e-12, atol=0), (what, a[:, 2:4], b[:, 2:4])


@pytest.mark.parametrize("sp", [None, S.ANISO], ids=["unit", "aniso"])
def test_surface_metrics_swap_permute_flip(dev, sp):
    """relations that need no reference: classes 2 (gt side emptied), 3 (pred side emptied) and 9 carry each flag"""
    pred, gt = S.degenerate_pair(G.blobs, (9, 17, 19))
    pred, gt = pred.copy(), gt.copy()
    gt[gt == 2] = 0
    pred[pred == 3] = 0
    cls, conn = [1, 2, 3, 9], 2
    base = _surface(dev, pred, gt, cls, sp, conn)
    assert base[:, 7].tolist() == [0, 2, 1, 3]
    swapped = _surface(dev, gt, pred, cls, sp, conn)
    exp = _swapped(base)
    assert np.array_equal(_bits(swapped), _bits(exp)), (swapped, exp)   # the same lines in the same blocks: the same bits
    for perm in itertools.permutations(range(3)):
        psp = None if sp is None else tuple(sp[a] for a in perm)
        got = _surface(dev, pred.transpose(perm), gt.transpose(perm), cls, psp, conn)
        _same_up_to_order_of_summation(got, base, sp is None, ("permute", perm))
    for axis in range(3):
        got = _surface(dev, np.flip(pred, axis), np.flip(gt, axis), cls, sp, conn)
        _same_up_to_order_of_summation(got, base, sp is None, ("flip", axis))


def test_surface_metrics_eight_classes_and_mixed_dtypes(dev):
    from pointcloududa_amd import kernels as K
    shape = (7, 20, 22)
    pred, gt = G.blobs(shape, 321, [1, 2, -3, 5], n=8), G.blobs(shape, 321, [1, 2, -3, 5], n=8, shift=2)
    cls = [1, 2, 1, 0, -3, 5, 7, -1]                                    # a duplicate, background, a negative, two empty
    exp = G.surface_brute(pred, gt, cls)
    assert np.array_equal(exp[0], exp[2]) and exp[6, 7] == 3 and exp[7, 7] == 3 and not exp[:6, 7].any()
    got = _surface(dev, pred, gt, cls)
    _check_rows(got, exp, "8 classes", exact_hd=True)
    _check_rows(_surface(dev, pred, gt, cls, S.ANISO, 3), G.surface_brute(pred, gt, cls, S.ANISO, 3), "8 classes aniso", False)
    # pred uint8 with gt int32: as both int32
    p8, g8 = np.abs(pred).astype(np.uint8), np.abs(gt).astype(np.int32)
    mixed = _surface(dev, p8, g8, [1, 2, 3, 5])
    assert np.array_equal(_bits(mixed), _bits(_surface(dev, p8.astype(np.int32), g8, [1, 2, 3, 5])))
    assert np.array_equal(_bits(_surface(dev, g8, p8, [1, 2, 3, 5])), _bits(_surface(dev, g8, p8.astype(np.int32), [1, 2, 3, 5])))
    _check_rows(mixed, G.surface_brute(p8, g8, [1, 2, 3, 5]), "uint8 x int32", exact_hd=True)
    for other in (np.int16, np.int64, bool):
        pb, gb = (p8 == 1).astype(other), (g8 == 1).astype(np.uint8)
        _check_rows(_surface(dev, pb, gb, [1]), G.surface_brute(pb, gb, [1]), other, exact_hd=True)
    # int64 labels beyond int32 match no class: not 1 (low 32 bits of 2^32 + 1), not -1, not 0
    wide_p, wide_g = pred.astype(np.int64), gt.astype(np.int64)
    wide_p[pred == 2] = 2 ** 32 + 1
    wide_g[gt == 2] = 2 ** 32 + 1
    wide_p[pred == 5] = -2 ** 32 - 1
    wide_g[gt == 5] = 2 ** 32
    wide_p[0, 0, :3], wide_g[0, 0, 1:4] = 2 ** 31 - 1, 2 ** 31 - 1     # the ends of the int32 range are class values
    wide_p[6, 19, :3], wide_g[6, 19, 1:4] = -2 ** 31, -2 ** 31
    wcls = [1, 2, 0, -1, -3, 5, 2 ** 31 - 1, -2 ** 31]
    exp = G.surface_brute(wide_p, wide_g, wcls)
    assert exp[1, 7] == 3 and exp[5, 7] == 3 and np.array_equal(exp[0], G.surface_brute(pred, gt, [1])[0])
    assert exp[6, 4:7].tolist() == [3, 3, 2] and exp[7, 4:7].tolist() == [3, 3, 2]      # not the wider labels with them
    _check_rows(_surface(dev, wide_p, wide_g, wcls), exp, "int64 beyond int32", exact_hd=True)
    with pytest.raises(ValueError, match="int32"):
        K.surface_metrics(torch.from_numpy(wide_p).to(dev), torch.from_numpy(wide_g).to(dev), [1, 2 ** 32 + 1])
    # a strided view: the result of its contiguous copy
    big_p = torch.from_numpy(np.full((9, 24, 44), 1, np.int32)).to(dev)
    big_g = torch.from_numpy(np.full((9, 24, 44), 2, np.int32)).to(dev)
    vp, vg = big_p[1:8, 2:22, 0:44:2], big_g[1:8, 2:22, 0:44:2]
    vp.copy_(torch.from_numpy(pred).to(dev)); vg.copy_(torch.from_numpy(gt).to(dev))
    assert not vp.is_contiguous() and not vg.is_contiguous()
    assert np.array_equal(_bits(_surface(dev, vp, vg, cls)), _bits(got))
    assert np.array_equal(_bits(K.surface_metrics(vp, vg.contiguous(), cls).cpu().numpy()), _bits(got))
    tp = torch.from_numpy(np.ascontiguousarray(pred.transpose(2, 0, 1))).to(dev).permute(1, 2, 0)
    tg = torch.from_numpy(np.ascontiguousarray(gt.transpose(2, 0, 1))).to(dev).permute(1, 2, 0)
    assert not tp.is_contiguous() and tuple(tp.shape) == shape
    assert np.array_equal(_bits(_surface(dev, tp, tg, cls)), _bits(got))


def test_raw_entry_points_refuse_a_short_workspace_on_the_device(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd import kernels as K
    lib = _lib.lib()
    pred, gt = (torch.from_numpy(a.astype(np.uint8)).to(dev) for a in S.degenerate_pair(G.blobs, (9, 17, 19)))
    cls = (ctypes.c_int * 3)(1, 2, 3)
    out = torch.full((3, 8), -5.0, dtype=torch.float64, device=dev)
    comp = torch.full((9, 17, 19), 77, dtype=torch.uint8, device=dev)
    aniso = (ctypes.c_double * 3)(*S.ANISO)
    for sp in (None, aniso):
        need = lib.pcuda_surface_metrics_workspace_size(3, 9, 17, 19, 3, sp)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        before = K.launch_count()
        rc = lib.pcuda_surface_metrics(pred.data_ptr(), gt.data_ptr(), 0, 3, 9, 17, 19, cls, 3, 1, sp, out.data_ptr(),
                                       ws.data_ptr(), need - 1, K._stream())
        assert rc == E_WORKSPACE and b"workspace" in lib.pcuda_last_error()
        assert K.launch_count() == before
    need = lib.pcuda_largest_components_workspace_size(3, 9, 17, 19)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    before = K.launch_count()
    rc = lib.pcuda_largest_components(pred.data_ptr(), 0, 3, 9, 17, 19, 17, comp.data_ptr(), ws.data_ptr(), need - 1, K._stream())
    assert rc == E_WORKSPACE and b"workspace" in lib.pcuda_last_error()
    assert K.launch_count() == before
    torch.cuda.synchronize()
    assert bool((out == -5.0).all()) and bool((comp == 77).all())       # nothing written
    # and with the full size the same buffers serve
    need = lib.pcuda_surface_metrics_workspace_size(3, 9, 17, 19, 3, None)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    assert lib.pcuda_surface_metrics(pred.data_ptr(), gt.data_ptr(), 0, 3, 9, 17, 19, cls, 3, 1, None, out.data_ptr(),
                                     ws.data_ptr(), need, K._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(K.surface_metrics(pred, gt, [1, 2, 3]).cpu().numpy()))
    assert K.launch_count() > before
