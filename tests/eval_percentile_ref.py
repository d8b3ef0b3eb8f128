"""References and cases for the percentile Hausdorff distance (medpy's hd95) and assd of surface_metrics_ext.

  sd_brute            the distance set sd(X, Y) of scripts/make_eval_golden.py by all pairs of border voxels, numpy only
                      (border_np, footprint_offsets); integer squared distances at unit spacing
  percentile_linear   numpy.percentile's 'linear' method restated operation by operation in fp64
  hd95_ref, assd_ref  medpy's definitions from a distance-set function: G.sd (scipy) by default
  cases()             every (name, pred, gt, classes, spacing, connectivity) the two test files run

numpy only at import: the GPU tests import this file and must not need scipy (G.sd imports it lazily).
tests/test_eval_percentile.py shows, without a GPU, that G.sd, sd_brute and numpy.percentile agree on every case; the
GPU tests then hold the kernels to the brute force, as tests/test_eval_edges_gpu.py does."""
import functools
import importlib.util
import os

import numpy as np

import eval_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_eval_golden", os.path.join(ROOT, "scripts", "make_eval_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

QS = (95.0, 50.0, 99.9, 0.0, 100.0)
FAR_KEY = 1058846                            # 1 + 4 + 1029^2: the far voxels of eval_shapes


# ------------------------------------------------------------------------------------------------ references
def sd_brute(x, y, spacing=None, connectivity=1):
    """G.sd without scipy: for each border voxel of x (raster order) the distance to the nearest border voxel of y"""
    x, y = np.asarray(x, dtype=bool), np.asarray(y, dtype=bool)
    pa, pb = np.argwhere(G.border_np(x, connectivity)), np.argwhere(G.border_np(y, connectivity))
    unit = spacing is None
    sp = None if unit else np.asarray(spacing, dtype=np.float64) * np.ones(x.ndim)
    out = np.empty(len(pa), np.float64)
    step = max(1, (1 << 21) // max(1, len(pb)))
    for i in range(0, len(pa), step):
        d = pa[i:i + step, None, :] - pb[None, :, :]                    # int64
        d2 = (d * d).sum(-1) if unit else ((d * sp) ** 2).sum(-1)
        out[i:i + step] = np.sqrt(d2.min(1).astype(np.float64))
    return out


def ranks(n, q):
    """(lo, hi, t) of numpy's linear method on n values"""
    v = (n - 1) * (float(q) / 100.0)
    lo = int(np.floor(v))
    return lo, min(lo + 1, n - 1), v - lo


def percentile_linear(values, q):
    s = np.sort(np.asarray(values, dtype=np.float64))
    lo, hi, t = ranks(s.size, q)
    a, b = float(s[lo]), float(s[hi])
    if t >= 0.5:
        return b - (b - a) * (1.0 - t)
    return a + (b - a) * t


def hd95_ref(result, reference, voxelspacing=None, connectivity=1, q=95.0, sd=None):
    """medpy.metric.binary.hd95 (q = 95): numpy.percentile of the two distance sets pooled"""
    sd = sd or G.sd
    a, b = np.asarray(result) != 0, np.asarray(reference) != 0
    return float(np.percentile(np.hstack((sd(a, b, voxelspacing, connectivity), sd(b, a, voxelspacing, connectivity))), q))


def assd_ref(result, reference, voxelspacing=None, connectivity=1, sd=None):
    """medpy.metric.binary.assd: numpy.mean of the two directed asd"""
    sd = sd or G.sd
    a, b = np.asarray(result) != 0, np.asarray(reference) != 0
    return float(np.mean((sd(a, b, voxelspacing, connectivity).mean(), sd(b, a, voxelspacing, connectivity).mean())))


def class_sets(pred, gt, classes, spacing=None, connectivity=1, sd=sd_brute):
    """per class: (sd(A, B), sd(B, A), |border(A)|, |border(B)|, flags); empty distance sets where a flag is set"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    out = []
    for c in classes:
        a, b = pred == c, gt == c
        flags = (0 if a.any() else 1) | (0 if b.any() else 2)
        na, nb = int(G.border_np(a, connectivity).sum()), int(G.border_np(b, connectivity).sum())
        if flags:
            ab = ba = np.zeros(0)
        else:
            ab, ba = sd(a, b, spacing, connectivity), sd(b, a, spacing, connectivity)
            assert ab.size == na and ba.size == nb
        ab.setflags(write=False); ba.setflags(write=False)
        out.append((ab, ba, na, nb, flags))
    return out


def ext_columns(sets, q):
    """columns 8..11 of surface_metrics_ext from class_sets: percentile, assd, border counts"""
    out = np.full((len(sets), 4), np.nan)
    for k, (ab, ba, na, nb, flags) in enumerate(sets):
        out[k, 2:] = [na, nb]
        if not flags:
            out[k, 0] = percentile_linear(np.hstack((ab, ba)), q)
            out[k, 1] = float(np.mean((ab.mean(), ba.mean())))
    return out


# ------------------------------------------------------------------------------------------------ cases
def lines_pair(a, b):
    """(pred, gt): a line of a voxels and a line of b voxels, seven rows apart and offset: a + b border voxels"""
    p, g = np.zeros((12, b + 9), np.uint8), np.zeros((12, b + 9), np.uint8)
    p[2, 3:3 + a] = 1
    g[9, 5:5 + b] = 1
    return p, g


def straddle(far):
    """(pred, gt): lines of five voxels along x, pred's at x = 0..4 and gt's at 1..5, and one voxel of pred at
    (1, 2, 5 + far).  The 11 pooled keys d^2 are eight 0, two 1 and 1 + 4 + far^2 (from the far voxel to gt's
    line end): at q = 95, v = 9.5, rank lo = 9 is a key 1 and rank hi = 10 the far key, t = 0.5"""
    p, g = np.zeros((2, 3, far + 6), np.uint8), np.zeros((2, 3, far + 6), np.uint8)
    p[0, 0, 0:5] = 1
    g[0, 0, 1:6] = 1
    p[1, 2, 5 + far] = 1
    return p, g


def big_pair():
    return G.blobs((8, 96, 96), 517, [1, 2, 3]), G.blobs((8, 96, 96), 517, [1, 2, 3], shift=2)


@functools.lru_cache(maxsize=None)
def cases():
    cs = list(S.surface_cases())
    for shape in S.DEGENERATE_SHAPES:
        p, g = S.degenerate_pair(G.blobs, shape)
        tag = "deg_" + "x".join(map(str, shape))
        for conn in range(1, len(shape) + 1):
            cs.append(("%s_conn%d" % (tag, conn), p, g, [1, 2, 3], None, conn))
            cs.append(("%s_conn%d_aniso" % (tag, conn), p, g, [1, 2, 3], S.ANISO[-len(shape):], conn))
    p, g = lines_pair(10, 11)
    cs.append(("n21", p, g, [1], None, 1))
    cs.append(("n21_aniso", p, g, [1], (0.7, 1.3), 1))
    p, g = lines_pair(50, 51)
    cs.append(("n101", p, g, [1], None, 1))
    p, g = straddle(1029)
    cs.append(("straddle", p, g, [1], None, 1))
    cs.append(("straddle_aniso", p, g, [1], S.ANISO, 1))
    p, g = straddle(5000)                    # d^2 >= 2^24: the queries part at the first 8-bit digit of an int32 key too
    cs.append(("straddle_long", p, g, [1], None, 1))
    p, g = big_pair()
    cs.append(("big_8x96x96", p, g, [1, 2, 3], None, 1))
    cs.append(("big_8x96x96_aniso", p, g, [1, 2, 3], S.ANISO, 1))
    for c in cs:
        for a in c[1:3]:
            a.setflags(write=False)
    return tuple(cs)


def case(name):
    return next(c[1:] for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def case_sets(name):
    """class_sets of a case by brute force: computed once, shared, read-only"""
    pred, gt, cls, sp, conn = case(name)
    return tuple(class_sets(pred, gt, cls, sp, conn))
