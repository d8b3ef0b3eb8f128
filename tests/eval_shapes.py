"""Label volumes that stress the evaluation kernels where compact blobs do not: long thin components that wind through
many workgroups (union-find contention), borders on every voxel (deep lower-envelope stacks), diagonals (long pop
runs), distances near the largest a volume allows.  numpy only: the GPU tests import this file, and so does the child
process of tests/test_eval_metrics.py that checks the scipy restatement against brute force on the same cases."""
import numpy as np


def snake(h, w):
    """a boustrophedon path: even rows full, odd rows one linking voxel at alternating ends (right first): one
    component whose raster-first voxel is the far end of the path from its last row"""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    m[1::4, w - 1] = 1
    m[3::4, 0] = 1
    return m


def comb(h, w):
    """row 0 plus every second column: the teeth meet only in row 0"""
    m = np.zeros((h, w), np.uint8)
    m[0] = 1
    m[:, 0::2] = 1
    return m


def rings(n):
    """concentric square rings, labels 1 and 2 alternating from the outside in: nested components of one label"""
    i = np.arange(n)
    d = np.minimum(i, n - 1 - i)
    return (1 + np.minimum(d[:, None], d[None, :]) % 2).astype(np.uint8)


def checker(shape):
    """labels 1 + (sum of indices) % 2: every voxel is a component of its own"""
    return (1 + sum(np.ogrid[tuple(slice(0, s) for s in shape)]) % 2).astype(np.uint8)


def diagonals(h, w):
    """(pred, gt): the main diagonal and the anti-diagonal"""
    i = np.arange(min(h, w))
    p, g = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    p[i, i] = 1
    g[i, w - 1 - i] = 1
    return p, g


def speckle(shape, p, seed):
    """every voxel 1 with probability p: almost every voxel is its own border"""
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def far_voxels(shape):
    """(pred, gt): one voxel each, in opposite corners"""
    p, g = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    p[(0,) * len(shape)] = 1
    g[tuple(s - 1 for s in shape)] = 1
    return p, g


def two_snakes(joined=False):
    """[3, 33, 35]: a snake in plane 0, its vertical mirror in plane 2, plane 1 empty (or one voxel joining them)"""
    m = np.zeros((3, 33, 35), np.uint8)
    m[0] = snake(33, 35)
    m[2] = snake(33, 35)[::-1]
    if joined:
        m[1, 0, 0] = 1
    return m


ANISO = (2.5, 1.0, 0.7)
DEGENERATE_SHAPES = ((1, 70), (70, 1), (3, 65), (65, 3), (33, 67), (1, 9, 65), (5, 1, 66), (7, 65, 1), (3, 33, 67),
                     (9, 17, 19))
DEGENERATE_CLASSES = [1, 2, 3, 9]            # 9: empty on both sides


def degenerate_pair(blobs, shape):
    """(pred, gt) of the degenerate-shape sweep; ``blobs`` is scripts/make_eval_golden.py's"""
    seed = 300 + DEGENERATE_SHAPES.index(tuple(shape))
    return blobs(shape, seed, [1, 2, 3], n=6), blobs(shape, seed, [1, 2, 3], n=6, shift=2)


def ccl_cases():
    """(name, uint8 mask, voxels kept or None) for largest_components; nl = shape[1]"""
    ones = np.ones((9, 33, 31), np.uint8)
    return [("snake", snake(129, 131), 8579),
            ("two_snakes", two_snakes(), 611),
            ("joined_snakes", two_snakes(True), 1223),
            ("comb", comb(40, 129), None),
            # teeth up / to the left: each junction voxel is hooked by its upper and its left neighbour at once, and
            # either hook is the only link of its side (the comb above has one hook per voxel: no lost atomicMin)
            ("hanging_comb", np.ascontiguousarray(comb(40, 129)[::-1]), 40 * 65 + 64),
            ("lying_comb", np.ascontiguousarray(comb(129, 40).T[::-1, ::-1]), 20 * 129 + 20),
            ("rings", rings(63), 488),
            ("checker", checker((5, 6, 7)), 2),
            ("all_ones", ones, ones.size),
            ("single_row", np.ones((1, 13), np.uint8), None),
            ("single_column", np.ones((4, 1), np.uint8), None)]


def surface_cases():
    """(name, pred, gt, classes, spacing, connectivity) beyond the degenerate-shape sweep"""
    cs = []
    for shape, p, seed in (((5, 33, 35), 0.15, 401), ((33, 67), 0.4, 403)):
        a, b = speckle(shape, p, seed), speckle(shape, p, seed + 1)
        tag = "speckle_%s" % "x".join(map(str, shape))
        cs.append((tag, a, b, [1], None, 1))
        cs.append((tag + "_aniso", a, b, [1], ANISO[-len(shape):], 1))
    p, g = diagonals(65, 67)
    cs.append(("diagonals_conn1", p, g, [1], None, 1))
    cs.append(("diagonals_conn2_aniso", p, g, [1], (0.7, 1.3), 2))
    p, g = far_voxels((2, 3, 1030))
    cs.append(("far_voxels", p, g, [1], None, 1))
    full = np.ones((6, 17, 19), np.uint8)
    one = np.zeros_like(full)
    one[2, 5, 11] = 1
    cs.append(("full_vs_itself", full, full, [1, 0], None, 1))
    cs.append(("full_vs_voxel", full, one, [1, 0], None, 1))
    cs.append(("full_vs_voxel_aniso_conn3", full, one, [1, 0], ANISO, 3))
    return cs
