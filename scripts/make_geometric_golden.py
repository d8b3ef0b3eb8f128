"""Generator of tests/golden/geometric.npz: the expected values of the device-side geometric augmentation
(pointcloududa_amd/utils/geometric.py, csrc/geometric.hip).

The convention is restated here twice, independently of the package, as interpreters of a program's arrays
(``opcode [B,S]``, ``iarg [B,S,4]``, ``farg [B,S,32]``, ``seed [B,S]`` as ``GeoProgram`` holds them):

* ``backend="scipy"``: ``scipy.ndimage.map_coordinates(float64, (sy, sx), order 0 / 1, prefilter=False)`` with the modes
  ``grid-constant``, ``nearest``, ``mirror``, ``reflect``, ``grid-wrap``; the elastic blur through ``scipy.ndimage.correlate1d``
  (``mode="mirror"``)
* ``backend="numpy"``: explicit index folding in integers and sums in the documented order; needs no scipy (the GPU tests
  use it at the production size)

Both compute a slot's source coordinates with the arithmetic DESIGN.md f8 writes down and share f7's plain-numpy
Philox4x32-10 (scripts/make_photometric_golden.py).  scipy folds the COORDINATE into the image before it takes neighbours,
the convention folds each neighbour INDEX: the two agree up to rounding in the last bits, so a pixel is EXCUSABLE only where
the pre-rounding value (order 1) lies within 1e-9 of k + 1/2, or where a source coordinate (order 0, labels) lies within
1e-9 of a half-integer.  The builder asserts that the two restatements agree on every other pixel, that excusable pixels
are at most 1e-5 of all pixels, and that no intermediate slot of a chain has one (a chain's input seed is bumped until that
holds).  The fixture stores inputs, programs, expected images and labels (uint8), the excusable pixels and the counts.

    python scripts/make_geometric_golden.py        # writes tests/golden/geometric.npz"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from make_augment_golden import ellipse_labels  # noqa: E402  (f6's label maps; numpy only)
from make_photometric_golden import _symmetric_pass, gaussian_weights, make_images, philox4x32_10  # noqa: E402  (f7)

OUT = os.path.join(ROOT, "tests", "golden", "geometric.npz")
EPS = 1e-9                      # half-width of the excusable band around a rounding boundary
EXCUSED_CAP = 1e-5              # of all pixels of the case set
NOP, HOMOGRAPHY, ELASTIC, PIECEWISE = range(4)
NAMES = ("nop", "homography", "elastic", "piecewise_affine")
CONSTANT, EDGE, REFLECT, SYMMETRIC, WRAP = range(5)
SCIPY_MODES = ("grid-constant", "nearest", "mirror", "reflect", "grid-wrap")
IARGS, FARGS = 4, 32
COORD_LIMIT = 2.0 ** 30
K_LABELS = 5


# ------------------------------------------------------------------------------------------------ coordinates
def elastic_noise(seed, h, w):
    """float64 [2,H,W]: 2 u - 1 with u = (word + 0.5) 2^-32, words 0 (dx) and 1 (dy) at counter = y W + x"""
    x0, x1, _, _ = philox4x32_10(seed, np.arange(h * w, dtype=np.uint32).reshape(h, w))
    return np.stack([2.0 * ((x.astype(np.float64) + 0.5) * 2.0 ** -32) - 1.0 for x in (x0, x1)])


def source_coords(op, ia, fa, seed, h, w, backend="numpy"):
    """one slot -> float64 (sx, sy) [H,W], the arithmetic in the documented order"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if op == HOMOGRAPHY:
        m = np.asarray(fa[:9], dtype=np.float64)
        d = (m[6] * xx + m[7] * yy) + m[8]
        with np.errstate(divide="ignore", invalid="ignore"):
            return ((m[0] * xx + m[1] * yy) + m[2]) / d, ((m[3] * xx + m[4] * yy) + m[5]) / d
    if op == ELASTIC:
        r = int(ia[3])
        alpha, wts = float(fa[0]), np.asarray(fa[1:2 + r], dtype=np.float64)
        n = elastic_noise(seed, h, w)
        if backend == "scipy":
            from scipy.ndimage import correlate1d
            full = np.concatenate([wts[:0:-1], wts])
            b = [correlate1d(correlate1d(n[k], full, axis=0, mode="mirror"), full, axis=1, mode="mirror") for k in range(2)]
        else:
            b = [_symmetric_pass(_symmetric_pass(n[k], wts, 0), wts, 1) for k in range(2)]
        return xx + alpha * b[0], yy + alpha * b[1]
    if op == PIECEWISE:
        g = int(ia[3])
        xi, yi = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
        cj = np.minimum((xi * (g - 1)) // (w - 1), g - 2)
        ci = np.minimum((yi * (g - 1)) // (h - 1), g - 2)
        u = ((xi * (g - 1) - cj * (w - 1)).astype(np.float64) / float(w - 1))[None, :]
        v = ((yi * (g - 1) - ci * (h - 1)).astype(np.float64) / float(h - 1))[:, None]
        out = []
        for k in range(2):
            p = np.asarray(fa[16 * k:16 * k + g * g], dtype=np.float64).reshape(g, g)
            tl, tr = p[ci][:, cj], p[ci][:, cj + 1]
            bl, br = p[ci + 1][:, cj], p[ci + 1][:, cj + 1]
            upper = (tl + u * (tr - tl)) + v * (br - tr)
            lower = (tl + u * (br - bl)) + v * (bl - tl)
            out.append(np.where(u >= v, upper, lower))
        return out[0], out[1]
    assert op == NOP, op
    return xx, yy


# ------------------------------------------------------------------------------------------------ sampling
def fold_index(i, n, mode):
    """integer neighbour indices -> (the texel index inside [0, n), whether the neighbour contributes its texel)"""
    i = np.asarray(i, dtype=np.int64)
    inside = np.ones(i.shape, dtype=bool)
    if mode == EDGE:
        return np.clip(i, 0, n - 1), inside
    if mode == REFLECT:
        p = 2 * (n - 1)
        m = np.mod(i, p)
        return np.where(m < n, m, p - m), inside
    if mode == SYMMETRIC:
        p = 2 * n
        m = np.mod(i, p)
        return np.where(m < n, m, p - 1 - m), inside
    if mode == WRAP:
        return np.mod(i, n), inside
    return np.clip(i, 0, n - 1), (i >= 0) & (i < n)


def near_half(s):
    """bool: s + 1/2 within EPS of an integer (a coordinate where floor(s + 0.5) may pick the neighbour, or a
    pre-rounding value where floor(v + 0.5) may)"""
    return np.abs((s + 0.5) - np.round(s + 0.5)) <= EPS


def sample_numpy(img, lab, sx, sy, order, mode, cval):
    """uint8 [H,W,C], int [H,W] sampled at (sx, sy) -> (pre-rounding float64 [H,W,C] for order 1 or the int64 texels for
    order 0, int64 labels)"""
    h, w, c = img.shape
    bad = ~(np.abs(sx) <= COORD_LIMIT) | ~(np.abs(sy) <= COORD_LIMIT)
    sx, sy = np.where(bad, 0.0, sx), np.where(bad, 0.0, sy)
    xn, yn = np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64)
    lin = ~bad & (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)
    labels = np.where(lin, lab[np.clip(yn, 0, h - 1), np.clip(xn, 0, w - 1)], 0).astype(np.int64)
    if order == 0:
        fx, ix = fold_index(xn, w, mode)
        fy, iy = fold_index(yn, h, mode)
        ok = (ix & iy & ~bad)[..., None]
        return np.where(ok, img[fy, fx].astype(np.int64), int(cval)), labels
    xf, yf = np.floor(sx), np.floor(sy)
    wx1, wy1 = (sx - xf)[..., None], (sy - yf)[..., None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    xa, ya = xf.astype(np.int64), yf.astype(np.int64)

    def tex(dy, dx):
        fx, ix = fold_index(xa + dx, w, mode)
        fy, iy = fold_index(ya + dy, h, mode)
        return np.where((ix & iy & ~bad)[..., None], img[fy, fx].astype(np.float64), float(cval))
    v = np.zeros((h, w, c), dtype=np.float64)
    v = v + tex(0, 0) * wy0 * wx0
    v = v + tex(0, 1) * wy0 * wx1
    v = v + tex(1, 0) * wy1 * wx0
    v = v + tex(1, 1) * wy1 * wx1
    return v, labels


def sample_scipy(img, lab, sx, sy, order, mode, cval):
    from scipy.ndimage import map_coordinates
    h, w, c = img.shape
    bad = ~(np.abs(sx) <= COORD_LIMIT) | ~(np.abs(sy) <= COORD_LIMIT)
    co = np.stack([np.where(bad, 0.0, sy), np.where(bad, 0.0, sx)])
    v = np.stack([map_coordinates(img[..., ch].astype(np.float64), co, output=np.float64, order=int(order),
                                  mode=SCIPY_MODES[mode], cval=float(cval), prefilter=False) for ch in range(c)], axis=-1)
    v = np.where(bad[..., None], float(cval), v)
    labels = map_coordinates(lab.astype(np.float64), co, output=np.float64, order=0, mode="grid-constant", cval=0.0,
                             prefilter=False)
    labels = np.where(bad, 0, labels).astype(np.int64)
    return (np.round(v).astype(np.int64) if order == 0 else v), labels


def to_u8(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def run_program(images, labels, opcode, iarg, farg, seed, backend="numpy"):
    """uint8 [B,H,W,C], int [B,H,W] + a program -> (uint8 images, int64 labels, excusable images bool [B,H,W,C], excusable
    labels bool [B,H,W] -- both of the LAST active slot --, the number of excusable pixels in earlier slots); uint8 again
    between two slots"""
    b, h, w, c = images.shape
    out, lab_out = np.empty_like(images), np.empty((b, h, w), dtype=np.int64)
    exc, exc_lab = np.zeros(images.shape, dtype=bool), np.zeros((b, h, w), dtype=bool)
    earlier = 0
    sample = sample_scipy if backend == "scipy" else sample_numpy
    for i in range(b):
        cur, lab = images[i], np.asarray(labels[i], dtype=np.int64)
        e, el = np.zeros((h, w, c), dtype=bool), np.zeros((h, w), dtype=bool)
        for s in range(opcode.shape[1]):
            op = int(opcode[i, s])
            if op == NOP:
                continue
            earlier += int(e.sum()) + int(el.sum())
            order, mode, cval = (int(v) for v in iarg[i, s, :3])
            sx, sy = source_coords(op, iarg[i, s], farg[i, s], int(seed[i, s]), h, w, backend)
            v, lab = sample(cur, lab, sx, sy, order, mode, cval)
            el = near_half(sx) | near_half(sy)
            if order == 0:
                e = np.broadcast_to(el[..., None], (h, w, c)).copy()
                cur = v.astype(np.uint8)
            else:
                e = near_half(v)
                cur = to_u8(v)
        out[i], lab_out[i], exc[i], exc_lab[i] = cur, lab, e, el
    return out, lab_out, exc, exc_lab, earlier


# ------------------------------------------------------------------------------------------------ programs, cases
class Prog:
    """the generator's own encoder of a program's arrays (the package's GeoProgram.set_* are checked against it)"""

    def __init__(self, b, slots=1):
        self.opcode = np.zeros((b, slots), dtype=np.int32)
        self.iarg = np.zeros((b, slots, IARGS), dtype=np.int32)
        self.farg = np.zeros((b, slots, FARGS), dtype=np.float64)
        self.seed = np.zeros((b, slots), dtype=np.uint64)

    def homography(self, i, s, m, order=1, mode=CONSTANT, cval=0):
        self.opcode[i, s] = HOMOGRAPHY
        self.iarg[i, s] = (order, mode, cval, 0)
        self.farg[i, s, :9] = np.asarray(m, dtype=np.float64).reshape(9)

    def elastic(self, i, s, alpha, sigma, seed, order=1, mode=CONSTANT, cval=0):
        wts = gaussian_weights(sigma) if int(4.0 * sigma + 0.5) > 0 else np.ones(1)
        self.opcode[i, s] = ELASTIC
        self.iarg[i, s] = (order, mode, cval, len(wts) - 1)
        self.farg[i, s, 0], self.farg[i, s, 1:1 + len(wts)], self.farg[i, s, 31] = alpha, wts, sigma
        self.seed[i, s] = seed

    def piecewise(self, i, s, h, w, dx, dy, order=1, mode=CONSTANT, cval=0):
        g = np.asarray(dx).shape[0]
        k = np.arange(g, dtype=np.float64)
        self.opcode[i, s] = PIECEWISE
        self.iarg[i, s] = (order, mode, cval, g)
        self.farg[i, s, :g * g] = ((k * (w - 1.0) / (g - 1.0))[None, :] + np.asarray(dx, dtype=np.float64)).reshape(-1)
        self.farg[i, s, 16:16 + g * g] = ((k * (h - 1.0) / (g - 1.0))[:, None] + np.asarray(dy, dtype=np.float64)).reshape(-1)


def _t(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype=np.float64)


def affine_inverse(h, w, scale_x=1.0, scale_y=1.0, translate_x=0.0, translate_y=0.0, rotate=0.0, shear=0.0):
    """f6's convention: A = T(c + (tx W, ty H)) . R(rotate) . Sh(shear) . S(sx, sy) . T(-c), c = ((W-1)/2, (H-1)/2); the
    inverse with the last row set to (0, 0, 1)"""
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    th, sh = math.radians(rotate), math.radians(shear)
    rot = np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]])
    shm = np.array([[1, math.tan(sh), 0], [0, 1, 0], [0, 0, 1]])
    scm = np.diag([float(scale_x), float(scale_y), 1.0])
    fwd = _t(cx + translate_x * w, cy + translate_y * h) @ rot @ shm @ scm @ _t(-cx, -cy)
    return np.vstack([np.linalg.inv(fwd)[:2], [0.0, 0.0, 1.0]])


def flip_lr(w):
    return np.array([[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def flip_ud(h):
    return np.array([[1.0, 0.0, 0.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]])


def crop_and_pad(h, w, top, right, bottom, left):
    """sx = (x + 0.5) (W + l + r) / W - 0.5 - l, y likewise: signed pixels, positive pads"""
    ax, ay = (w + float(left) + float(right)) / w, (h + float(top) + float(bottom)) / h
    return np.array([[ax, 0.0, 0.5 * ax - 0.5 - float(left)], [0.0, ay, 0.5 * ay - 0.5 - float(top)], [0.0, 0.0, 1.0]])


def perspective(h, w, jitter):
    """the output's corners TL, TR, BR, BL -> the corners moved inward by |jitter| (fractions of W, H); h8 = 1"""
    j = np.abs(np.asarray(jitter, dtype=np.float64)).reshape(4, 2)
    xo, yo = [0.0, w - 1.0, w - 1.0, 0.0], [0.0, 0.0, h - 1.0, h - 1.0]
    xs = [j[0, 0] * w, w - 1.0 - j[1, 0] * w, w - 1.0 - j[2, 0] * w, j[3, 0] * w]
    ys = [j[0, 1] * h, j[1, 1] * h, h - 1.0 - j[2, 1] * h, h - 1.0 - j[3, 1] * h]
    a, rhs = np.zeros((8, 8)), np.zeros(8)
    for k in range(4):
        a[2 * k] = [xo[k], yo[k], 1, 0, 0, 0, -xs[k] * xo[k], -xs[k] * yo[k]]
        a[2 * k + 1] = [0, 0, 0, xo[k], yo[k], 1, -ys[k] * xo[k], -ys[k] * yo[k]]
        rhs[2 * k], rhs[2 * k + 1] = xs[k], ys[k]
    return np.append(np.linalg.solve(a, rhs), 1.0).reshape(3, 3)


def crop_pad_range(size):
    """signed pixels of the percent range (-0.05, 0.1) of data_generator_mscmrseg.py:29: floor(percent size + 0.5)"""
    return int(np.floor(-0.05 * size + 0.5)), int(np.floor(0.1 * size + 0.5))


def full_denominator(size, first, second):
    """the second amount of an axis moved as little as possible inside the range so that size + first + second shares no
    factor with 2 size.  The resize's interpolation weights are then odd multiples of 1 / (2 size), not of a small
    denominator: with a few distinct weights a bilinear sum of integers lands EXACTLY on k + 1/2 at one pixel in a few
    hundred, which is an excusable pixel by the rule below"""
    lo, hi = crop_pad_range(size)
    for k in range(hi - lo + 1):
        for cand in (second + k, second - k):
            if lo <= cand <= hi and cand != 0 and math.gcd(size + first + cand, 2 * size) == 1:
                return cand
    raise AssertionError((size, first, second))


SHAPES = (((64, 48), 1), ((64, 48), 3), ((96, 80), 1), ((96, 80), 3))


def _near(rng, lo, hi, end):
    """a continuous parameter within 2 % of an end of its range (not the round value itself)"""
    t = rng.uniform(0.0, 0.02)
    return lo + t * (hi - lo) if end == 0 else hi - t * (hi - lo)


def _affine_ends(rng, h, w, ends):
    ex, ey, et, er, es = ends
    return affine_inverse(h, w, _near(rng, 0.8, 1.2, ex), _near(rng, 0.8, 1.2, ey), _near(rng, -0.2, 0.2, et),
                          _near(rng, -0.2, 0.2, 1 - et), _near(rng, -45, 45, er), _near(rng, -16, 16, es))


def _random_slot(prog, i, s, kind, rng, h, w):
    """one slot of a chain, parameters from the reference's ranges"""
    u = lambda lo, hi: float(rng.uniform(lo, hi))
    order, mode, cval = int(rng.integers(0, 2)), int(rng.integers(0, 5)), int(rng.integers(0, 256))
    if kind == "flip_lr":
        prog.homography(i, s, flip_lr(w), 0)
    elif kind == "flip_ud":
        prog.homography(i, s, flip_ud(h), 0)
    elif kind == "affine":
        prog.homography(i, s, affine_inverse(h, w, u(0.8, 1.2), u(0.8, 1.2), u(-0.2, 0.2), u(-0.2, 0.2), u(-45, 45), u(-16, 16)),
                        order, mode, cval)
    elif kind == "crop_pad":
        t, r, b, l = (int(np.floor(u(-0.05, 0.1) * n + 0.5)) for n in (h, w, h, w))
        prog.homography(i, s, crop_and_pad(h, w, t, r, full_denominator(h, t, b), full_denominator(w, r, l)), 1, mode, cval)
    elif kind == "perspective":
        prog.homography(i, s, perspective(h, w, rng.normal(0, u(0.01, 0.1), (4, 2)).clip(-0.45, 0.45)), 1, CONSTANT, 0)
    elif kind == "elastic":
        prog.elastic(i, s, u(0.5, 3.5), 0.25, int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
    else:
        assert kind == "piecewise", kind
        sc = u(0.01, 0.05)
        prog.piecewise(i, s, h, w, rng.normal(0, sc * w, (4, 4)), rng.normal(0, sc * h, (4, 4)))


# input seeds that the re-seeding loop of expected() arrived at (it starts from them, so a rebuild takes seconds)
SEEDS = {"crop_pad_64x48_c1": 1502, "crop_pad_96x80_c3": 267520, "chain0_96x80_c1": 1524, "chain1_64x48_c3": 7525}
CHAIN_KINDS = ("flip_lr", "flip_ud", "affine", "crop_pad", "perspective", "elastic", "piecewise")


def cases():
    """list of dicts: name, b, h, w, c, seed, kind, chain, prog"""
    cs = []
    rng = np.random.default_rng(20268)
    n = [0]

    def add(name, shape, c, kind, prog, chain=False):
        h, w = shape
        name = "%s_%dx%d_c%d" % (name, h, w, c)
        cs.append(dict(name=name, b=prog.opcode.shape[0], h=h, w=w, c=c, seed=SEEDS.get(name, 500 + n[0]), kind=kind, chain=chain,
                       prog=prog))
        n[0] += 1
    for (h, w), c in SHAPES:
        shape = (h, w)
        img_kind = "grey3" if c == 3 and h == 96 else ("smooth", "random")[(h == 64) & (c == 3)]
        # every mode x order through one generic affine per sample
        # (on the large size every mode once, the order alternating: the fixture stays under 1 MB)
        prog = Prog(10 if h == 64 else 5)
        for i in range(prog.opcode.shape[0]):
            prog.homography(i, 0, _affine_ends(rng, h, w, [(i >> k) & 1 for k in range(5)]), i % 2, i // 2 if h == 64 else i,
                            int(rng.integers(1, 256)))
        add("modes", shape, c, img_kind, prog)
        # the affine at the ends of its ranges (the other corners), the flips, the identity
        prog = Prog(5 if h == 64 else 3)
        for i, ends in enumerate(((1, 1, 1, 1, 1), (0, 0, 0, 0, 0), (1, 0, 1, 0, 1))):
            prog.homography(i, 0, _affine_ends(rng, h, w, ends), 1 - i % 2, CONSTANT, (0, 255, 77)[i])
        if h == 64:
            prog.homography(3, 0, flip_lr(w), 0)
            prog.homography(4, 0, flip_ud(h), 0)
        add("affine_flips", shape, c, "smooth", prog)
        # a crop, a pad and (on the small size) a mix, one side of each axis at an end of (-0.05, 0.1)
        prog = Prog(3 if h == 64 else 2)
        (lh, hh), (lw, hw) = crop_pad_range(h), crop_pad_range(w)
        for i, (t, r, b, l) in enumerate(((lh, lw, -1, -1), (hh, hw, 1, 1), (lh, hw, hh, lw))[:prog.opcode.shape[0]]):
            prog.homography(i, 0, crop_and_pad(h, w, t, r, full_denominator(h, t, b), full_denominator(w, r, l)), 1, (3, 0, 4)[i],
                            (0, 200, 0)[i])
        # (uniform random texels: on a smooth image, whose neighbours differ by a few grey levels, the resize's rational
        # weights put one value in a thousand exactly on k + 1/2)
        add("crop_pad", shape, c, "random", prog)
        # perspective: close to the validity limit, both ends of the scale range
        prog = Prog(3)
        jit = (np.array([[0.45, 0.44], [0.45, 0.43], [0.44, 0.45], [0.43, 0.45]]), rng.normal(0, 0.1, (4, 2)).clip(-0.45, 0.45),
               rng.normal(0, 0.01, (4, 2)))
        for i in range(3):
            prog.homography(i, 0, perspective(h, w, jit[i]), 1, CONSTANT, 0)
        add("perspective", shape, c, img_kind, prog)
        # elastic: r = 0, 1, 4 and both ends of alpha
        prog = Prog(4)
        for i, (alpha, sigma) in enumerate(((_near(rng, 0.5, 3.5, 1), 0.25), (_near(rng, 0.5, 3.5, 0), 0.25), (3.0, 0.1), (20.0, 1.0))):
            prog.elastic(i, 0, alpha, sigma, int(rng.integers(0, 2 ** 64, dtype=np.uint64)), 1 - i // 3, (0, 0, 2, 4)[i], 0)
        add("elastic", shape, c, "smooth" if c == 1 else "grey3", prog)
        # piecewise: G = 2, 3, 4 and both ends of the scale
        prog = Prog(4)
        for i, (g, sc) in enumerate(((4, _near(rng, 0.01, 0.05, 1)), (4, _near(rng, 0.01, 0.05, 0)), (3, 0.04), (2, 0.05))):
            prog.piecewise(i, 0, h, w, rng.normal(0, sc * w, (g, g)), rng.normal(0, sc * h, (g, g)), 1 - i // 3, (0, 0, 3, 1)[i], 0)
        add("piecewise", shape, c, img_kind, prog)
    # chains of 4-5 slots, every sample its own order
    for j, ((h, w), c, kind, slots) in enumerate((((96, 80), 1, "random", 5), ((64, 48), 3, "random", 4), ((64, 48), 1, "random", 5))):
        prog = Prog(3, slots)
        for i in range(3):
            # (one crop / pad per chain: each adds a few exact ties per thousand values, and a chain is to have none)
            pool = [k for k in CHAIN_KINDS if k != "crop_pad" or i == j % 3]
            kinds = rng.permutation(pool)[:slots] if (i + j) % 2 else np.roll(pool, -(2 * i + 3 * j))[:slots]
            if i == j % 3 and "crop_pad" not in kinds:
                kinds[-1] = "crop_pad"
            for s, k in enumerate(kinds):
                _random_slot(prog, i, s, str(k), rng, h, w)
        add("chain%d" % j, (h, w), c, kind, prog, chain=True)
    return cs


def case_inputs(case):
    """(uint8 images [B,H,W,C], int64 labels [B,H,W]) of a case, rebuilt from its seed (numpy only): every sample of a case
    warps the SAME image and label map (the fixture stores them once)"""
    b, h, w, c, seed = (int(case[k]) for k in ("b", "h", "w", "c", "seed"))
    return (np.repeat(make_images(case["kind"], 1, h, w, c, seed), b, axis=0),
            np.repeat(ellipse_labels(1, h, w, K_LABELS, seed + 1000), b, axis=0))


def _arrays(case):
    p = case["prog"]
    return p.opcode, p.iarg, p.farg, p.seed


def expected(case):
    """both restatements of a case -> dict(images, labels, u8, lab, exc, exc_lab); asserts that they agree outside the
    excusable pixels.  The input seed is bumped until a chain has no excusable pixel in any slot, and until any other case
    has at most one"""
    for attempt in range(1000):
        x, lab = case_inputs(case)
        a, la, ea, ela, ma = run_program(x, lab, *_arrays(case), backend="scipy")
        n, ln, en, eln, mn = run_program(x, lab, *_arrays(case), backend="numpy")
        e, el = ea | en, ela | eln
        if case["chain"] and (ma or mn or e.any() or el.any()):      # (an excusable pixel of an earlier slot spreads)
            case["seed"] = int(case["seed"]) + 1000
            continue
        assert np.array_equal(a[~e], n[~e]), (case["name"], int((a != n)[~e].sum()))
        assert np.abs(a.astype(int) - n.astype(int)).max() <= 1, case["name"]
        assert np.array_equal(la[~el], ln[~el]), (case["name"], int((la != ln)[~el].sum()))
        if int(e.sum()) + int(el.sum()) <= 1:
            return dict(images=x, labels=lab, u8=a, lab=la, exc=e, exc_lab=el)
        case["seed"] = int(case["seed"]) + 1000      # re-seed
    raise AssertionError("no seed without an excusable pixel for %s" % case["name"])


def build():
    g = {}
    tot = exc = 0
    for n, case in enumerate(cases()):
        r = expected(case)
        k = "c%02d_" % n
        g[k + "name"] = np.array(case["name"])
        g[k + "kind"] = np.array(case["kind"])
        g[k + "dims"] = np.array([case[s] for s in ("b", "h", "w", "c", "seed")], dtype=np.int64)
        g[k + "chain"] = np.array(bool(case["chain"]))
        g[k + "opcode"], g[k + "iarg"], g[k + "farg"], g[k + "seed"] = _arrays(case)
        g[k + "in_u8"] = planar(r["images"][:1])      # stored [1,C,H,W]: the planes compress better than interleaved channels
        g[k + "in_lab"] = r["labels"][:1].astype(np.uint8)
        g[k + "u8"] = planar(r["u8"])
        g[k + "lab"] = r["lab"].astype(np.uint8)
        g[k + "exc"] = np.argwhere(r["exc"]).astype(np.int32).reshape(-1, 4)
        g[k + "exc_lab"] = np.argwhere(r["exc_lab"]).astype(np.int32).reshape(-1, 3)
        tot += r["u8"].size + r["lab"].size
        exc += int(r["exc"].sum()) + int(r["exc_lab"].sum())
    assert exc <= EXCUSED_CAP * tot, (exc, tot)
    g["counts"] = np.array([tot, exc], dtype=np.int64)
    return g


def planar(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, 1))


def load_cases(g):
    """the cases of a loaded fixture: dicts with the inputs, the program arrays, the expected images ([B,H,W,C] again) and
    labels, and the excusable pixels as index arrays"""
    out = []
    for k in sorted(f[:-4] for f in g.files if f.endswith("_name")):
        b, h, w, c, seed = (int(v) for v in g[k + "dims"])
        out.append(dict(name=str(g[k + "name"]), kind=str(g[k + "kind"]), b=b, h=h, w=w, c=c, seed=seed, chain=bool(g[k + "chain"]),
                        opcode=g[k + "opcode"], iarg=g[k + "iarg"], farg=g[k + "farg"], seed_arr=g[k + "seed"],
                        images=np.ascontiguousarray(np.repeat(np.moveaxis(g[k + "in_u8"], 1, -1), b, axis=0)),
                        labels=np.repeat(g[k + "in_lab"].astype(np.int64), b, axis=0),
                        u8=np.ascontiguousarray(np.moveaxis(g[k + "u8"], 1, -1)), lab=g[k + "lab"].astype(np.int64),
                        exc=g[k + "exc"], exc_lab=g[k + "exc_lab"]))
    return out


def exc_masks(case):
    """the excusable pixels of a loaded case as bool arrays (images [B,H,W,C], labels [B,H,W])"""
    e, el = np.zeros(case["u8"].shape, dtype=bool), np.zeros(case["lab"].shape, dtype=bool)
    e[tuple(case["exc"].T)] = True
    el[tuple(case["exc_lab"].T)] = True
    return e, el


if __name__ == "__main__":
    g = build()
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays; pixels %d, excusable %d" % tuple(g["counts"]))
