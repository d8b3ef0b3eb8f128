"""Generator of tests/golden/geometric_cubic.npz: the expected values of ORDER 3 of the device-side geometric augmentation
(pointcloududa_amd/utils/geometric.py, csrc/geometric.hip through pcuda_geometric_cubic).

The rule -- the Keys cubic convolution with A = -0.75 over the 4 x 4 neighbours floor(s) - 1 .. floor(s) + 2, the border mode
folding each of the eight neighbour indices -- is restated here twice, independently of the package, on top of f8's
generator (scripts/make_geometric_golden.py: the source coordinates, the index folding, orders 0 and 1, the case inputs):

* ``backend="numpy"``: vectorised float64 in exactly the documented order of operations (what the device executes: the GPU
  tests hold the device to it bit for bit)
* ``backend="exact"``: the same float64 source coordinates, then Python ``fractions``: the weights as exact polynomials of
  ``t = s - floor(s)``, the sixteen products summed exactly, ONE rounding at the end

A value is EXCUSABLE where the exact pre-rounding value lies within 1e-9 of k + 1/2.  The builder refuses to write unless the
two restatements agree on every other value, excusable values are at most 1e-5 of all values, and no slot of a chain has one
(slots of order 0 / 1 inside a chain follow f8's restatement; an order-1 value within 1e-9 of a tie counts).  A case's input
seed is bumped until it has no excusable value at all; SEEDS records where that ended.

    python scripts/make_geometric_cubic_golden.py        # writes tests/golden/geometric_cubic.npz"""
from __future__ import annotations

import math
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import make_geometric_golden as G  # noqa: E402  (f8: coordinates, folding, orders 0 and 1, inputs)
from make_geometric_golden import (CONSTANT, EDGE, REFLECT, SYMMETRIC, WRAP, HOMOGRAPHY, NOP, Prog, exc_masks,  # noqa: E402,F401
                                   load_cases, planar)

OUT = os.path.join(ROOT, "tests", "golden", "geometric_cubic.npz")
EPS = Fraction(1, 10 ** 9)      # (sample_cubic_exact compares in integers) half-width of the excusable band around a rounding boundary
EXCUSED_CAP = 1e-5              # of all values of the case set (f8's cap)
A = -0.75                       # the constant OpenCV documents for INTER_CUBIC
K_LABELS = G.K_LABELS


# ------------------------------------------------------------------------------------------------ restatement 1: numpy
def cubic_weights(t):
    """float64 weights of the taps i0 - 1, i0, i0 + 1, i0 + 2 for the fraction t, every operation rounded on its own"""
    u = t + 1.0
    wm = ((A * u - 5.0 * A) * u + 8.0 * A) * u - 4.0 * A
    w0 = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0
    r = 1.0 - t
    w1 = ((A + 2.0) * r - (A + 3.0)) * r * r + 1.0
    w2 = ((1.0 - wm) - w0) - w1
    return wm, w0, w1, w2


def _prepare(img, lab, sx, sy):
    """f8's coordinate-safety rule and label rule (order 0, constant 0), shared by both restatements"""
    h, w, _ = img.shape
    bad = ~(np.abs(sx) <= G.COORD_LIMIT) | ~(np.abs(sy) <= G.COORD_LIMIT)
    sx, sy = np.where(bad, 0.0, sx), np.where(bad, 0.0, sy)
    xn, yn = np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64)
    lin = ~bad & (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)
    labels = np.where(lin, lab[np.clip(yn, 0, h - 1), np.clip(xn, 0, w - 1)], 0).astype(np.int64)
    return bad, sx, sy, labels


def sample_cubic_numpy(img, lab, sx, sy, mode, cval):
    """uint8 [H,W,C], int [H,W] sampled at (sx, sy) with order 3 -> (pre-rounding float64 [H,W,C], int64 labels)"""
    h, w, c = img.shape
    bad, sx, sy, labels = _prepare(img, lab, sx, sy)
    xf, yf = np.floor(sx), np.floor(sy)
    wx = [v[..., None] for v in cubic_weights(sx - xf)]
    wy = [v[..., None] for v in cubic_weights(sy - yf)]
    xa, ya = xf.astype(np.int64) - 1, yf.astype(np.int64) - 1
    fx, ix = zip(*(G.fold_index(xa + q, w, mode) for q in range(4)))
    fy, iy = zip(*(G.fold_index(ya + k, h, mode) for k in range(4)))

    def tex(k, q):
        return np.where((ix[q] & iy[k] & ~bad)[..., None], img[fy[k], fx[q]].astype(np.float64), float(cval))
    rows = [((tex(k, 0) * wx[0] + tex(k, 1) * wx[1]) + tex(k, 2) * wx[2]) + tex(k, 3) * wx[3] for k in range(4)]
    return ((rows[0] * wy[0] + rows[1] * wy[1]) + rows[2] * wy[2]) + rows[3] * wy[3], labels


# ------------------------------------------------------------------------------------------------ restatement 2: exact
_FA = Fraction(-3, 4)


def cubic_weights_exact(t: Fraction):
    """the Keys kernel k(x) (|x| <= 1: (A + 2)|x|^3 - (A + 3)|x|^2 + 1; 1 < |x| < 2: A|x|^3 - 5A|x|^2 + 8A|x| - 4A) at the four
    distances 1 + t, t, 1 - t, 2 - t: written from the kernel's definition, not from the float recipe (its fourth weight is
    1 minus the others only because the kernel is a partition of unity)"""
    def k(x):
        x = abs(x)
        if x <= 1:
            return (_FA + 2) * x ** 3 - (_FA + 3) * x ** 2 + 1
        return _FA * x ** 3 - 5 * _FA * x ** 2 + 8 * _FA * x - 4 * _FA if x < 2 else Fraction(0)
    return [k(1 + t), k(t), k(1 - t), k(2 - t)]


def _fold_scalar(i, n, mode):
    """-> (texel index, contributes its texel): plain integers"""
    if 0 <= i < n:
        return i, True
    if mode == EDGE:
        return (0 if i < 0 else n - 1), True
    if mode == REFLECT:
        p = 2 * (n - 1)
        m = i % p
        return (m if m < n else p - m), True
    if mode == SYMMETRIC:
        p = 2 * n
        m = i % p
        return (m if m < n else p - 1 - m), True
    if mode == WRAP:
        return i % n, True
    return 0, False


def _int_weights(t: Fraction):
    """the four exact weights as integer numerators over the denominator 4 q^3, t = p / q: the kernel's two cubics with
    A = -3/4 cleared of fractions (4 k(x) = 5 x^3 - 9 x^2 + 4 inside, -3 x^3 + 15 x^2 - 24 x + 12 outside); equal to
    cubic_weights_exact(t), which tests/test_geometric_cubic.py checks -- plain integers are ten times faster"""
    p, q = t.numerator, t.denominator
    q2 = q * q
    q3 = q2 * q

    def inner(a):
        return 5 * a * a * a - 9 * a * a * q + 4 * q3

    def outer(a):
        return -3 * a * a * a + 15 * a * a * q - 24 * a * q2 + 12 * q3
    return [outer(q + p), inner(p), inner(q - p), outer(2 * q - p)], 4 * q3


_EPS_DEN = 10 ** 9


def sample_cubic_exact(img, lab, sx, sy, mode, cval):
    """-> (uint8 [H,W,C] after ONE rounding floor(v + 1/2) of the exact value, clipped; bool: the exact value within EPS of
    a tie; int64 labels; the smallest and the largest exact pre-rounding value as Fractions)"""
    h, w, c = img.shape
    bad, sx, sy, labels = _prepare(img, lab, sx, sy)
    px = img.astype(np.int64).tolist()
    u8, exc = np.empty((h, w, c), dtype=np.uint8), np.zeros((h, w, c), dtype=bool)
    cval = int(cval)
    lo = hi = Fraction(int(img.flat[0]))
    for y in range(h):
        for x in range(w):
            if bad[y, x]:
                u8[y, x, :] = cval
                continue
            fsx, fsy = float(sx[y, x]), float(sy[y, x])
            x0, y0 = math.floor(fsx), math.floor(fsy)
            nx, dx = _int_weights(Fraction(fsx) - x0)
            ny, dy = _int_weights(Fraction(fsy) - y0)
            den = dx * dy
            cols = [_fold_scalar(x0 - 1 + q, w, mode) for q in range(4)]
            rws = [_fold_scalar(y0 - 1 + k, h, mode) for k in range(4)]
            for ch in range(c):
                tot = 0
                for k in range(4):
                    fy, iy = rws[k]
                    row = 0
                    for q in range(4):
                        fx, ix = cols[q]
                        row += (px[fy][fx][ch] if (ix and iy) else cval) * nx[q]
                    tot += row * ny[k]
                # v = tot / den; floor(v + 1/2) = (2 tot + den) // (2 den), the remainder tells the distance to a tie
                fl, rem = divmod(2 * tot + den, 2 * den)
                u8[y, x, ch] = min(max(fl, 0), 255)
                exc[y, x, ch] = min(rem, 2 * den - rem) * _EPS_DEN <= 2 * den      # (EPS = 1e-9 of one grey level)
                if tot < lo * den or tot > hi * den:
                    v = Fraction(tot, den)
                    lo, hi = min(lo, v), max(hi, v)
    return u8, exc, labels, lo, hi


# ------------------------------------------------------------------------------------------------ programs
def run_program(images, labels, opcode, iarg, farg, seed, backend="numpy", info=None):
    """uint8 [B,H,W,C], int [B,H,W] + a program whose slots have order 0, 1 or 3 -> (uint8 images, int64 labels, excusable
    values of the LAST active slot bool [B,H,W,C], the number of excusable values in earlier slots).  ``backend="exact"``
    restates the order-3 slots in rational arithmetic (orders 0 and 1 are f8's numpy restatement in both); only it knows
    the excusable values of an order-3 slot.  ``info``: a dict that collects the extreme pre-rounding values of order 3"""
    b, h, w, c = images.shape
    out, lab_out = np.empty_like(images), np.empty((b, h, w), dtype=np.int64)
    exc = np.zeros(images.shape, dtype=bool)
    earlier = 0
    for i in range(b):
        cur, lab = images[i], np.asarray(labels[i], dtype=np.int64)
        e = np.zeros((h, w, c), dtype=bool)
        for s in range(opcode.shape[1]):
            op = int(opcode[i, s])
            if op == NOP:
                continue
            earlier += int(e.sum())
            order, mode, cval = (int(v) for v in iarg[i, s, :3])
            sx, sy = G.source_coords(op, iarg[i, s], farg[i, s], int(seed[i, s]), h, w, "numpy")
            if order != 3:
                v, lab = G.sample_numpy(cur, lab, sx, sy, order, mode, cval)
                e = G.near_half(v) if order == 1 else np.zeros((h, w, c), dtype=bool)
                cur = G.to_u8(v) if order == 1 else v.astype(np.uint8)
            elif backend == "exact":
                cur, e, lab, lo, hi = sample_cubic_exact(cur, lab, sx, sy, mode, cval)
                if info is not None:
                    info["lo"] = min(info.get("lo", 0.0), float(lo))
                    info["hi"] = max(info.get("hi", 255.0), float(hi))
            else:
                v, lab = sample_cubic_numpy(cur, lab, sx, sy, mode, cval)
                e = np.zeros((h, w, c), dtype=bool)
                cur = G.to_u8(v)
        out[i], lab_out[i], exc[i] = cur, lab, e
    return out, lab_out, exc, earlier


def stripes_image(h, w, c):
    """uint8 [1,H,W,C] of 0 / 255 only: vertical stripes two pixels wide (top half), a checkerboard of single pixels (bottom
    half): the sharpest edges there are, so the cubic overshoots past both ends of [0, 255]"""
    yy, xx = np.mgrid[0:h, 0:w]
    plane = np.where(yy < h // 2, (xx // 2) % 2, (xx + yy) % 2).astype(np.uint8) * 255
    return np.repeat(plane[None, :, :, None], c, axis=3)


def case_inputs(case):
    b, h, w, c = (int(case[k]) for k in ("b", "h", "w", "c"))
    if case["kind"] == "stripes":
        return (np.repeat(stripes_image(h, w, c), b, axis=0),
                np.repeat(G.ellipse_labels(1, h, w, K_LABELS, int(case["seed"]) + 1000), b, axis=0))
    return G.case_inputs(case)


# input seeds that the re-seeding loop of expected() arrived at (it starts from them)
SEEDS = {}
SHAPES = G.SHAPES


def cases():
    """list of dicts: name, b, h, w, c, seed, kind, chain, prog"""
    cs = []
    rng = np.random.default_rng(20273)
    n = [0]

    def add(name, shape, c, kind, prog, chain=False):
        h, w = shape
        name = "%s_%dx%d_c%d" % (name, h, w, c)
        cs.append(dict(name=name, b=prog.opcode.shape[0], h=h, w=w, c=c, seed=SEEDS.get(name, 900 + n[0]), kind=kind, chain=chain,
                       prog=prog))
        n[0] += 1
    for (h, w), c in SHAPES:
        shape = (h, w)
        img_kind = "grey3" if c == 3 and h == 96 else ("smooth", "random")[(h == 64) & (c == 3)]
        # order 3 with each of the five modes, through affines at the ends of their ranges
        prog = Prog(5)
        for i in range(5):
            prog.homography(i, 0, G._affine_ends(rng, h, w, [((i + 3 * c) >> k) & 1 for k in range(5)]), 3, i, int(rng.integers(1, 256)))
        add("modes", shape, c, img_kind, prog)
        # a perspective close to the validity limit and a drawn one
        prog = Prog(2)
        jit = (np.array([[0.45, 0.44], [0.45, 0.43], [0.44, 0.45], [0.43, 0.45]]), rng.normal(0, 0.1, (4, 2)).clip(-0.45, 0.45))
        for i in range(2):
            prog.homography(i, 0, G.perspective(h, w, jit[i]), 3, CONSTANT, 0)
        add("perspective", shape, c, img_kind, prog)
        # a crop and a pad, one side of each axis at an end of (-0.05, 0.1); amounts as f8 chooses them (full_denominator)
        prog = Prog(2)
        (lh, hh), (lw, hw) = G.crop_pad_range(h), G.crop_pad_range(w)
        for i, (t, r, b, l) in enumerate(((lh, lw, -1, -1), (hh, hw, 1, 1))):
            prog.homography(i, 0, G.crop_and_pad(h, w, t, r, G.full_denominator(h, t, b), G.full_denominator(w, r, l)), 3, (3, 0)[i],
                            (0, 200)[i])
        add("crop_pad", shape, c, "random", prog)
        # elastic: r = 0, 1 and 4
        prog = Prog(3)
        for i, (alpha, sigma) in enumerate(((3.0, 0.1), (G._near(rng, 0.5, 3.5, 1), 0.25), (20.0, 1.0))):
            prog.elastic(i, 0, alpha, sigma, int(rng.integers(0, 2 ** 64, dtype=np.uint64)), 3, (0, 2, 4)[i], 0)
        add("elastic", shape, c, "smooth" if c == 1 else "grey3", prog)
        # piecewise: G = 2, 3 and 4
        prog = Prog(3)
        for i, (g, sc) in enumerate(((2, 0.05), (3, 0.04), (4, G._near(rng, 0.01, 0.05, 1)))):
            prog.piecewise(i, 0, h, w, rng.normal(0, sc * w, (g, g)), rng.normal(0, sc * h, (g, g)), 3, (1, 3, 0)[i], 0)
        add("piecewise", shape, c, img_kind, prog)
    # one chain that mixes the orders 0, 1 and 3
    h, w = 64, 48
    prog = Prog(2, 4)
    u = lambda lo, hi: float(rng.uniform(lo, hi))
    for i in range(2):
        aff = G.affine_inverse(h, w, u(0.8, 1.2), u(0.8, 1.2), u(-0.2, 0.2), u(-0.2, 0.2), u(-45, 45), u(-16, 16))
        slots = [lambda s: prog.homography(i, s, G.flip_lr(w), 0),
                 lambda s: prog.homography(i, s, aff, (1, 3)[i], int(rng.integers(0, 5)), int(rng.integers(0, 256))),
                 lambda s: prog.elastic(i, s, u(0.5, 3.5), 0.25, int(rng.integers(0, 2 ** 64, dtype=np.uint64)), 3),
                 lambda s: prog.piecewise(i, s, h, w, rng.normal(0, 0.03 * w, (4, 4)), rng.normal(0, 0.03 * h, (4, 4)), (3, 1)[i],
                                          int(rng.integers(0, 5)), 7)]
        for s, k in enumerate(np.roll(np.arange(4), -i)):
            slots[int(k)](s)
    add("chain", (h, w), 3, "random", prog, chain=True)
    # 0 / 255 stripes and checkerboard: both clips of round_u8 are reached (build() asserts it)
    prog = Prog(3)
    prog.homography(0, 0, G.affine_inverse(h, w, 1.07, 0.93, 0.01, -0.02, 7.0, 3.0), 3, REFLECT, 0)
    prog.elastic(1, 0, 3.5, 0.25, 20273, 3, WRAP, 0)
    prog.homography(2, 0, np.array([[1.0, 0.0, 0.37], [0.0, 1.0, 0.21], [0.0, 0.0, 1.0]]), 3, EDGE, 0)
    add("stripes", (h, w), 1, "stripes", prog)
    return cs


def _arrays(case):
    p = case["prog"]
    return p.opcode, p.iarg, p.farg, p.seed


def expected(case, info=None):
    """both restatements of a case -> dict(images, labels, u8, lab); asserts that they agree outside the excusable values.
    The input seed is bumped until no slot has an excusable value (the synthetic stripes have no seed to bump for the
    image: they must be clean as they are)"""
    for _ in range(100):
        x, lab = case_inputs(case)
        mine = {}
        a, la, ea, ma = run_program(x, lab, *_arrays(case), backend="exact", info=mine)
        n, ln, en, mn = run_program(x, lab, *_arrays(case), backend="numpy")
        e = ea | en
        assert np.array_equal(la, ln), case["name"]
        assert np.array_equal(a[~e], n[~e]), (case["name"], int((a != n)[~e].sum()))
        assert np.abs(a.astype(int) - n.astype(int)).max() <= 1, case["name"]
        if not (ma or mn or e.any()):
            if info is not None:
                info.update(mine)
            return dict(images=x, labels=lab, u8=n, lab=ln, exc=e)
        assert case["kind"] != "stripes", "the synthetic case has an excusable value"
        case["seed"] = int(case["seed"]) + 1000
    raise AssertionError("no seed without an excusable value for %s" % case["name"])


def build():
    g = {}
    tot = exc = 0
    seeds = {}
    for n, case in enumerate(cases()):
        info = {}
        r = expected(case, info)
        if case["kind"] == "stripes":
            assert info["lo"] < -0.5 and info["hi"] >= 255.5, ("both clips must be hit", info)
            g["stripes_extremes"] = np.array([info["lo"], info["hi"]], dtype=np.float64)
        seeds[case["name"]] = int(case["seed"])
        k = "c%02d_" % n
        g[k + "name"] = np.array(case["name"])
        g[k + "kind"] = np.array(case["kind"])
        g[k + "dims"] = np.array([case[s] for s in ("b", "h", "w", "c", "seed")], dtype=np.int64)
        g[k + "chain"] = np.array(bool(case["chain"]))
        g[k + "opcode"], g[k + "iarg"], g[k + "farg"], g[k + "seed"] = _arrays(case)
        g[k + "in_u8"] = planar(r["images"][:1])
        g[k + "in_lab"] = r["labels"][:1].astype(np.uint8)
        g[k + "u8"] = planar(r["u8"])
        g[k + "lab"] = r["lab"].astype(np.uint8)
        g[k + "exc"] = np.argwhere(r["exc"]).astype(np.int32).reshape(-1, 4)
        g[k + "exc_lab"] = np.zeros((0, 3), dtype=np.int32)
        tot += r["u8"].size
        exc += int(r["exc"].sum())
    assert exc <= EXCUSED_CAP * tot, (exc, tot)
    g["counts"] = np.array([tot, exc], dtype=np.int64)
    build.seeds = seeds
    return g


if __name__ == "__main__":
    g = build()
    np.savez_compressed(OUT, **g)
    moved = {k: v for k, v in build.seeds.items() if v >= 1900}
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays; values %d, excusable %d" % tuple(g["counts"]))
    print("re-seeded cases (record them in SEEDS):", moved)
