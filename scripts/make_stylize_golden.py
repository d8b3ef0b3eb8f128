"""Generator of tests/golden/stylize.npz: the expected values of the device-side stylize augmentation
(pointcloududa_amd/utils/stylize.py, csrc/stylize.hip).

The convention is restated here twice, independently of the package, as interpreters of a program's arrays (``opcode [B,S]``,
``iarg [B,S,12]``, ``farg [B,S,16]``, ``table [B,S,768]``, ``seed [B,S]`` as ``StyleProgram`` holds them):

* ``backend="numpy"``: vectorised numpy in the documented order
* ``backend="independent"``: hue / saturation and superpixels in plain Python integers, pixel by pixel; noise-alpha with
  ``scipy.ndimage.map_coordinates(order=1, mode="nearest")`` for the upscale, ``scipy.special.expit`` for the sigmoid and
  ``scipy.ndimage.correlate(mode="mirror")`` for the 3x3 kernel

Philox4x32-10, ``to_u8``, ``near_boundary``, ``dilate`` and the input kinds are f7's (make_photometric_golden.py), imported, not
copied.  Hue / saturation and superpixels are integer operators: the two interpreters agree exactly.  Noise-alpha is float64:
where the 3x3 correlation's or the blend's pre-rounding value lies within 1e-9 of a rounding boundary the pixel is EXCUSABLE
(it may differ by one grey level); in a chain a pixel whose dependency window holds such a pixel is excusable too (the window
of a superpixel slot is the whole image).  The builder asserts that the excusable pixels are at most 1e-5 of all pixels and
that the chains have none.

    python scripts/make_stylize_golden.py        # writes tests/golden/stylize.npz"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import make_photometric_golden as F7  # noqa: E402
from make_photometric_golden import EPS, EXCUSED_CAP, dilate, near_boundary, philox4x32_10, planar, to_u8  # noqa: E402,F401

OUT = os.path.join(ROOT, "tests", "golden", "stylize.npz")
NOP, HUE_SATURATION, NOISE_ALPHA, SUPERPIXELS = range(4)
NAMES = ("nop", "hue_saturation", "noise_alpha", "superpixels")
INTEGER_OPS = (NOP, HUE_SATURATION, SUPERPIXELS)
IARGS, FARGS, GRID, TABLE = 12, 16, 256, 768
KINDS = F7.KINDS + ("const", "halves")


def rdiv(a, b):
    """floor((2 a + b) / (2 b)); numpy's and Python's ``//`` floor"""
    return (2 * a + b) // (2 * b)


# ------------------------------------------------------------------------------------------------ hue / saturation
def hue_numpy(img, dh, ds):
    v = img.astype(np.int64)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    V, m = v.max(-1), v.min(-1)
    d = V - m
    S = np.where(V == 0, 0, rdiv(255 * d, np.maximum(V, 1)))
    base = np.where(V == r, 0, np.where(V == g, 60, 120))
    num = np.where(V == r, g - b, np.where(V == g, b - r, r - g))
    H = np.where(d == 0, 0, (base + rdiv(30 * num, np.maximum(d, 1))) % 180)
    H2, S2 = (H + int(dh)) % 180, np.clip(S + int(ds), 0, 255)
    sec, F = H2 // 30, H2 % 30
    p, q, t = rdiv(V * (255 - S2), 255), rdiv(V * (7650 - S2 * F), 7650), rdiv(V * (7650 - S2 * (30 - F)), 7650)
    pick = lambda opts: np.choose(sec, opts)
    out = np.stack([pick([V, q, p, p, t, V]), pick([t, V, V, q, p, p]), pick([p, p, t, V, V, q])], axis=-1)
    return out


def hue_pixel_python(r, g, b, dh, ds):
    V, m = max(r, g, b), min(r, g, b)
    d = V - m
    S = 0 if V == 0 else (2 * 255 * d + V) // (2 * V)
    if d == 0:
        H = 0
    else:
        if V == r:
            base, num = 0, g - b
        elif V == g:
            base, num = 60, b - r
        else:
            base, num = 120, r - g
        H = (base + (2 * 30 * num + d) // (2 * d)) % 180
    H2, S2 = (H + dh) % 180, min(255, max(0, S + ds))
    sec, F = divmod(H2, 30)
    p = (2 * V * (255 - S2) + 255) // 510
    q = (2 * V * (7650 - S2 * F) + 7650) // 15300
    t = (2 * V * (7650 - S2 * (30 - F)) + 7650) // 15300
    return ((V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q))[sec]


def hue_python(img, dh, ds):
    h, w, _ = img.shape
    out = np.zeros((h, w, 3), dtype=np.int64)
    px = img.tolist()
    for y in range(h):
        row = px[y]
        for x in range(w):
            out[y, x] = hue_pixel_python(row[x][0], row[x][1], row[x][2], int(dh), int(ds))
    return out


# ------------------------------------------------------------------------------------------------ noise-alpha
def _grids(ia, tb):
    out = []
    for k in range(int(ia[0])):
        h2, w2 = int(ia[4 + 2 * k]), int(ia[5 + 2 * k])
        out.append(np.asarray(tb[GRID * k:GRID * k + h2 * w2], dtype=np.float64).reshape(h2, w2))
    return out


def _upscale_numpy(g, h, w, bilinear):
    h2, w2 = g.shape
    if not bilinear:
        return g[(np.arange(h) * h2) // h][:, (np.arange(w) * w2) // w]
    sy = np.clip((np.arange(h, dtype=np.float64) + 0.5) * float(h2) / float(h) - 0.5, 0.0, float(h2 - 1))
    sx = np.clip((np.arange(w, dtype=np.float64) + 0.5) * float(w2) / float(w) - 0.5, 0.0, float(w2 - 1))
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h2 - 1), np.minimum(x0 + 1, w2 - 1)
    fy, fx = (sy - y0)[:, None], (sx - x0)[None, :]
    top = g[y0][:, x0] * (1.0 - fx) + g[y0][:, x1] * fx
    bot = g[y1][:, x0] * (1.0 - fx) + g[y1][:, x1] * fx
    return top * (1.0 - fy) + bot * fy


def _upscale_scipy(g, h, w, bilinear):
    from scipy.ndimage import map_coordinates
    h2, w2 = g.shape
    if not bilinear:
        yy = np.array([(y * h2) // h for y in range(h)], dtype=np.float64)
        xx = np.array([(x * w2) // w for x in range(w)], dtype=np.float64)
        order = 0
    else:
        yy = np.clip((np.arange(h) + 0.5) * h2 / h - 0.5, 0, h2 - 1)
        xx = np.clip((np.arange(w) + 0.5) * w2 / w - 0.5, 0, w2 - 1)
        order = 1
    cy, cx = np.meshgrid(yy, xx, indexing="ij")
    return map_coordinates(g, [cy, cx], order=order, mode="nearest")


def noise_alpha(img, ia, fa, tb, backend):
    """-> (pre-rounding values of the 3x3 correlation, pre-rounding values of the blend): float64 [H,W,C]"""
    h, w, c = img.shape
    x = img.astype(np.float64)
    bilinear, agg, sigmoid, thr = int(ia[1]) == 1, int(ia[2]), bool(ia[3]), float(fa[9])
    wts = np.asarray(fa[:9], dtype=np.float64)
    if backend == "numpy":
        ms = [_upscale_numpy(g, h, w, bilinear) for g in _grids(ia, tb)]
        m = ms[0]
        for v in ms[1:]:
            m = np.minimum(m, v) if agg == 0 else (np.maximum(m, v) if agg == 2 else m + v)
        if agg == 1:
            m = m / float(len(ms))
        if sigmoid:
            m = 1.0 / (1.0 + np.exp(-(20.0 * (m - 0.5) - thr)))
        p = np.pad(x, ((1, 1), (1, 1), (0, 0)), mode="reflect")
        t = np.zeros((h, w, c), dtype=np.float64)
        for i in range(9):
            t = t + p[i // 3:i // 3 + h, i % 3:i % 3 + w] * wts[i]
    else:
        from scipy.ndimage import correlate
        from scipy.special import expit
        ms = np.stack([_upscale_scipy(g, h, w, bilinear) for g in _grids(ia, tb)])
        m = ms.min(0) if agg == 0 else (ms.max(0) if agg == 2 else ms.mean(0))
        if sigmoid:
            m = expit(20.0 * (m - 0.5) - thr)
        t = correlate(x, wts.reshape(3, 3, 1), mode="mirror")
    e = to_u8(t).astype(np.float64)
    m = m[..., None]
    return t, (1.0 - m) * x + m * e


# ------------------------------------------------------------------------------------------------ superpixels
def threshold(p):
    return min(int(np.floor(float(p) * 2.0 ** 32)), 2 ** 32 - 1)


def slic_numpy(img, gy, gx, iters, m2):
    """the grid SLIC alone -> (labels int64 [H,W] of the last assignment, mean colours int64 [K,C], pixels per centre, centres
    without a pixel in any pass)"""
    h, w, c = img.shape
    v = img.astype(np.int64)
    k_all = gy * gx
    j, i = np.divmod(np.arange(k_all), gx)
    cy, cx = ((2 * j + 1) * h) // (2 * gy), ((2 * i + 1) * w) // (2 * gx)
    cc = v[cy, cx].copy()
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cj, ci = (yy * gy) // h, (xx * gx) // w
    s2 = max(1, (h * w) // k_all)
    empties = 0
    for it in range(iters + 1):
        best = np.full((h, w), np.iinfo(np.int64).max, dtype=np.int64)
        lab = np.zeros((h, w), dtype=np.int64)
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                jj, ii = cj + dj, ci + di
                ok = (jj >= 0) & (jj < gy) & (ii >= 0) & (ii < gx)
                k = np.where(ok, jj * gx + ii, 0)
                dist = ((v - cc[k]) ** 2).sum(-1) * s2 + m2 * ((yy - cy[k]) ** 2 + (xx - cx[k]) ** 2)
                upd = ok & (dist < best)
                best, lab = np.where(upd, dist, best), np.where(upd, k, lab)
        flat = lab.ravel()
        n = np.bincount(flat, minlength=k_all).astype(np.int64)
        has = n > 0
        empties += int((~has).sum())
        sums = np.zeros((k_all, c), dtype=np.int64)
        np.add.at(sums, flat, v.reshape(-1, c))
        cc[has] = rdiv(sums[has], n[has, None])
        if it < iters:
            sy, sx = np.zeros(k_all, dtype=np.int64), np.zeros(k_all, dtype=np.int64)
            np.add.at(sy, flat, yy.ravel())
            np.add.at(sx, flat, xx.ravel())
            cy[has], cx[has] = rdiv(sy[has], n[has]), rdiv(sx[has], n[has])
    return lab, cc, n, empties


def superpixels_numpy(img, gy, gx, iters, m2, thr, seed):
    """-> (int64 [H,W,C], pixels per centre after the last assignment, centres without a pixel in any pass)"""
    lab, cc, n, empties = slic_numpy(img, gy, gx, iters, m2)
    k_all, v = gy * gx, img.astype(np.int64)
    rep = philox4x32_10(seed, np.arange(k_all, dtype=np.uint32))[0] < np.uint32(thr) if thr else np.zeros(k_all, dtype=bool)
    return np.where(rep[lab][..., None], cc[lab], v), n, empties


def _philox_word0_python(key, c0):
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    c1 = c2 = c3 = 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def slic_python(img, gy, gx, iters, m2):
    """the grid SLIC alone in plain Python integers -> (labels: list of H W, mean colours: list of K lists, pixels per centre)"""
    h, w, c = img.shape
    px = img.reshape(h * w, c).tolist()
    k_all = gy * gx
    cy = [((2 * (k // gx) + 1) * h) // (2 * gy) for k in range(k_all)]
    cx = [((2 * (k % gx) + 1) * w) // (2 * gx) for k in range(k_all)]
    cc = [list(px[cy[k] * w + cx[k]]) for k in range(k_all)]
    s2 = max(1, (h * w) // k_all)
    lab = [0] * (h * w)
    chans = range(c)
    for it in range(iters + 1):
        n, sy, sx = [0] * k_all, [0] * k_all, [0] * k_all
        sc = [[0] * c for _ in range(k_all)]
        for y in range(h):
            cj = (y * gy) // h
            rows = [jj for jj in (cj - 1, cj, cj + 1) if 0 <= jj < gy]
            for x in range(w):
                ci = (x * gx) // w
                val = px[y * w + x]
                best, bk = None, 0
                for jj in rows:
                    for ii in (ci - 1, ci, ci + 1):
                        if ii < 0 or ii >= gx:
                            continue
                        k = jj * gx + ii
                        ck = cc[k]
                        dc2 = 0
                        for ch in chans:
                            dc2 += (val[ch] - ck[ch]) ** 2
                        dist = dc2 * s2 + m2 * ((y - cy[k]) ** 2 + (x - cx[k]) ** 2)
                        if best is None or dist < best:
                            best, bk = dist, k
                lab[y * w + x] = bk
                n[bk] += 1
                sy[bk] += y
                sx[bk] += x
                acc = sc[bk]
                for ch in chans:
                    acc[ch] += val[ch]
        for k in range(k_all):
            if n[k]:
                cc[k] = [(2 * sc[k][ch] + n[k]) // (2 * n[k]) for ch in chans]
                if it < iters:
                    cy[k], cx[k] = (2 * sy[k] + n[k]) // (2 * n[k]), (2 * sx[k] + n[k]) // (2 * n[k])
    return lab, cc, n


def superpixels_python(img, gy, gx, iters, m2, thr, seed):
    h, w, c = img.shape
    px = img.reshape(h * w, c).tolist()
    k_all = gy * gx
    lab, cc, n = slic_python(img, gy, gx, iters, m2)
    rep = [_philox_word0_python(int(seed), k) < thr for k in range(k_all)]
    out = [cc[lab[p]] if rep[lab[p]] else px[p] for p in range(h * w)]
    return np.array(out, dtype=np.int64).reshape(h, w, c), np.array(n, dtype=np.int64), None


# ------------------------------------------------------------------------------------------------ interpreter
def run_program(images, opcode, iarg, farg, table, seed, backend="numpy", info=None):
    """uint8 [B,H,W,C] + a program -> (uint8 [B,H,W,C], excusable bool [B,H,W,C]); uint8 again between two slots.  ``info``
    (a list) receives (sample, slot, pixels per centre, empty centres over the passes) of every superpixel slot."""
    out = np.empty_like(images)
    exc = np.zeros(images.shape, dtype=bool)
    for i in range(images.shape[0]):
        cur, e = images[i], np.zeros(images.shape[1:], dtype=bool)
        for s in range(opcode.shape[1]):
            op, ia, fa = int(opcode[i, s]), iarg[i, s], farg[i, s]
            if op == HUE_SATURATION:
                assert cur.shape[-1] == 3, "HUE_SATURATION takes 3 channels"
                cur = (hue_numpy if backend == "numpy" else hue_python)(cur, int(ia[0]), int(ia[1])).astype(np.uint8)
                e = dilate(e, 0, True)
            elif op == NOISE_ALPHA:
                t, v = noise_alpha(cur, ia, fa, table[i, s], backend)
                e = dilate(e, 1, False) | near_boundary(t) | near_boundary(v)
                cur = to_u8(v)
            elif op == SUPERPIXELS:
                fn = superpixels_numpy if backend == "numpy" else superpixels_python
                v, n, empties = fn(cur, int(ia[0]), int(ia[1]), int(ia[2]), int(ia[3]), threshold(fa[0]), int(seed[i, s]))
                if info is not None:
                    info.append((i, s, n, empties))
                e = np.full_like(e, bool(e.any()))      # (every pixel depends on every pixel)
                cur = v.astype(np.uint8)
            else:
                assert op == NOP, op
        out[i], exc[i] = cur, e
    return out, exc


# ------------------------------------------------------------------------------------------------ programs, cases
_F2, _G2 = 0.5 * (math.sqrt(3.0) - 1.0), (3.0 - math.sqrt(3.0)) / 6.0
_GRAD = np.array(((1.0, 0.3), (-0.3, 1.0), (-1.0, -0.3), (0.3, -1.0), (0.8, 0.7), (-0.7, 0.8), (-0.8, -0.7), (0.7, -0.8)), dtype=np.float64)


def simplex_grid(h2, w2, seed):
    """the generator's own 2-D simplex noise on the integer points (shifted by the seed's offsets), in [0, 1] (the package's
    is checked against it)"""
    off = philox4x32_10(seed, np.array([0xFFFFFFFF, 0xFFFFFFFE], dtype=np.uint32))[0]
    ox, oy = 1.0 + float(int(off[0]) & 0xFFF), 1.0 + float(int(off[1]) & 0xFFF)
    y, x = np.meshgrid(np.arange(h2, dtype=np.float64) + oy, np.arange(w2, dtype=np.float64) + ox, indexing="ij")
    s = (x + y) * _F2
    i, j = np.floor(x + s), np.floor(y + s)
    t = (i + j) * _G2
    x0, y0 = x - (i - t), y - (j - t)
    i1 = (x0 > y0).astype(np.float64)
    j1 = 1.0 - i1
    total = np.zeros((h2, w2))
    for di, dj, xk, yk in ((0.0, 0.0, x0, y0), (i1, j1, x0 - i1 + _G2, y0 - j1 + _G2), (1.0, 1.0, x0 - 1.0 + 2.0 * _G2, y0 - 1.0 + 2.0 * _G2)):
        ii, jj = (i + di).astype(np.int64), (j + dj).astype(np.int64)
        g = _GRAD[philox4x32_10(seed, (((ii & 0xFFFF) << 16) | (jj & 0xFFFF)).astype(np.uint32))[0] & np.uint32(7)]
        tt = 0.5 - xk * xk - yk * yk
        t2 = tt * tt
        total = total + np.where(tt < 0.0, 0.0, t2 * t2 * (g[..., 0] * xk + g[..., 1] * yk))
    return np.clip((70.0 * total + 1.0) * 0.5, 0.0, 1.0)


def edge(alpha):
    ident = np.zeros((3, 3)); ident[1, 1] = 1.0
    return (1.0 - alpha) * ident + alpha * np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]], dtype=np.float64)


def directed_edge(alpha, direction):
    a = 2.0 * np.pi * direction - 0.5 * np.pi
    d = np.array([np.cos(a), np.sin(a)])
    eff = np.zeros((3, 3))
    for y in (-1, 0, 1):
        for x in (-1, 0, 1):
            if x or y:
                cell = np.array([x, y], dtype=np.float64)
                ang = np.degrees(np.arccos(np.clip(np.dot(cell / np.linalg.norm(cell), d), -1.0, 1.0)))
                eff[y + 1, x + 1] = (1.0 - ang / 180.0) ** 4
    eff /= eff.sum()
    eff[1, 1] = -1.0
    ident = np.zeros((3, 3)); ident[1, 1] = 1.0
    return (1.0 - alpha) * ident + alpha * eff


class Prog:
    """the generator's own encoder of a program's arrays (the package's StyleProgram.set_* are checked against it)"""

    def __init__(self, b, slots=1):
        self.opcode = np.zeros((b, slots), dtype=np.int32)
        self.iarg = np.zeros((b, slots, IARGS), dtype=np.int32)
        self.farg = np.zeros((b, slots, FARGS), dtype=np.float64)
        self.table = np.zeros((b, slots, TABLE), dtype=np.float64)
        self.seed = np.zeros((b, slots), dtype=np.uint64)

    def put(self, i, s, op, **kw):
        self.opcode[i, s] = op
        ia, fa = self.iarg[i, s], self.farg[i, s]
        if op == HUE_SATURATION:
            ia[0], ia[1] = kw["dh"], kw["ds"]
        elif op == NOISE_ALPHA:
            sizes = kw["sizes"]
            ia[:4] = (len(sizes), kw["upscale"], kw["aggregation"], int(kw["sigmoid"]))
            for k, (h2, w2) in enumerate(sizes):
                ia[4 + 2 * k], ia[5 + 2 * k] = h2, w2
                self.table[i, s, GRID * k:GRID * k + h2 * w2] = simplex_grid(h2, w2, kw["seed"] + k).reshape(-1)
            fa[:9], fa[9] = np.asarray(kw["weights"], dtype=np.float64).reshape(9), kw["thresh"]
        elif op == SUPERPIXELS:
            ia[:4] = (kw["gy"], kw["gx"], kw["iters"], int(math.floor(kw.get("compactness", 10) ** 2 + 0.5)))
            fa[0], fa[1], self.seed[i, s] = kw["p"], kw.get("compactness", 10), kw["seed"]


def corner_slots(op, rng):
    """the parameter corners of an opcode: a list of keyword dicts, one per sample"""
    sd = lambda: int(rng.integers(0, 2 ** 63))
    if op == HUE_SATURATION:      # the ends of -20..20 (dh = floor(v 180 / 255 + 0.5)), the wrap at +/-180, a pure rotation
        return [dict(dh=-14, ds=-20), dict(dh=14, ds=20), dict(dh=180, ds=255), dict(dh=-180, ds=-255), dict(dh=60, ds=0),
                dict(dh=-7, ds=-10)]
    if op == NOISE_ALPHA:      # (alpha within 2 % of an end of 0.5..1, not the round value itself: see f7's _near)
        return [dict(sizes=[(2, 2)], upscale=0, aggregation=0, sigmoid=False, thresh=0.0, weights=edge(F7._near(rng, 0.5, 1.0, 0)), seed=sd()),
                dict(sizes=[(16, 16)] * 3, upscale=1, aggregation=1, sigmoid=True, thresh=0.0, weights=directed_edge(F7._near(rng, 0.5, 1.0, 1), 0.0), seed=sd()),
                dict(sizes=[(2, 16), (16, 2), (7, 5)], upscale=1, aggregation=2, sigmoid=True, thresh=7.3, weights=edge(F7._near(rng, 0.5, 1.0, 1)), seed=sd()),
                dict(sizes=[(3, 9), (11, 4)], upscale=0, aggregation=1, sigmoid=True, thresh=-6.1,
                     weights=directed_edge(float(rng.uniform(0.5, 1.0)), float(rng.uniform(0.0, 1.0))), seed=sd()),
                dict(sizes=[(5, 6), (16, 16)], upscale=1, aggregation=0, sigmoid=False, thresh=0.0, weights=directed_edge(F7._near(rng, 0.5, 1.0, 0), 1.0), seed=sd())]
    assert op == SUPERPIXELS
    mid = lambda: float(rng.uniform(0.3, 0.7))
    return [dict(gy=1, gx=1, iters=0, p=1.0, seed=sd()), dict(gy=1, gx=1, iters=5, p=mid(), seed=sd()),
            dict(gy=4, gx=5, iters=5, p=1.0, seed=sd()), dict(gy=4, gx=5, iters=0, p=mid(), seed=sd()),
            dict(gy=10, gx=20, iters=5, p=mid(), seed=sd()), dict(gy=10, gx=20, iters=0, p=1.0, seed=sd()),
            dict(gy=16, gx=16, iters=5, p=1.0, seed=sd()), dict(gy=16, gx=16, iters=0, p=mid(), seed=sd()),
            dict(gy=4, gx=5, iters=5, p=0.0, seed=sd())]


def random_slot(op, rng):
    sd = int(rng.integers(0, 2 ** 63))
    if op == HUE_SATURATION:
        v = int(rng.integers(-20, 21))
        return dict(dh=int(math.floor(v * 180.0 / 255.0 + 0.5)), ds=v)
    if op == NOISE_ALPHA:
        sizes = [tuple(int(q) for q in rng.integers(2, 17, 2)) for _ in range(int(rng.integers(1, 4)))]
        wts = edge(float(rng.uniform(0.5, 1))) if rng.integers(0, 2) else directed_edge(float(rng.uniform(0.5, 1)), float(rng.uniform(0, 1)))
        return dict(sizes=sizes, upscale=int(rng.integers(0, 2)), aggregation=int(rng.integers(0, 3)), sigmoid=bool(rng.integers(0, 2)),
                    thresh=float(rng.normal(0, 5)), weights=wts, seed=sd)
    gy, gx = ((4, 5), (6, 7), (10, 12))[int(rng.integers(0, 3))]
    return dict(gy=gy, gx=gx, iters=5, p=float(rng.uniform(0.2, 0.9)), seed=sd)


def cases():
    """list of dicts: name, b, h, w, c, seed, kind, chain, program"""
    cs = []
    rng = np.random.default_rng(20269)
    n = 0

    def add(op, h, w, c, kind, slots, tag=""):
        nonlocal n
        prog = Prog(len(slots), 1)
        for i, kw in enumerate(slots):
            prog.put(i, 0, op, **kw)
        cs.append(dict(name="%s_%dx%d_c%d_%s%s" % (NAMES[op], h, w, c, kind, tag), b=len(slots), h=h, w=w, c=c, seed=500 + n, kind=kind,
                       chain=False, prog=prog))
        n += 1
    for (h, w), kind in (((64, 48), "random"), ((64, 48), "grey3"), ((96, 80), "smooth")):
        slots = corner_slots(HUE_SATURATION, rng)
        add(HUE_SATURATION, h, w, 3, kind, slots if h == 64 else slots[:3])
    for (h, w), c, kind in (((64, 48), 1, "random"), ((64, 48), 3, "grey3"), ((64, 48), 3, "random"), ((96, 80), 1, "smooth"),
                            ((96, 80), 3, "smooth")):
        slots = corner_slots(NOISE_ALPHA, rng)
        add(NOISE_ALPHA, h, w, c, kind, slots if h == 64 else slots[1:4])
    for (h, w), c, kind in (((64, 48), 1, "smooth"), ((64, 48), 3, "random"), ((64, 48), 3, "grey3"), ((96, 80), 1, "random"),
                            ((96, 80), 3, "smooth"), ((50, 70), 1, "random"), ((50, 70), 3, "smooth")):
        slots = corner_slots(SUPERPIXELS, rng)
        if (h, w) == (96, 80):
            slots = [slots[1], slots[2], slots[4], slots[7]]
        elif (h, w) == (50, 70):
            slots = [slots[0], slots[2], slots[4], slots[6], slots[3]]
        add(SUPERPIXELS, h, w, c, kind, slots)
    sd = lambda: int(rng.integers(0, 2 ** 63))
    # a constant image: every dc2 is zero, ties decide
    add(SUPERPIXELS, 64, 48, 3, "const", [dict(gy=4, gx=5, iters=5, p=1.0, seed=sd()), dict(gy=16, gx=16, iters=5, p=0.5, seed=sd()),
                                          dict(gy=10, gx=20, iters=0, p=1.0, seed=sd())])
    # compactness 0 on an image whose right half is constant: the centres there tie, the lowest k takes every pixel and the
    # others end without one (build() asserts it)
    add(SUPERPIXELS, 64, 48, 3, "halves", [dict(gy=4, gx=5, iters=5, p=1.0, compactness=0, seed=sd()),
                                           dict(gy=10, gx=20, iters=5, p=1.0, compactness=0, seed=sd())], "_empty")
    # chains mixing the three opcodes, every sample its own order
    pool = [HUE_SATURATION, NOISE_ALPHA, SUPERPIXELS]
    for j, ((h, w), kind) in enumerate((((96, 80), "grey3"), ((64, 48), "smooth"), ((64, 48), "random"))):
        b, slots = 3, 4
        prog = Prog(b, slots)
        for i in range(b):
            ops = list(np.roll(pool, -(i + j))) + [pool[(2 * i + j) % 3]]
            for s, op in enumerate(ops):
                prog.put(i, s, int(op), **random_slot(int(op), rng))
        cs.append(dict(name="chain%d_%dx%d_c3_%s" % (j, h, w, kind), b=b, h=h, w=w, c=3, seed=600 + j, kind=kind, chain=True, prog=prog))
    return cs


def make_images(kind, b, h, w, c, seed):
    """uint8 [B,H,W,C] of an input kind, from a seed (numpy only): f7's three kinds, a constant image, and an image whose
    left half is random and whose right half is constant"""
    if kind == "const":
        return np.full((b, h, w, c), 117, dtype=np.uint8)
    if kind == "halves":
        x = np.random.default_rng(seed).integers(0, 256, (b, h, w, c), dtype=np.uint8)
        x[:, :, w // 2:] = 90
        return x
    return F7.make_images(kind, b, h, w, c, seed)


def case_inputs(case):
    return make_images(case["kind"], *(int(case[k]) for k in ("b", "h", "w", "c", "seed")))


def _arrays(case):
    p = case["prog"]
    return p.opcode, p.iarg, p.farg, p.table, p.seed


def check_restatement(case_list=None):
    """the independent interpreter against the vectorised one on every case: integer operators identical, noise-alpha
    identical outside the excusable set and within one grey level inside it, excusable pixels at most EXCUSED_CAP of all
    pixels.  -> (pixels, excused)"""
    tot = exc = 0
    for case in case_list or cases():
        x = case_inputs(case)
        a, ea = run_program(x, *_arrays(case), backend="independent")
        n, en = run_program(x, *_arrays(case), backend="numpy")
        e = ea | en
        if np.all(np.isin(case["prog"].opcode, INTEGER_OPS)):
            assert not e.any() and np.array_equal(a, n), (case["name"], int((a != n).sum()))
        assert not ((a != n) & ~e).any(), (case["name"], int(((a != n) & ~e).sum()))
        assert np.abs(a.astype(int) - n.astype(int)).max() <= 1, case["name"]
        tot += a.size
        exc += int(e.sum())
    assert exc <= EXCUSED_CAP * tot, (exc, tot)
    return tot, exc


def build():
    g = {}
    tot = exc = 0
    for n, case in enumerate(cases()):
        info = []
        out, e = run_program(case_inputs(case), *_arrays(case), backend="numpy", info=info)
        k = "c%02d_" % n
        g[k + "name"] = np.array(case["name"])
        g[k + "kind"] = np.array(case["kind"])
        g[k + "dims"] = np.array([case[s] for s in ("b", "h", "w", "c", "seed")], dtype=np.int64)
        g[k + "chain"] = np.array(bool(case["chain"]))
        g[k + "opcode"], g[k + "iarg"], g[k + "farg"], g[k + "table"], g[k + "seed"] = _arrays(case)
        g[k + "u8"] = planar(out)       # stored [B,C,H,W]: the planes compress better than interleaved channels
        g[k + "exc"] = np.argwhere(e).astype(np.int32).reshape(-1, 4)
        g[k + "empty"] = np.array(sum(int((q[2] == 0).sum()) for q in info), dtype=np.int64)      # centres without a pixel at the end
        if case["chain"]:
            assert not e.any(), "pick another seed: the chains are meant to have no excusable pixel (%s)" % case["name"]
        if np.all(np.isin(case["prog"].opcode, INTEGER_OPS)):
            assert not e.any(), case["name"]
        if case["name"].endswith("_empty"):
            assert all((q[2] == 0).any() for q in info) and info, "the empty-centre case has no empty centre"
        tot += out.size
        exc += int(e.sum())
    assert exc <= EXCUSED_CAP * tot, (exc, tot)
    return g


def load_cases(g):
    """the cases of a loaded fixture: dicts with the program arrays, the expected images ([B,H,W,C] again) and ``exc``"""
    out = []
    for k in sorted(f[:-4] for f in g.files if f.endswith("_name")):
        b, h, w, c, seed = (int(v) for v in g[k + "dims"])
        out.append(dict(name=str(g[k + "name"]), kind=str(g[k + "kind"]), b=b, h=h, w=w, c=c, seed=seed, chain=bool(g[k + "chain"]),
                        opcode=g[k + "opcode"], iarg=g[k + "iarg"], farg=g[k + "farg"], table=g[k + "table"], seed_arr=g[k + "seed"],
                        exc=g[k + "exc"], empty=int(g[k + "empty"]), u8=np.ascontiguousarray(np.moveaxis(g[k + "u8"], 1, -1))))
    return out


if __name__ == "__main__":
    print("restatement: %d pixels, %d excusable" % check_restatement())
    g = build()
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays")
