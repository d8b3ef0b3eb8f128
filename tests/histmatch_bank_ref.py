"""Plain numpy restatement of the sorted-plane rule of csrc/histmatch_bank.hip, and the inputs the
CPU and the GPU tests of the reference bank share.  Not a test module.

fp32, per image plane of N values against a reference plane of M values: ``k`` = the reference's sorted order-preserving keys,
``val(key)`` the float the key came from widened to float64, ``E(p) = float64(p) / float64(M)``, ``q = float64(cnt) /
float64(N)`` with ``cnt`` = the number of plane values <= the value:

1. ``e* = max{e in [0, M] : E(e) <= q}``, by the division itself (``int(q M)`` is a first guess, its neighbours are tested)
2. ``p = e*`` if ``e* == 0``, ``e* == M`` or ``k[e*-1] != k[e*]``, else ``lower_bound(k, k[e*])``
3. ``p == 0``: ``val(k[0])``;  4. ``p == M``: ``val(k[M-1])``
5. ``q0 = E(p)``, ``v0 = val(k[p-1])``; ``q0 == q``: ``v0``; else ``p1 = upper_bound(k, k[p])``, ``q1 = E(p1)``, ``v1 = val(k[p])``,
   ``slope = (v1 - v0) / (q1 - q0)``, ``r = slope (q - q0) + v0``
6. ``float32(r)``

uint8: the image plane's 256-bin histogram and its scan give ``q`` per bin; the reference plane's 256 counts, scanned and
compacted to the bins that are not empty, are ``tq`` / ``tv``; np.interp's arithmetic written out; truncation into a LUT."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_module():
    """scripts/make_match_hist_golden.py (match_unique, match_sorted, the input generators, bit_equal)"""
    gen = os.path.join(ROOT, "scripts", "make_match_hist_golden.py")
    sys.path.insert(0, os.path.dirname(gen))
    try:
        spec = importlib.util.spec_from_file_location("make_match_hist_golden", gen)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(os.path.dirname(gen))
    return m


G = golden_module()


# ---------------------------------------------------------------------------------------------- the rule
def float_key(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0                                              # -0.0 == +0.0
    return np.where(u & 0x80000000 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_value(k):
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k & 0x80000000 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


def e_star_guess(q, m):
    """the first guess alone: trunc(q M), clamped"""
    return np.clip((np.asarray(q, dtype=np.float64) * np.float64(m)).astype(np.int64), 0, m)


def e_star(q, m):
    """step 1: the guess, then its neighbours tested with the division (two steps up, two steps down)"""
    q, dm = np.asarray(q, dtype=np.float64), np.float64(m)
    e = e_star_guess(q, m)
    for _ in range(2):
        e = e + ((e < m) & ((np.minimum(e + 1, m)).astype(np.float64) / dm <= q))
    for _ in range(2):
        e = e - ((e > 0) & (e.astype(np.float64) / dm > q))
    return e


def e_star_brute(q, m):
    """the definition, by testing every e (scalars)"""
    return max(e for e in range(m + 1) if np.float64(e) / np.float64(m) <= q)


def plane_f32(s, t):
    """float32 result of one fp32 image plane ``s`` against one fp32 reference plane ``t`` (any shapes): steps 1 to 6"""
    sk = float_key(s.ravel())
    cnt = np.searchsorted(np.sort(sk), sk, side="right")
    q = cnt.astype(np.float64) / np.float64(sk.size)
    k = np.sort(float_key(t.ravel()))
    m, dm = k.size, np.float64(k.size)
    e = e_star(q, m)
    ka, kb = k[np.maximum(e - 1, 0)], k[np.minimum(e, m - 1)]
    inside = (e > 0) & (e < m) & (ka == kb)
    p = np.where(inside, np.searchsorted(k, kb, side="left"), e)
    k0, k1 = k[np.maximum(p - 1, 0)], k[np.minimum(p, m - 1)]
    v0, v1, q0 = key_value(k0), key_value(k1), p.astype(np.float64) / dm
    q1 = np.searchsorted(k, k1, side="right").astype(np.float64) / dm
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        slope = (v1 - v0) / (q1 - q0)
        r = slope * (q - q0) + v0
    r = np.where(p == 0, v1, np.where((p == m) | (q0 == q), v0, r))
    return r.astype(np.float32).reshape(s.shape)


def plane_u8(s, t):
    """uint8 result of one uint8 image plane against one uint8 reference plane: the 256-count form"""
    cnt = np.cumsum(np.bincount(s.ravel(), minlength=256))
    q = cnt.astype(np.float64) / np.float64(s.size)
    tc = np.bincount(t.ravel(), minlength=256)
    cum, full = np.cumsum(tc), tc != 0
    tq, tv = cum[full].astype(np.float64) / np.float64(t.size), np.flatnonzero(full).astype(np.float64)
    n = len(tv)
    j = np.searchsorted(tq, q, side="right") - 1
    j0 = np.clip(j, 0, n - 1)
    j1 = np.minimum(j0 + 1, n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (tv[j1] - tv[j0]) / (tq[j1] - tq[j0])
        r = slope * (q - tq[j0]) + tv[j0]
    r = np.where((j < 0) | (j >= n - 1) | (tq[j0] == q), tv[j0], r)
    lut = np.clip(r, 0.0, 255.0).astype(np.int64).astype(np.uint8)             # truncation toward zero
    return lut[s]


def match_bank(images, references, index):
    """[B,H,W,C] images against references[index[i]] per sample, by the rule above"""
    images, references = np.asarray(images), np.asarray(references)
    fn = plane_u8 if images.dtype == np.uint8 else plane_f32
    out = np.empty_like(images)
    for b in range(images.shape[0]):
        for c in range(images.shape[-1]):
            out[b, ..., c] = fn(images[b, ..., c], references[index[b], ..., c])
    return out


def expected(images, references, index):
    """the two restatements of scripts/make_match_hist_golden.py, sample by sample with references[index[i]] + 0.0 (a
    reference's -0.0 is read as +0.0); they must agree with each other"""
    rows = []
    for b in range(images.shape[0]):
        ref = references[index[b]] + 0 if references.dtype == np.uint8 else references[index[b]] + np.float32(0.0)
        one = G.match_unique(images[b:b + 1], ref)
        assert G.bit_equal(one, G.match_sorted(images[b:b + 1], ref)), "the two restatements disagree"
        rows.append(one)
    return np.concatenate(rows, axis=0)


# ---------------------------------------------------------------------------------------------- inputs
def finite_key_coverage(shape, seed):
    """key_coverage_f32 without its infinities (non-finite REFERENCE values are unsupported on the bank path)"""
    v = G.key_coverage_f32(shape, seed)
    return np.where(np.isinf(v), np.copysign(np.float32(3e38), v), v).astype(np.float32)


def f32_set(count, h, w, c, seed, finite):
    """``count`` fp32 [h,w,c] images taking turns: normal, 37 levels (heavy ties), key coverage"""
    gens = (lambda s: G.normal_f32((h, w, c), s, 3.0, 10.0), lambda s: G.levels_f32((h, w, c), s),
            lambda s: finite_key_coverage((h, w, c), s) if finite else G.key_coverage_f32((h, w, c), s))
    return np.stack([gens[i % 3](seed + i) for i in range(count)], axis=0)


IMAGE_SHAPES = {"one_tile_64x64x1": (3, 64, 64, 1), "tile_plus_1_17x241x1": (3, 17, 241, 1), "c2_63x65x2": (3, 63, 65, 2),
                "below_a_tile_31x33x1": (3, 31, 33, 1), "several_tiles_b2_257x130x1": (2, 257, 130, 1)}
REF_PLANES = ((64, 64), (31, 33), (17, 241), (32, 64))


def f32_pairings(name):
    """(images, references, index) of one image shape against every reference plane: M != N except 64x64 against 64x64"""
    b, h, w, c = IMAGE_SHAPES[name]
    seed = 100 + 10 * sorted(IMAGE_SHAPES).index(name)
    images = f32_set(b, h, w, c, seed, finite=False)
    if b == 2:
        images = images[[1, 0]].copy()                                     # (levels first: both generators with ties and keys)
        images[1] = G.key_coverage_f32((h, w, c), seed + 7)
    out = []
    for i, (rh, rw) in enumerate(REF_PLANES):
        if rh * rw == h * w and (h, w) != (64, 64):
            continue
        refs = f32_set(3, rh, rw, c, seed + 50 + i, finite=True)
        index = [(j + i) % 3 for j in range(b)]
        out.append((images, refs, index))
    return out


def floor_guess_misses(limit=512):
    """(N, M, cnt) with N, M <= limit where trunc(q M) alone is not e*"""
    found = []
    n = np.repeat(np.arange(1, limit + 1), np.arange(1, limit + 1))            # every (n, cnt) with 1 <= cnt <= n
    cnt = np.concatenate([np.arange(1, i + 1) for i in range(1, limit + 1)])
    q = cnt.astype(np.float64) / n.astype(np.float64)
    for m in range(1, limit + 1):
        dm = np.float64(m)
        g = e_star_guess(q, m)
        miss = ((g < m) & (np.minimum(g + 1, m).astype(np.float64) / dm <= q)) | ((g > 0) & (g.astype(np.float64) / dm > q))
        found.extend((int(n[i]), m, int(cnt[i])) for i in np.flatnonzero(miss))
    return found
