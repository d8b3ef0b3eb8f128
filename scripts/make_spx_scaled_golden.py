"""Generator of tests/golden/spx_scaled.npz and tests/golden/spx_scaled_edges.json: the expected values of superpixels at a
working size (pointcloududa_amd/utils/stylize.py ``max_size``, csrc/spx_scale.hip).

The rule (integers only, this build's own; imgaug, cv2 and skimage are not installed, parity with imgaug's ``max_size=128``
path -- its resize, its working size and its shortcut for an image without a replaced segment -- is unpinned).  ``iarg[6] = m``
of a SUPERPIXELS slot; the slot is scaled iff ``m >= 1`` and ``L = max(H, W) > m``, else it is make_spx_connect_golden.py's slot:

1. working size ``h' = max(1, (H m) // L)``, ``w' = max(1, (W m) // L)``
2. linear resize ``R(src[Sh x Sw x C] -> Dh x Dw)``, per axis with source size S, destination size D, destination index d:
   ``a = clip((2 d + 1) S - D, 0, 2 D (S - 1))``, ``i0 = a // (2 D)``, ``t = a - 2 D i0``, ``i1 = min(i0 + 1, S - 1)``;
   ``num = (2 Dh - ty) ((2 Dw - tx) p00 + tx p01) + ty ((2 Dw - tx) p10 + tx p11)``, ``den = 4 Dh Dw``, value =
   ``floor((2 num + den) / (2 den))``
3. ``small = R(slot input -> h' x w')``; the grid SLIC runs on ``small`` with ``h', w'`` in place of ``H, W``; ``iarg[5] >= 1``
   runs the connectivity rule on the working-size label plane (ids and Philox counters ``r = y w' + x``); the repaint over
   the pixels of ``small`` gives ``painted``
4. ``out = R(painted -> H x W)``, unless no final segment that holds a pixel is replaced: then the output is the slot's input

restated twice, independently:

* ``numpy``: int64 arrays; the resize as a sum of four taps with the weights ``(2 Dh - ty) (2 Dw - tx)``, ``(2 Dh - ty) tx``,
  ``ty (2 Dw - tx)``, ``ty tx``; make_stylize_golden.py's ``slic_numpy`` and make_spx_connect_golden.py's ``connect_numpy``
* ``independent``: plain Python integers, pixel by pixel, the resize in the nested form of the rule; ``slic_python`` and
  ``connect_python``

``main`` refuses to write unless the two agree bit for bit on every case, and asserts the resize's anchors: equal sizes
return the input, an exact 2x shrink is ``rdiv(2x2 sum, 4)``, a constant stays constant, the values stay inside the input's
range.  (A float64 restatement of the same formula is NOT equivalent: on the 11 x 16 -> 40 x 56 enlargement of the first case
it differs by one grey level on a handful of values, ties decided by rounding error; ``float_mismatches`` counts them.)

    python scripts/make_spx_scaled_golden.py        # writes the two files"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import make_spx_connect_golden as F9B  # noqa: E402
import make_stylize_golden as F9  # noqa: E402
from make_stylize_golden import HUE_SATURATION, NOISE_ALPHA, SUPERPIXELS, Prog, dilate, philox4x32_10, planar, rdiv, threshold  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spx_scaled.npz")
OUT_EDGES = os.path.join(ROOT, "tests", "golden", "spx_scaled_edges.json")


def working_size(h, w, m):
    """(h', w'): the slot is scaled iff m >= 1 and max(h, w) > m, else (h, w)"""
    big = max(h, w)
    if m < 1 or big <= m:
        return h, w
    return max(1, (h * m) // big), max(1, (w * m) // big)


def is_scaled(h, w, m):
    return m >= 1 and max(h, w) > m


# ------------------------------------------------------------------------------------------------ the resize, twice
def _taps_numpy(s, d):
    a = np.clip((2 * np.arange(d, dtype=np.int64) + 1) * s - d, 0, 2 * d * (s - 1))
    i0 = a // (2 * d)
    return i0, np.minimum(i0 + 1, s - 1), a - 2 * d * i0


def resize_numpy(src, dh, dw):
    """[Sh,Sw,C] of integers -> int64 [dh,dw,C]: four taps, four weights"""
    sh, sw, _ = src.shape
    v = src.astype(np.int64)
    y0, y1, ty = _taps_numpy(sh, dh)
    x0, x1, tx = _taps_numpy(sw, dw)
    wy1, wx1 = ty[:, None, None], tx[None, :, None]
    wy0, wx0 = 2 * dh - wy1, 2 * dw - wx1
    num = (wy0 * wx0) * v[y0][:, x0] + (wy0 * wx1) * v[y0][:, x1] + (wy1 * wx0) * v[y1][:, x0] + (wy1 * wx1) * v[y1][:, x1]
    den = 4 * dh * dw
    return (2 * num + den) // (2 * den)


def resize_python(src, dh, dw):
    """the same in plain Python integers, pixel by pixel, in the nested form"""
    sh, sw, c = src.shape
    px = src.tolist()
    den = 4 * dh * dw
    out = []
    for y in range(dh):
        ay = min(max((2 * y + 1) * sh - dh, 0), 2 * dh * (sh - 1))
        y0 = ay // (2 * dh)
        ty, y1 = ay - 2 * dh * y0, min(y0 + 1, sh - 1)
        row = []
        for x in range(dw):
            ax = min(max((2 * x + 1) * sw - dw, 0), 2 * dw * (sw - 1))
            x0 = ax // (2 * dw)
            tx, x1 = ax - 2 * dw * x0, min(x0 + 1, sw - 1)
            p00, p01, p10, p11 = px[y0][x0], px[y0][x1], px[y1][x0], px[y1][x1]
            val = []
            for ch in range(c):
                num = (2 * dh - ty) * ((2 * dw - tx) * p00[ch] + tx * p01[ch]) + ty * ((2 * dw - tx) * p10[ch] + tx * p11[ch])
                val.append((2 * num + den) // (2 * den))
            row.append(val)
        out.append(row)
    return np.array(out, dtype=np.int64).reshape(dh, dw, c)


def resize_float(src, dh, dw):
    """float64 restatement of the same formula (NOT the rule: shown to differ, see the module docstring)"""
    sh, sw, _ = src.shape
    v = src.astype(np.float64)
    sy = np.clip((np.arange(dh) + 0.5) * sh / dh - 0.5, 0, sh - 1)
    sx = np.clip((np.arange(dw) + 0.5) * sw / dw - 0.5, 0, sw - 1)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
    fy, fx = (sy - y0)[:, None, None], (sx - x0)[None, :, None]
    top = v[y0][:, x0] * (1 - fx) + v[y0][:, x1] * fx
    bot = v[y1][:, x0] * (1 - fx) + v[y1][:, x1] * fx
    return np.floor(top * (1 - fy) + bot * fy + 0.5).astype(np.int64)


def check_resize_anchors():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
    for fn in (resize_numpy, resize_python):
        assert np.array_equal(fn(x, 12, 10), x), "equal sizes return the input"
        two = x.astype(np.int64).reshape(6, 2, 5, 2, 3).sum((1, 3))
        assert np.array_equal(fn(x, 6, 5), rdiv(two, 4)), "an exact 2x shrink is rdiv(2x2 sum, 4)"
        assert np.all(fn(np.full((7, 9, 2), 201, dtype=np.uint8), 20, 3) == 201), "a constant stays constant"
        for dh, dw in ((40, 56), (5, 3), (1, 1), (12, 31)):
            y = fn(x, dh, dw)
            assert y.min() >= x.min() and y.max() <= x.max()
    assert np.array_equal(resize_numpy(x, 29, 33), resize_python(x, 29, 33))


def float_mismatches():
    """values of the first case's 11 x 16 -> 40 x 56 enlargement on which the float64 restatement differs"""
    small = resize_numpy(F9B._noisy("smooth", 40, 56, 3, 900), 11, 16)
    a, b = resize_numpy(small, 40, 56), resize_float(small, 40, 56)
    assert np.abs(a - b).max() <= 1
    return int((a != b).sum()), int(a.size)


# ------------------------------------------------------------------------------------------------ a scaled slot, twice
def scaled_slot(cur, ia, thr, seed, backend="numpy", info=None):
    """uint8 [H,W,C] through a scaled SUPERPIXELS slot -> uint8 [H,W,C]"""
    h, w, _ = cur.shape
    hs, ws = working_size(h, w, int(ia[6]))
    gy, gx, iters, m2, min_size = (int(v) for v in (ia[0], ia[1], ia[2], ia[3], ia[5]))
    k_all = gy * gx
    if backend == "numpy":
        small = resize_numpy(cur, hs, ws).astype(np.uint8)
        if min_size > 0:
            lab = F9.slic_numpy(small, gy, gx, iters, m2)[0]
            v, fin, _ = F9B.connect_numpy(small, lab, min(min_size, hs * ws), thr, seed)
            seg = np.unique(fin)
            flag = bool(thr) and bool(np.any(philox4x32_10(seed, seg.astype(np.uint32))[0] < np.uint32(thr)))
        else:
            v, n, _ = F9.superpixels_numpy(small, gy, gx, iters, m2, thr, seed)
            rep = philox4x32_10(seed, np.arange(k_all, dtype=np.uint32))[0] < np.uint32(thr) if thr else np.zeros(k_all, dtype=bool)
            flag = bool(np.any(rep & (n > 0)))
        out = resize_numpy(v.astype(np.uint8), h, w).astype(np.uint8) if flag else cur
    else:
        small = resize_python(cur, hs, ws).astype(np.uint8)
        if min_size > 0:
            lab = F9.slic_python(small, gy, gx, iters, m2)[0]
            v, fin = F9B.connect_python(small, lab, min(min_size, hs * ws), thr, seed)
            flag = any(F9._philox_word0_python(int(seed), f) < thr for f in sorted(set(fin.ravel().tolist())))
        else:
            v, n, _ = F9.superpixels_python(small, gy, gx, iters, m2, thr, seed)
            flag = any(int(n[k]) > 0 and F9._philox_word0_python(int(seed), k) < thr for k in range(k_all))
        out = resize_python(v.astype(np.uint8), h, w).astype(np.uint8) if flag else cur
    if info is not None:
        info.append(dict(working=[hs, ws], replaced=bool(flag)))
    return out


def run_program(images, opcode, iarg, farg, table, seed, backend="numpy", info=None):
    """uint8 [B,H,W,C] + a program -> (uint8 [B,H,W,C], excusable bool [B,H,W,C]) as make_spx_connect_golden.run_program, with
    ``iarg[6]`` of SUPERPIXELS slots honoured; ``info`` (a list) receives a dict per scaled slot"""
    out = np.empty_like(images)
    exc = np.zeros(images.shape, dtype=bool)
    h, w = images.shape[1:3]
    for i in range(images.shape[0]):
        cur, e = images[i], np.zeros(images.shape[1:], dtype=bool)
        for s in range(opcode.shape[1]):
            op, ia = int(opcode[i, s]), iarg[i, s]
            if op == SUPERPIXELS and is_scaled(h, w, int(ia[6])):
                d = []
                cur = scaled_slot(cur, ia, threshold(farg[i, s, 0]), int(seed[i, s]), backend, d)
                if info is not None:
                    info.append(dict(d[0], sample=i, slot=s))
                e = np.full_like(e, bool(e.any()))      # (every pixel depends on every pixel)
            else:
                one = tuple(np.ascontiguousarray(a[i:i + 1, s:s + 1]) for a in (opcode, iarg, farg, table, seed))
                o, ee = F9B.run_program(cur[None], *one, backend=backend)
                radius, mixes = {HUE_SATURATION: (0, True), NOISE_ALPHA: (1, False)}.get(op, (0, False))
                e = (np.full_like(e, bool(e.any())) if op == SUPERPIXELS else dilate(e, radius, mixes)) | ee[0]
                cur = o[0]
        out[i], exc[i] = cur, e
    return out, exc


# ------------------------------------------------------------------------------------------------ cases
P_BETWEEN = 0.55
SMALL = (      # name, (h, w, c), max_size, kind, (gy, gx), connected samples
    ("non_integer", (40, 56, 3), 16, "smooth", (3, 4), "half"),
    ("tall_c1", (56, 40, 1), 16, "smooth", (4, 3), "half"),
    ("odd_c4_connected", (33, 47, 4), 20, "smooth", (4, 5), "all"),
    ("exact_2x", (64, 64, 3), 32, "smooth", (5, 5), "half"),
)
EDGES = (("production_n20", 20), ("production_n200", 200))


def small_cases():
    """one image per case, six samples: p_replace in {0, between, 1} x min_size in {0, superpixel_min_size} (``half``) or
    min_size in {superpixel_min_size, 1} (``all``), both measured on the working size"""
    cs = []
    rng = np.random.default_rng(20280)
    for n, (name, (h, w, c), m, kind, (gy, gx), conn) in enumerate(SMALL):
        hs, ws = working_size(h, w, m)
        sizes = (0, F9B.superpixel_min_size(gy, gx, hs, ws)) if conn == "half" else (F9B.superpixel_min_size(gy, gx, hs, ws), 1)
        prog = Prog(6, 1)
        for i in range(6):
            prog.put(i, 0, SUPERPIXELS, gy=gy, gx=gx, iters=5, compactness=10, p=(0.0, P_BETWEEN, 1.0)[i % 3],
                     seed=int(rng.integers(0, 2 ** 63)))
            prog.iarg[i, 0, 5], prog.iarg[i, 0, 6] = sizes[i // 3], m
        cs.append(dict(name="%s_%dx%dx%d_m%d" % (name, h, w, c, m), b=6, h=h, w=w, c=c, seed=900 + n, kind=kind, prog=prog))
    return cs


def edge_cases():
    """the workload's shape: 256 x 256 x 3, B = 2 (a smooth image with noise, uniform noise), max_size 128, n_segments 20 and
    200 through the package's grid rule restated here on the working size, 5 updates, connected"""
    cs = []
    rng = np.random.default_rng(20281)
    for n, (name, segments) in enumerate(EDGES):
        h = w = 256
        hs, ws = working_size(h, w, 128)
        gy = min(hs, max(1, int(np.floor(np.sqrt(segments * hs / ws) + 0.5))))
        gx = min(ws, max(1, int(np.floor(segments / gy + 0.5))))
        prog = Prog(2, 1)
        for i in range(2):
            prog.put(i, 0, SUPERPIXELS, gy=gy, gx=gx, iters=5, p=(1.0, P_BETWEEN)[i], seed=int(rng.integers(0, 2 ** 63)))
            prog.iarg[i, 0, 5], prog.iarg[i, 0, 6] = F9B.superpixel_min_size(gy, gx, hs, ws), 128
        cs.append(dict(name=name, b=2, h=h, w=w, c=3, seed=950 + n, kind="mixed", prog=prog))
    return cs


case_inputs = F9B.case_inputs


def _arrays(case):
    p = case["prog"]
    return p.opcode, p.iarg, p.farg, p.table, p.seed


def expected(case, backend="numpy", info=None):
    out, exc = run_program(case_inputs(case), *_arrays(case), backend=backend, info=info)
    assert not exc.any()
    return out


def check_restatement(case_list):
    """the sequential restatement against the vectorised one, bit for bit -> values compared"""
    tot = 0
    for case in case_list:
        a, n = expected(case, "independent"), expected(case, "numpy")
        assert np.array_equal(a, n), (case["name"], int((a != n).sum()))
        tot += a.size
    return tot


def build():
    g = {}
    for n, case in enumerate(small_cases()):
        info = []
        out = expected(case, "numpy", info=info)
        x = case_inputs(case)
        assert len(info) == 6 and all(d["working"] == info[0]["working"] for d in info)
        assert not info[0]["replaced"] and not info[3]["replaced"] and info[2]["replaced"] and info[5]["replaced"]
        assert np.array_equal(out[0], x[0]) and np.array_equal(out[3], x[3]), "p_replace = 0 returns the input"
        assert not np.array_equal(out[2], x[2]) and not np.array_equal(out[5], x[5])
        k = "c%02d_" % n
        g[k + "name"] = np.array(case["name"])
        g[k + "kind"] = np.array(case["kind"])
        g[k + "dims"] = np.array([case[s] for s in ("b", "h", "w", "c", "seed")], dtype=np.int64)
        g[k + "working"] = np.array(info[0]["working"], dtype=np.int64)
        g[k + "replaced"] = np.array([d["replaced"] for d in info])
        g[k + "opcode"], g[k + "iarg"], g[k + "farg"], g[k + "table"], g[k + "seed"] = _arrays(case)
        g[k + "u8"] = planar(out)
    return g


def build_edges():
    d = {}
    for case in edge_cases():
        info = []
        out = expected(case, "numpy", info=info)
        d[case["name"]] = dict(sha256=hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest(),
                               dims=[int(case[s]) for s in ("b", "h", "w", "c", "seed")],
                               grid=[int(v) for v in case["prog"].iarg[0, 0, :2]], min_size=int(case["prog"].iarg[0, 0, 5]),
                               max_size=int(case["prog"].iarg[0, 0, 6]), working=info[0]["working"],
                               replaced=[q["replaced"] for q in info])
    return d


def load_cases(g):
    """the cases of a loaded fixture: dicts with the program arrays and the expected images ([B,H,W,C] again)"""
    out = []
    for k in sorted(f[:-4] for f in g.files if f.endswith("_name")):
        b, h, w, c, seed = (int(v) for v in g[k + "dims"])
        out.append(dict(name=str(g[k + "name"]), kind=str(g[k + "kind"]), b=b, h=h, w=w, c=c, seed=seed, opcode=g[k + "opcode"],
                        iarg=g[k + "iarg"], farg=g[k + "farg"], table=g[k + "table"], seed_arr=g[k + "seed"],
                        working=[int(v) for v in g[k + "working"]], replaced=g[k + "replaced"],
                        u8=np.ascontiguousarray(np.moveaxis(g[k + "u8"], 1, -1))))
    return out


if __name__ == "__main__":
    check_resize_anchors()
    print("float64 restatement of the resize differs on %d of %d values" % float_mismatches())
    print("restatements agree on %d values" % check_restatement(small_cases() + edge_cases()))
    g, d = build(), build_edges()
    np.savez_compressed(OUT, **g)
    with open(OUT_EDGES, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays;", OUT_EDGES)
