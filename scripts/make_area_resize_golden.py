"""Writes tests/golden/area_resize.npz and tests/golden/area_resize_edges.json: the fixtures of the native-size evaluation of
MS-CMRSeg (csrc/area_resize.hip, ``kernels.area_resize`` / ``kernels.reconstruct_resize_argmax``).

The reference resizes every class plane with ``cv2.resize(.., INTER_AREA)``.  OpenCV is not at hand, so the rule below is this
build's own convention, written after OpenCV's ``resize.cpp``; its parity with OpenCV is NOT pinned.  What pins the rule: the two
restatements in this file (``resize_vec``: vectorised numpy over per-axis tables; ``resize_loops``: Python loops over Python
floats and ``numpy.float32`` scalars, per output pixel), which must agree bit for bit before anything is written, the files they
write, and three anchors that hold for OpenCV by its documentation: equal sizes return the input, an integer enlargement
replicates pixels, an integer shrink averages blocks.

The rule, per axis with source size S and destination size D, ``scale = S / D`` and ``inv = D / S`` in float64:
  * both axes shrink or stay (S >= D on both): the area table.  ``f1 = d * scale``, ``f2 = f1 + scale``, ``cell = min(scale,
    S - f1)``, ``s1 = ceil(f1)``, ``s2 = min(floor(f2), S - 1)``, ``s1 = min(s1, s2)``; tap ``s1 - 1`` with ``(s1 - f1) / cell``
    if ``s1 - f1 > 1e-3``, taps ``s1 .. s2 - 1`` with ``1 / cell``, tap ``s2`` with ``min(min(f2 - s2, 1), cell) / cell`` if
    ``f2 - s2 > 1e-3``; the weights rounded to float32
  * otherwise two taps on both axes: ``sx = floor(d * scale)``, ``fx = (d + 1) - (sx + 1) * inv``, ``fx = 0`` if ``fx <= 0`` else
    ``fx - floor(fx)``; ``sx >= S - 1``: ``sx = S - 1``, ``fx = 0``; taps ``sx`` with ``float32(1 - fx)`` and ``sx + 1`` with
    ``float32(fx)``, the tap ``sx`` alone (weight 1) when ``fx == 0``
  * the output, in float32 with every operation rounded on its own: for each source row of the vertical taps in order, the row
    is reduced over the horizontal taps in order (``h = w0 * v0``, then ``h = h + w * v``), then ``out = wy0 * h0``, then ``out =
    out + wy * h``.  The first term of each sum is assigned, so a single tap of weight 1 returns the value's bits

    python scripts/make_area_resize_golden.py            # writes both files
    python scripts/make_area_resize_golden.py --check    # regenerates and compares with the files"""
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "area_resize.npz")
EDGES = os.path.join(ROOT, "tests", "golden", "area_resize_edges.json")

SRC_W, SRC_H = 24, 20
# (w, h) as cv2's dsize: fractional enlargement, x 2, equal, / 2, fractional shrink, mixed (the two-tap rule on both axes)
SIZES = ((45, 37), (48, 40), (24, 20), (12, 10), (17, 13), (45, 13))
# a shrinking axis under the two-tap rule whose source patch is too large to stage: [600, 16] -> [5, 32]
TALL = (16, 600, 32, 5)
FUSED_SMALL = dict(n=2, c=4, crop=6, origin=16, sizes=((29, 23), (32, 32), (11, 13), (16, 16)))
FUSED_LARGE = dict(n=2, c=4, crop=112, origin=256, sizes=((480, 480), (511, 257)))


# ---------------------------------------------------------------------------------------------- the tables, vectorised
def is_area(sh, sw, dh, dw):
    return sw >= dw and sh >= dh


def table_vec(S, D, area):
    """-> (idx int64 [D, T], w float32 [D, T], n int64 [D]): the taps of every output index of the axis, in order"""
    d = np.arange(D, dtype=np.float64)
    scale = np.float64(S) / np.float64(D)
    if area:
        f1 = d * scale
        f2 = f1 + scale
        cell = np.minimum(scale, np.float64(S) - f1)
        s1 = np.ceil(f1).astype(np.int64)
        s2 = np.minimum(np.floor(f2).astype(np.int64), S - 1)
        s1 = np.minimum(s1, s2)
        lead = (s1 - f1) > 1e-3
        trail = (f2 - s2) > 1e-3
        n = lead.astype(np.int64) + (s2 - s1) + trail.astype(np.int64)
        start = s1 - lead.astype(np.int64)
        t = np.arange(int(n.max()), dtype=np.int64)
        idx = start[:, None] + t[None, :]
        w = np.repeat((1.0 / cell).astype(np.float32)[:, None], len(t), axis=1)
        w[lead, 0] = ((s1 - f1) / cell).astype(np.float32)[lead]
        wt = (np.minimum(np.minimum(f2 - s2, 1.0), cell) / cell).astype(np.float32)
        w[np.nonzero(trail)[0], (n - 1)[trail]] = wt[trail]
        return idx, w, n
    inv = np.float64(D) / np.float64(S)
    sx = np.floor(d * scale).astype(np.int64)
    fx = (d + 1.0) - (sx + 1).astype(np.float64) * inv
    fx = np.where(fx <= 0, 0.0, fx - np.floor(fx))
    last = sx >= S - 1
    sx = np.where(last, S - 1, sx)
    fx = np.where(last, 0.0, fx)
    n = np.where(fx == 0, 1, 2).astype(np.int64)
    idx = np.stack([sx, sx + 1], axis=1)
    w = np.stack([(1.0 - fx).astype(np.float32), fx.astype(np.float32)], axis=1)
    return idx, w, n


def _reduce(a, tab, dtype):
    """a [R, S] -> [R, D]: the taps of ``tab`` along the last axis, in order, the first term assigned"""
    idx, w, n = tab
    a = a.astype(dtype, copy=False)
    w = w.astype(dtype)
    safe = np.clip(idx, 0, a.shape[1] - 1)
    with np.errstate(all="ignore"):
        acc = w[None, :, 0] * a[:, safe[:, 0]]
        for t in range(1, idx.shape[1]):
            acc = np.where((t < n)[None, :], acc + w[None, :, t] * a[:, safe[:, t]], acc)
    return acc


def resize_vec(src, dh, dw, dtype=np.float32):
    """one plane [sh, sw] float32 -> [dh, dw]; ``dtype=np.float64``: the same tables (float32 weights) evaluated in float64"""
    sh, sw = src.shape
    area = is_area(sh, sw, dh, dw)
    h = _reduce(src, table_vec(sw, dw, area), dtype)                      # [sh, dw]: every source row reduced horizontally
    return np.ascontiguousarray(_reduce(h.T, table_vec(sh, dh, area), dtype).T)


def max_taps(sh, sw, dh, dw):
    """the largest number of horizontal taps plus the largest number of vertical taps of the resize"""
    area = is_area(sh, sw, dh, dw)
    return int(table_vec(sw, dw, area)[2].max() + table_vec(sh, dh, area)[2].max())


# ---------------------------------------------------------------------------------------------- the same, in plain Python
def taps_loops(d, S, D, area):
    """-> [(source index, numpy.float32 weight), ..] of output index d, with Python floats (float64)"""
    scale = float(S) / float(D)
    if area:
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, S - f1)
        s1 = int(math.ceil(f1))
        s2 = min(int(math.floor(f2)), S - 1)
        s1 = min(s1, s2)
        out = []
        if s1 - f1 > 1e-3:
            out.append((s1 - 1, np.float32((s1 - f1) / cell)))
        for s in range(s1, s2):
            out.append((s, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            out.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
        return out
    inv = float(D) / float(S)
    sx = int(math.floor(d * scale))
    fx = (d + 1) - (sx + 1) * inv
    fx = 0.0 if fx <= 0 else fx - math.floor(fx)
    if sx >= S - 1:
        sx, fx = S - 1, 0.0
    if fx == 0:
        return [(sx, np.float32(1.0))]
    return [(sx, np.float32(1.0 - fx)), (sx + 1, np.float32(fx))]


def resize_loops(src, dh, dw):
    sh, sw = src.shape
    area = is_area(sh, sw, dh, dw)
    out = np.empty((dh, dw), np.float32)
    xt = [taps_loops(d, sw, dw, area) for d in range(dw)]
    with np.errstate(all="ignore"):
        for dy in range(dh):
            yt = taps_loops(dy, sh, dh, area)
            for dx in range(dw):
                acc = None
                for sy, wy in yt:
                    h = None
                    for sx, wx in xt[dx]:
                        t = wx * src[sy, sx]
                        h = t if h is None else h + t
                    q = wy * h
                    acc = q if acc is None else acc + q
                assert type(acc) is np.float32
                out[dy, dx] = acc
    return out


# ---------------------------------------------------------------------------------------------- reconstruct, argmax
def reconstruct(logits, crop, origin):
    """``reconstuct_volume`` on channels-first logits [N, C, 2 crop, 2 crop] -> [N, C, origin, origin]"""
    n, c = logits.shape[:2]
    out = np.zeros((n, c, origin, origin), np.float32)
    o = int(origin / 2)
    out[:, :, o - crop:o + crop, o - crop:o + crop] = logits
    return out


def argmax_rule(planes):
    """[N, C, H, W] -> uint8 [N, H, W]: the first class holding the maximum, 0 where any class is NaN (``M.argmax_labels``)"""
    lab = np.argmax(planes, axis=1)
    lab[np.isnan(planes).any(axis=1)] = 0
    return lab.astype(np.uint8)


def resized_planes(canvas, dh, dw, fn=resize_vec):
    return np.stack([np.stack([fn(p, dh, dw) for p in img]) for img in canvas])


# ---------------------------------------------------------------------------------------------- inputs (seeded)
def source_planes(seed=0, n=2, h=SRC_H, w=SRC_W):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w)) * 3.0).astype(np.float32)
    x[0, :4, :4] = rng.integers(-8, 9, (4, 4)).astype(np.float32)           # small integers
    x[0, 5, 5], x[0, 5, 6], x[1, 0, 0] = -0.0, 0.0, -0.0                    # signed zeros: equal sizes must keep the bits
    x[1, -1, -1], x[1, 7, 3] = np.float32(1e-40), np.float32(3e38)          # a subnormal, a value near the largest
    return x


def logits_case(n, c, size, seed):
    """logits [n, c, size, size]: mostly negative at the rim of the window (the zero canvas wins at the border), class 0
    dominant nowhere, exact ties between classes planted in a block"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, c, size, size)) * 2.0 - 0.5).astype(np.float32)
    x[:, :, :2, :] -= 4.0
    x[:, :, :, -2:] -= 4.0
    q = size // 4
    if c > 1:
        x[:, 1, q:2 * q, q:2 * q] = x[:, 0, q:2 * q, q:2 * q]               # ties of classes 0 and 1
        x[:, c - 1, 2 * q:3 * q, q:2 * q] = np.maximum(x[:, c - 1, 2 * q:3 * q, q:2 * q], 3.0)
    x[:, 0, -q:, :q] = 0.0                                                  # ties with the canvas' zero
    return x


def digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(("%s %r " % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- the files
def build():
    """the arrays of area_resize.npz; raises SystemExit unless the two restatements agree bit for bit on every one"""
    data = {"numpy_version": np.array(np.__version__)}
    src = source_planes()
    data["src"] = src

    def both(planes, dh, dw, tag):
        a = np.stack([resize_vec(p, dh, dw) for p in planes])
        b = np.stack([resize_loops(p, dh, dw) for p in planes])
        if a.dtype != np.float32 or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            raise SystemExit("the two restatements differ on %s" % tag)
        return a

    for w, h in SIZES:
        data["out_%dx%d" % (w, h)] = both(src, h, w, "%dx%d" % (w, h))
    sw, sh, dw, dh = TALL
    tall = (np.random.default_rng(3).standard_normal((1, sh, sw)) * 2.0).astype(np.float32)
    data["tall_src"], data["tall_out"] = tall, both(tall, dh, dw, "tall")
    f = FUSED_SMALL
    logits = logits_case(f["n"], f["c"], 2 * f["crop"], seed=5)
    data["fused_logits"] = logits
    canvas = reconstruct(logits, f["crop"], f["origin"])
    for w, h in f["sizes"]:
        planes = np.stack([both(img, h, w, "fused %dx%d" % (w, h)) for img in canvas])
        data["fused_labels_%dx%d" % (w, h)] = argmax_rule(planes)
    return data


def edges():
    """the cases above one tile, as digests: N = 2, C = 4, 224 x 224 logits in a 256 canvas to 480 x 480 and to 511 x 257 (w x h).
    Vectorised restatement; its agreement with the loops is checked on the top-left 40 x 40 outputs' worth of one plane"""
    f = FUSED_LARGE
    logits = logits_case(f["n"], f["c"], 2 * f["crop"], seed=11)
    canvas = reconstruct(logits, f["crop"], f["origin"])
    cases = {}
    for w, h in f["sizes"]:
        planes = resized_planes(canvas, h, w)
        # a resize of a sub-image is no sub-image of the resize in general: compare on a whole small problem of the same ratio class
        sub = canvas[0, 1, 100:140, 100:140]
        sw_, sh_ = max(1, round(40 * w / f["origin"])), max(1, round(40 * h / f["origin"]))
        if not np.array_equal(resize_vec(sub, sh_, sw_).view(np.uint32), resize_loops(sub, sh_, sw_).view(np.uint32)):
            raise SystemExit("the two restatements differ at the ratio of %dx%d" % (w, h))
        cases["canvas_%dx%d" % (w, h)] = {"shape": [f["n"], f["c"], h, w], "planes": digest(planes), "labels": digest(argmax_rule(planes))}
    return {"numpy_version": np.__version__, "cases": cases}


def main():
    data, edge = build(), edges()
    if "--check" in sys.argv:
        old = np.load(PATH)
        assert sorted(old.files) == sorted(data), "the file holds other arrays"
        for k in data:
            if k != "numpy_version":
                assert old[k].dtype == data[k].dtype and np.array_equal(old[k].view(np.uint8), data[k].view(np.uint8)), k
        assert json.load(open(EDGES))["cases"] == edge["cases"], "the digests differ"
        print("ok: %d arrays equal %s, %d digests equal %s" % (len(data), PATH, len(edge["cases"]), EDGES))
        return
    np.savez_compressed(PATH, **data)
    with open(EDGES, "w") as fh:
        json.dump(edge, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d arrays, %d bytes; %s: %d cases" % (PATH, len(data), os.path.getsize(PATH), EDGES, len(edge["cases"])))


if __name__ == "__main__":
    main()
