"""Writes tests/golden/croppad.npz: the fixture of the device-side CropAndPad with numpy's pad modes
(pointcloududa_amd/utils/croppad.py, csrc/croppad.hip).

The expected intermediates (``pad_*``) are the outputs of ``numpy.pad`` ITSELF, called as imgaug calls it: ``constant_values =
cval`` for ``constant``, ``end_values = cval`` for ``linear_ramp``, the statistical modes over the whole axis.  Next to it stands
a plain restatement of what the kernels compute (no ``numpy.pad``, no ``linspace``): index folding, the statistics with their
rounding, the two forms of the ramp.  The file is written only if the restatement equals ``numpy.pad`` bit for bit on every case,
and if a second, independent restatement of the resize (Python loops over Python floats) equals the vectorised one.  Inputs are
synthetic (seeded).  The numpy version is recorded in the file; the GPU tests read the file alone.

What numpy.pad does (checked against numpy 2.2.6), and the restatement follows:
  * axis 0 is padded first, axis 1 on the padded array: a left / right pad value of row y (a pad row included) comes from that
    row of the axis-0-padded array, a corner is a statistic of statistics or a ramp of a ramp
  * mean and median are numpy.round (half to even) of the float64 statistic; the median of an even count is the mean of the
    two middle values
  * linear_ramp, per side: floor(end + k step), k = 0 outermost, step = (edge - end) / width -- unless ANY edge value of that
    side's linspace call (all columns and channels of the side) equals end: then the whole call is floor(end + (k / width) delta)
    (linspace's any_step_zero branch).  The two differ, e.g. width 10, end 0, edge 90, k = 7: 63 against 62

    python scripts/make_croppad_golden.py            # writes the file
    python scripts/make_croppad_golden.py --check    # regenerates and compares the array contents with the file
    python scripts/make_croppad_golden.py --digests  # writes tests/golden/heavy_plan_digests.json (see plan_digest)
    python scripts/make_croppad_golden.py --edges    # writes tests/golden/croppad_edges.json (see edges)"""
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "croppad.npz")
DIGESTS = os.path.join(ROOT, "tests", "golden", "heavy_plan_digests.json")
MODES = ("constant", "edge", "linear_ramp", "maximum", "mean", "median", "minimum", "reflect", "symmetric", "wrap")
SHAPES = ((9, 7), (12, 10), (33, 18), (64, 48))
MAX_PAD = 64


# ---------------------------------------------------------------------------------------------- geometry
def split_sides(h, w, top, right, bottom, left):
    """-> (ct, cb, cl, cr, pt, pb, pl, pr): the cropped and the padded pixels of the four sides"""
    crops = tuple(max(-int(v), 0) for v in (top, bottom, left, right))
    pads = tuple(max(int(v), 0) for v in (top, bottom, left, right))
    return crops + pads


def crop(x, top, right, bottom, left):
    h, w = x.shape[:2]
    ct, cb, cl, cr = split_sides(h, w, top, right, bottom, left)[:4]
    return x[ct:h - cb, cl:w - cr]


# ---------------------------------------------------------------------------------------------- numpy itself
def numpy_pad(xc, pt, pb, pl, pr, mode, cval):
    """numpy.pad as imgaug calls it: the reference"""
    name = MODES[mode]
    kw = {}
    if name == "constant":
        kw["constant_values"] = cval
    elif name == "linear_ramp":
        kw["end_values"] = cval
    return np.pad(xc, ((pt, pb), (pl, pr), (0, 0)), mode=name, **kw)


# ---------------------------------------------------------------------------------------------- the plain restatement
def _fold(i, n, name):
    """the index inside [0, n) that index i of the padded axis reads"""
    if name == "reflect":
        p = 2 * (n - 1)
        i = i % p
        return np.where(i < n, i, p - i)
    if name == "symmetric":
        p = 2 * n
        i = i % p
        return np.where(i < n, i, p - 1 - i)
    if name == "wrap":
        return i % n
    return np.clip(i, 0, n - 1)      # edge


def _round_half_even_halves(twice):
    """round(twice / 2) half to even, in integers"""
    r = twice >> 1
    return r + np.where(twice & 1, r & 1, 0)


def _stat(a, axis, name):
    """numpy.pad's statistic of a uint8 array along an axis, as int64"""
    a = a.astype(np.int64)
    n = a.shape[axis]
    if name == "maximum":
        return a.max(axis)
    if name == "minimum":
        return a.min(axis)
    if name == "mean":
        return np.rint(a.sum(axis) / float(n)).astype(np.int64)      # (an exact integer sum, one division, half to even)
    s = np.sort(a, axis=axis)
    return _round_half_even_halves(np.take(s, (n - 1) // 2, axis) + np.take(s, n // 2, axis))


def _ramp(edge, width, end, outer_first):
    """one side: [width, ...] values from `end` (k = 0, outermost) towards the edge values `edge`"""
    e = edge.astype(np.float64)
    k = np.arange(width, dtype=np.float64).reshape((width,) + (1,) * e.ndim)
    delta = e - float(end)
    if np.any(edge == end):
        v = np.floor(float(end) + (k / float(width)) * delta[None])
    else:
        v = np.floor(float(end) + k * (delta / float(width))[None])
    v = v.astype(np.uint8)
    return v if outer_first else v[::-1]


def pad_restated(xc, pt, pb, pl, pr, mode, cval):
    """I of section 1 of the issue, without numpy.pad: uint8 [Hc + pt + pb, Wc + pl + pr, C]"""
    name = MODES[mode]
    hc, wc, c = xc.shape
    if name in ("edge", "reflect", "symmetric", "wrap"):
        iy = _fold(np.arange(-pt, hc + pb), hc, name)
        ix = _fold(np.arange(-pl, wc + pr), wc, name)
        return xc[iy][:, ix]
    if name == "constant":
        out = np.full((hc + pt + pb, wc + pl + pr, c), cval, dtype=np.uint8)
        out[pt:pt + hc, pl:pl + wc] = xc
        return out
    if name == "linear_ramp":
        rows = [xc]
        if pt:
            rows.insert(0, _ramp(xc[0], pt, cval, True))
        if pb:
            rows.append(_ramp(xc[-1], pb, cval, False))
        a0 = np.concatenate(rows, axis=0)
        cols = [a0]
        if pl:
            cols.insert(0, np.moveaxis(_ramp(a0[:, 0], pl, cval, True), 0, 1))
        if pr:
            cols.append(np.moveaxis(_ramp(a0[:, -1], pr, cval, False), 0, 1))
        return np.concatenate(cols, axis=1)
    col = _stat(xc, 0, name).astype(np.uint8)                       # [Wc, C]
    a0 = np.concatenate([np.broadcast_to(col, (pt, wc, c)), xc, np.broadcast_to(col, (pb, wc, c))], axis=0)
    row = _stat(a0, 1, name).astype(np.uint8)[:, None, :]           # [Hi, 1, C]
    return np.concatenate([np.broadcast_to(row, (a0.shape[0], pl, c)), a0, np.broadcast_to(row, (a0.shape[0], pr, c))], axis=1)


def _axis_terms(n_i, n_out):
    """(i0, i1, w1) of every output index: s = (k + 0.5) (n_i / n_out) - 0.5, the neighbours clamped into [0, n_i)"""
    a = float(n_i) / float(n_out)
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * a - 0.5
    f = np.floor(s)
    i0 = f.astype(np.int64)
    return np.clip(i0, 0, n_i - 1), np.clip(i0 + 1, 0, n_i - 1), s - f, np.floor(s + 0.5).astype(np.int64)


def resize_restated(img, h, w):
    """I (uint8 [Hi, Wi, C]) -> uint8 [h, w, C] by the order-1 rule, float64, every operation rounded on its own"""
    y0, y1, wy1, _ = _axis_terms(img.shape[0], h)
    x0, x1, wx1, _ = _axis_terms(img.shape[1], w)
    f = img.astype(np.float64)
    wy1, wx1 = wy1[:, None, None], wx1[None, :, None]
    wy0, wx0 = 1.0 - wy1, 1.0 - wx1
    v = np.zeros((h, w, img.shape[2]), dtype=np.float64)
    v = v + f[y0][:, x0] * wy0 * wx0
    v = v + f[y0][:, x1] * wy0 * wx1
    v = v + f[y1][:, x0] * wy1 * wx0
    v = v + f[y1][:, x1] * wy1 * wx1
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def resize_loops(img, h, w):
    """the same rule once more, independently: Python loops over Python floats"""
    hi, wi, c = img.shape
    out = np.zeros((h, w, c), dtype=np.uint8)
    ay, ax = hi / h, wi / w
    for y in range(h):
        sy = (y + 0.5) * ay - 0.5
        fy = math.floor(sy)
        ty = sy - fy
        ya, yb = min(max(fy, 0), hi - 1), min(max(fy + 1, 0), hi - 1)
        for x in range(w):
            sx = (x + 0.5) * ax - 0.5
            fx = math.floor(sx)
            tx = sx - fx
            xa, xb = min(max(fx, 0), wi - 1), min(max(fx + 1, 0), wi - 1)
            for k in range(c):
                v = 0.0
                v += float(img[ya, xa, k]) * (1.0 - ty) * (1.0 - tx)
                v += float(img[ya, xb, k]) * (1.0 - ty) * tx
                v += float(img[yb, xa, k]) * ty * (1.0 - tx)
                v += float(img[yb, xb, k]) * ty * tx
                out[y, x, k] = min(max(math.floor(v + 0.5), 0), 255)
    return out


def labels_restated(lab, top, right, bottom, left):
    """integer [H, W] -> the same crop, constant 0 around it, the texel at floor(s + 0.5)"""
    h, w = lab.shape
    ct, cb, cl, cr, pt, pb, pl, pr = split_sides(h, w, top, right, bottom, left)
    lc = lab[ct:h - cb, cl:w - cr]
    big = np.zeros((lc.shape[0] + pt + pb, lc.shape[1] + pl + pr), dtype=lab.dtype)
    big[pt:pt + lc.shape[0], pl:pl + lc.shape[1]] = lc
    yn, xn = _axis_terms(big.shape[0], h)[3], _axis_terms(big.shape[1], w)[3]
    return big[np.clip(yn, 0, big.shape[0] - 1)][:, np.clip(xn, 0, big.shape[1] - 1)]


def crop_pad_restated(x, top, right, bottom, left, mode, cval, pad_fn=pad_restated):
    """-> (I, the output): one live sample of section 1"""
    h, w = x.shape[:2]
    pt, pb, pl, pr = split_sides(h, w, top, right, bottom, left)[4:]
    big = pad_fn(crop(x, top, right, bottom, left), pt, pb, pl, pr, mode, cval)
    return big, resize_restated(big, h, w)


def sides_valid(h, w, top, right, bottom, left):
    ct, cb, cl, cr, pt, pb, pl, pr = split_sides(h, w, top, right, bottom, left)
    hc, wc = h - ct - cb, w - cl - cr
    return hc >= 2 and wc >= 2 and max(pt, pb) <= min(MAX_PAD, hc - 1) and max(pl, pr) <= min(MAX_PAD, wc - 1)


# ---------------------------------------------------------------------------------------------- the cases
def side_sets(h, w):
    """the side sets of the GPU tests that an h x w image admits, (top, right, bottom, left)"""
    sets = [(3, 2, 0, 4), (0, 0, 0, 0), (-2, -1, -3, -2), (5, -2, -1, 6), (min(MAX_PAD, h - 1), 0, 0, min(MAX_PAD, w - 1))]
    return [s for s in sets if sides_valid(h, w, *s)]


def test_image(h, w, c, seed):
    """smooth gradients plus noise, with 0 and 255 present: statistics and ramps get distinct columns"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (yy[..., None] * 5 + xx[..., None] * 3 + np.arange(c) * 40) % 200
    img = np.clip(base + rng.integers(0, 56, (h, w, c)), 0, 255).astype(np.uint8)
    img[rng.integers(0, h), rng.integers(0, w)] = 0
    img[rng.integers(0, h), rng.integers(0, w)] = 255
    return img


def half_image():
    """6 x 8 x 1: column x holds x three times and x + 1 three times (shuffled): mean and median are x + 0.5, x even and odd"""
    img = np.zeros((6, 8, 1), dtype=np.uint8)
    order = np.array([1, 0, 0, 1, 1, 0])
    for x in range(8):
        img[:, x, 0] = x + np.roll(order, x)
    return img


def ramp_pair():
    """22 x 22 x 1, no value 0; left column 90.  The second image has one more left-edge value equal to the end value 0"""
    rng = np.random.default_rng(7)
    a = rng.integers(1, 256, (22, 22, 1)).astype(np.uint8)
    a[:, 0] = 90
    b = a.copy()
    b[13, 0] = 0
    return a, b


def build():
    out = {"numpy_version": np.array(np.__version__), "mode_names": np.array(MODES)}
    checked = []

    def add(key, x, sides, mode, cval):
        h, w = x.shape[:2]
        assert sides_valid(h, w, *sides), (key, sides)
        pt, pb, pl, pr = split_sides(h, w, *sides)[4:]
        ref = numpy_pad(crop(x, *sides), pt, pb, pl, pr, mode, cval)
        big, res = crop_pad_restated(x, *sides, mode, cval)
        if big.dtype != ref.dtype or big.shape != ref.shape or not np.array_equal(big, ref):
            raise SystemExit("the restatement differs from numpy.pad on %s (mode %s, sides %r)" % (key, MODES[mode], sides))
        if not np.array_equal(res, resize_loops(ref, h, w)):
            raise SystemExit("the two restatements of the resize differ on %s" % key)
        out["pad_" + key], out["out_" + key] = ref, res
        out["arg_" + key] = np.array(list(sides) + [mode, cval], dtype=np.int32)
        checked.append(key)

    # every mode, C in {1, 3}, four shapes; the side sets rotate so that every mode meets every set
    for c in (1, 3):
        for si, (h, w) in enumerate(SHAPES):
            out["img_%dx%dx%d" % (h, w, c)] = test_image(h, w, c, 100 * c + si)
    combo = 0
    turn = {}                                        # per number of admitted sets: how often such a shape came by
    names = []
    for c in (1, 3):
        for si, (h, w) in enumerate(SHAPES):
            sets = side_sets(h, w)
            k = turn.get(len(sets), 0)
            turn[len(sets)] = k + 1
            for mode in range(10):
                key = "%dx%dx%d_m%d" % (h, w, c, mode)
                add(key, out["img_%dx%dx%d" % (h, w, c)], sets[(k + mode) % len(sets)], mode, (37 * mode + 11 * combo) % 256)
                names.append(key)
            combo += 1
    out["case_names"] = np.array(names)
    # the net-zero geometries at 22 x 22: the output is numpy.pad's array itself
    out["img_22x22x3"] = test_image(22, 22, 3, 5)
    for mode in range(10):
        for tag, sides in (("a", (10, -10, -10, 10)), ("b", (-7, 10, 7, -10))):
            key = "zero%s_m%d" % (tag, mode)
            add(key, out["img_22x22x3"], sides, mode, 0 if mode == 2 else 200)
            assert np.array_equal(out["pad_" + key], out["out_" + key]), key
    # the pair that separates the two forms of the ramp
    ra, rb = ramp_pair()
    out["img_ramp_a"], out["img_ramp_b"] = ra, rb
    add("ramp_a", ra, (0, -10, 0, 10), 2, 0)
    add("ramp_b", rb, (0, -10, 0, 10), 2, 0)
    assert out["pad_ramp_a"][0, 7, 0] == 63 and out["pad_ramp_b"][0, 7, 0] == 62 and out["pad_ramp_b"][13, 7, 0] == 0
    # statistics that are k + 0.5 (even and odd k); a median over an even (6) and an odd (5) count
    out["img_half"] = half_image()
    for mode in (4, 5):
        add("half_even_m%d" % mode, out["img_half"], (2, 3, 1, 2), mode, 0)
        add("half_odd_m%d" % mode, out["img_half"], (2, 3, -1, 2), mode, 0)
    assert np.array_equal(out["pad_half_even_m4"][0, 2:10, 0], [0, 2, 2, 4, 4, 6, 6, 8])
    assert np.array_equal(out["pad_half_even_m5"][0, 2:10, 0], [0, 2, 2, 4, 4, 6, 6, 8])
    # masks: the same crop, constant 0, nearest -- whatever the image's mode is
    rng = np.random.default_rng(11)
    for (h, w) in ((12, 10), (33, 18)):
        lab = rng.integers(0, 5, (h, w)).astype(np.int32)
        out["lab_%dx%d" % (h, w)] = lab
        for k, sides in enumerate(side_sets(h, w)):
            out["labout_%dx%d_s%d" % (h, w, k)] = labels_restated(lab, *sides)
            out["labarg_%dx%d_s%d" % (h, w, k)] = np.array(sides, dtype=np.int32)
    out["checked"] = np.array(checked)
    return out


# ---------------------------------------------------------------------------------------------- the old presets' draws
DIGEST_PRESETS = ("heavy_device", "mscmrseg_aug2_device", "heavy_full_device", "mscmrseg_aug2_full_device")
DIGEST_BATCH, DIGEST_H, DIGEST_W, DIGEST_SEEDS = 16, 64, 48, 20


def plan_digest(plan):
    """sha256 over the stages of a HeavyPlan: each stage's type name and every array field (name, dtype, shape, bytes)"""
    h = hashlib.sha256()
    for st in plan.stages:
        h.update(type(st).__name__.encode())
        for name in sorted(vars(st)):
            a = np.ascontiguousarray(getattr(st, name))
            h.update(("%s|%s|%r|" % (name, a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
    return h.hexdigest()


def digests():
    """the four presets that existed before f14, seeds 0..19: to be recorded on a commit whose draws are to be pinned"""
    sys.path.insert(0, ROOT)
    from pointcloududa_amd.utils.heavy import sample_heavy_plan
    return {p: [plan_digest(sample_heavy_plan(DIGEST_BATCH, p, np.random.default_rng(s), DIGEST_H, DIGEST_W))
                for s in range(DIGEST_SEEDS)] for p in DIGEST_PRESETS}


# ---------------------------------------------------------------------------------------------- the edge shapes
EDGES = os.path.join(ROOT, "tests", "golden", "croppad_edges.json")


def edges():
    """tests/croppad_edge_cases.py's table (shapes above one tile, C = 2 and 4, lines above 64, pads of 64, 256 x 256): per
    row the sha256 of the restated output, per side set that of the restated labels.  Nothing is recorded unless I equals
    numpy.pad bit for bit and, below 100 x 100, the two restatements of the resize agree"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("croppad_edge_cases", os.path.join(ROOT, "tests", "croppad_edge_cases.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    cases = {}
    for cs in t.CASES:
        x = t.image_of(cs)
        for row, (big, res) in zip(cs.rows, t.expected_rows(cs)):
            pt, pb, pl, pr = split_sides(cs.h, cs.w, *row[:4])[4:]
            ref = numpy_pad(crop(x, *row[:4]), pt, pb, pl, pr, row[4], row[5])
            if big.dtype != ref.dtype or big.shape != ref.shape or not np.array_equal(big, ref):
                raise SystemExit("the restatement differs from numpy.pad on %s, row %r" % (cs.name, row))
            if max(cs.h, cs.w) < t.LOOPS_BELOW and not np.array_equal(res, resize_loops(ref, cs.h, cs.w)):
                raise SystemExit("the two restatements of the resize differ on %s, row %r" % (cs.name, row))
        cases[cs.name] = t.digests_of(cs)
    return {"numpy_version": np.__version__, "cases": cases}


def main():
    if "--edges" in sys.argv:
        data = edges()
        with open(EDGES, "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote %s: %d bytes" % (EDGES, os.path.getsize(EDGES)))
        return
    if "--digests" in sys.argv:
        with open(DIGESTS, "w") as fh:
            json.dump(digests(), fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", DIGESTS)
        return
    data = build()
    if "--check" in sys.argv:
        old = np.load(PATH)
        assert sorted(old.files) == sorted(data), "the file holds other arrays"
        for k in data:
            if k != "numpy_version":
                assert old[k].dtype == data[k].dtype and np.array_equal(old[k], data[k]), k
        print("ok: %d arrays equal %s" % (len(data), PATH))
        return
    np.savez_compressed(PATH, **data)
    print("wrote %s: %d arrays, %d bytes, %d cases equal to numpy.pad %s" % (PATH, len(data), os.path.getsize(PATH),
                                                                             len(data["checked"]), np.__version__))


if __name__ == "__main__":
    main()
