"""Writes tests/golden/resample.npz: the fixture of the device-side spacing resample (pointcloududa_amd/utils/resample.py,
csrc/resample.hip) -- the .npy path of the reference's utils/read_nii_image.py.

The expected arrays are the outputs of scipy.ndimage.zoom / numpy THEMSELVES, by the reference's own call sequence:

  images  ndimage.zoom(vol, [1, fy, fx], order=1) -> crop_volume -> (image - image.mean()) / image.std()
  labels  chained np.where remap -> to_categorical -> ndimage.zoom(onehot, [1, 1, fy, fx], order=1) -> argmax(axis=1) -> crop_volume

Next to them stands an independent plain restatement (vectorised numpy / Python integers, no scipy) of what the kernels
compute: the four-tap float64 rule, the fused label rule without a one-hot tensor, the exact integer statistics.  The file
is written only if the restatement equals the scipy outputs bit for bit.  Inputs are synthetic (seeded random volumes,
analytic discs).  The scipy and numpy versions are recorded in the file; the GPU tests read the file alone.

The four-tap rule, per axis: z = (in - 1) / (out - 1) (1.0 when out == 1), cc = double(k) z, i0 = floor(cc), t = cc - i0,
w0 = 1 - t, w1 = t; per pixel acc = (c00 wy0) wx0, += (c01 wy0) wx1, += (c10 wy1) wx0, += (c11 wy1) wx1, every operation
rounded on its own; a tap whose index equals the input size is 0 (mode='constant', cval=0).  One more rule comes out of the
search for an overshooting pair below: where double(out - 1) z > in - 1 the LAST coordinate lies beyond the last sample, and
scipy does not interpolate beyond the edge under mode='constant': the whole pixel is cval = 0 (not the edge value times
1 - t).  Such pairs exist (12551 of them with both sizes in 2..512); the smallest is in the fixture on either axis.

A second file, tests/golden/resample_edges.npz, holds the dispatch edges of the kernels under the same discipline (the section
'the second file' below).

    python scripts/make_resample_golden.py            # writes both files (one whose arrays are unchanged is left as it is)
    python scripts/make_resample_golden.py --check    # regenerates and compares the array contents with both files"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "resample.npz")
DTYPES = (("f32", np.float32), ("i16", np.int16), ("u8", np.uint8))
REMAP = ((200, 1), (500, 2), (600, 3))


# ---------------------------------------------------------------------------------------------- the plain restatement
def axis_terms(n_in, n_out):
    """(i0, t, outside) of every output index: outside marks a coordinate beyond the last sample (the pixel is 0)"""
    z = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
    cc = np.arange(n_out, dtype=np.float64) * z
    i0 = np.floor(cc)
    return i0.astype(np.int64), cc - i0, cc > n_in - 1


def crop_window(zh, zw, crop):
    """rows / columns of the reference's crop_volume(vol, crop // 2) on a (zh, zw) slice -> (y0, x0, oh, ow); crop 0: none"""
    if not crop:
        return 0, 0, zh, zw
    half = crop // 2
    y0, x0 = zh // 2 - half, zw // 2 - half
    if half < 1 or y0 < 0 or x0 < 0 or y0 + 2 * half > zh or x0 + 2 * half > zw:
        raise ValueError("the crop window of %d leaves the %dx%d slice" % (crop, zh, zw))
    return y0, x0, 2 * half, 2 * half


def _taps(vol, zh, zw, crop):
    """the four tap planes (float64, 0 where the index equals the size), the weights and the outside mask of the window"""
    n, sh, sw = vol.shape
    y0, x0, oh, ow = crop_window(zh, zw, crop)
    iy, ty, oy = (a[y0:y0 + oh] for a in axis_terms(sh, zh))
    ix, tx, ox = (a[x0:x0 + ow] for a in axis_terms(sw, zw))
    pad = np.zeros((n, sh + 1, sw + 1), np.float64)
    pad[:, :sh, :sw] = vol
    iy, ix = np.minimum(iy, sh - 1), np.minimum(ix, sw - 1)
    c = [pad[:, (iy + dy)[:, None], (ix + dx)[None, :]] for dy in (0, 1) for dx in (0, 1)]
    wy = ((1.0 - ty)[None, :, None], ty[None, :, None])
    wx = ((1.0 - tx)[None, None, :], tx[None, None, :])
    return c, wy, wx, (oy[:, None] | ox[None, :])[None]


def _accumulate(c, wy, wx, outside):
    acc = (c[0] * wy[0]) * wx[0]
    acc = acc + (c[1] * wy[0]) * wx[1]
    acc = acc + (c[2] * wy[1]) * wx[0]
    acc = acc + (c[3] * wy[1]) * wx[1]
    return np.where(outside, 0.0, acc)


def _round_to(acc, dtype):
    if dtype == np.float32:
        return acc.astype(np.float32)
    info = np.iinfo(dtype)
    r = np.where(acc > 0, acc + 0.5, acc - 0.5)
    return np.trunc(np.clip(r, info.min, info.max)).astype(dtype)


def zoom_rule(vol, zh, zw, crop=0):
    """the four-tap rule on [N,H,W] -> the crop window of the (zh, zw) zoomed slices, in the volume's dtype"""
    return _round_to(_accumulate(*_taps(vol, zh, zw, crop)), vol.dtype.type)


def remap_rule(raw, remap):
    v = raw.astype(np.int64)
    for a, b in remap:
        v = np.where(v == a, b, v)
    return v


def label_rule(raw, zh, zw, num_classes, remap=(), crop=0):
    """the fused label rule: per class the four taps over [label == c] as 0.0 / 1.0, rounded as uint8; the first class whose
    rounded channel is largest.  -> (uint8 labels, the number of input values outside [0, num_classes))"""
    v = remap_rule(raw, remap)
    best = None
    for c in range(num_classes):
        ch = _round_to(_accumulate(*_taps((v == c).astype(np.float64), zh, zw, crop)), np.uint8)
        if best is None:
            best, lab = ch.copy(), np.zeros(ch.shape, np.uint8)
        else:
            lab[ch > best] = c
            best = np.maximum(best, ch)
    return lab, int(np.count_nonzero((v < 0) | (v >= num_classes)))


def int_stats(x):
    """exact statistics of an integer array: mean = Sx / n in double; std = sqrt(double(n Sxx - Sx Sx) / (double(n) double(n)))
    with the numerator an exact integer, converted once (round to nearest even)"""
    flat = [int(v) for v in x.ravel()]
    n, s1, s2 = len(flat), sum(flat), sum(v * v for v in flat)
    return s1 / n, math.sqrt(float(n * s2 - s1 * s1) / (float(n) * float(n)))


def f32_stats(x):
    """this build's own convention for fp32 volumes: statistics of the fp32-rounded zoomed values accumulated in float64,
    mean first, then the mean of the squared deviations (numpy's float32 pairwise accumulation is NOT reproduced)"""
    d = x.astype(np.float64).ravel()
    mean = math.fsum(d) / d.size
    return mean, math.sqrt(math.fsum((d - mean) ** 2) / d.size)


def standardize_rule(z, mean, std):
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((z.astype(np.float64) - mean) / std).astype(np.float32)


def zoom_output_shape(shape_hw, zoom_yx):
    return tuple(int(round(d * f)) for d, f in zip(shape_hw, zoom_yx))


# ---------------------------------------------------------------------------------------------- the real thing
def zoom_scipy(vol, zh, zw, crop=0):
    from scipy import ndimage
    n, sh, sw = vol.shape
    out = ndimage.zoom(vol, [1, zh / sh, zw / sw], order=1)
    assert out.shape == (n, zh, zw) and out.dtype == vol.dtype, (out.shape, out.dtype)
    y0, x0, oh, ow = crop_window(zh, zw, crop)
    return np.ascontiguousarray(out[:, y0:y0 + oh, x0:x0 + ow])


def labels_scipy(raw, zh, zw, num_classes, remap=(), crop=0):
    """the reference's read_*_nii_label_save_npy: np.where chain, to_categorical (np.eye(..)[mask], channel first), zoom, argmax, crop"""
    from scipy import ndimage
    v = raw
    for a, b in remap:
        v = np.where(v == a, b, v)
    assert v.min() >= 0 and v.max() < num_classes
    onehot = np.moveaxis(np.eye(num_classes, dtype="uint8")[v], -1, 1)
    n, sh, sw = raw.shape
    masks = ndimage.zoom(onehot, [1, 1, zh / sh, zw / sw], order=1)
    assert masks.shape == (n, num_classes, zh, zw) and masks.dtype == np.uint8
    lab = np.argmax(masks, axis=1)
    y0, x0, oh, ow = crop_window(zh, zw, crop)
    return np.ascontiguousarray(lab[:, y0:y0 + oh, x0:x0 + ow]).astype(np.uint8), masks


def nearest_scipy(lab, zh, zw):
    from scipy import ndimage
    return ndimage.zoom(lab, [1, zh / lab.shape[1], zw / lab.shape[2]], order=0)


# ---------------------------------------------------------------------------------------------- inputs
def overshoot_pairs(limit=512):
    """(in, out) with double(out - 1) ((in - 1) / (out - 1)) > in - 1, both sizes in 2..limit, smallest in + out first"""
    found = [(i, o) for i in range(2, limit + 1) for o in range(2, limit + 1) if float(o - 1) * ((i - 1) / (o - 1)) > i - 1]
    return sorted(found, key=lambda p: (p[0] + p[1], p))


def volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        return (rng.standard_normal(shape) * 300.0 + 40.0).astype(np.float32)
    if dtype == np.int16:
        return rng.integers(-1200, 2500, shape).astype(np.int16)
    return rng.integers(0, 256, shape).astype(np.uint8)


def smooth_volume(shape, dtype, seed):
    """a production-like volume that still compresses: flat tissue (a background and three discs of constant intensity, shifted
    from slice to slice) crossed by a band of rows of full-entropy noise"""
    rng = np.random.default_rng(seed)
    n, h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    v = np.full(shape, 60.0)
    for k in range(n):
        for (cy, cx, r), level in zip(((0.50, 0.45, 0.22), (0.38, 0.60, 0.09), (0.63, 0.55, 0.06)), (400.0, 900.0, 250.0)):
            v[k][(y - cy * h - 3 * k) ** 2 + (x - cx * w + 2 * k) ** 2 <= (r * h) ** 2] = level
    band = slice(int(0.44 * h), int(0.52 * h))
    v[:, band] += rng.standard_normal((n, band.stop - band.start, w)) * 120.0
    if dtype == np.uint8:
        return np.clip(v / 5.0, 0, 255).astype(np.uint8)
    return (v - 150.0).astype(dtype)


def discs(codes, dtype, n=3):
    """three discs on a 24x28 grid (the second and third overlap the first's rim), one slice shifted by a pixel"""
    y, x = np.mgrid[0:24, 0:28]
    out = np.zeros((n, 24, 28), dtype)
    for k in range(n):
        for (cy, cx, r), code in zip(((11 + k, 9, 6.3), (8, 18 + k, 4.6), (17, 16, 3.7)), codes[1:]):
            out[k][(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = code
        out[k][out[k] == 0] = codes[0]
    return out


def zoom_cases():
    pair = overshoot_pairs()[0]
    shapes = [("20x24_to_21x25", 2, (20, 24), (21, 25), 0), ("20x24_to_13x9", 2, (20, 24), (13, 9), 0),
              ("7x5_to_16x3", 3, (7, 5), (16, 3), 0), ("5x6_identity", 2, (5, 6), (5, 6), 0), ("9x9_to_1x4", 2, (9, 9), (1, 4), 0),
              ("37x41_to_50x33_crop24", 2, (37, 41), (50, 33), 24), ("37x41_to_50x33", 2, (37, 41), (50, 33), 0),
              ("256x256_to_267x267_crop224", 2, (256, 256), (267, 267), 224),
              ("overshoot_rows_%dx5_to_%dx7" % pair, 1, (pair[0], 5), (pair[1], 7), 0),
              ("overshoot_cols_5x%d_to_6x%d" % pair, 1, (5, pair[0]), (6, pair[1]), 0)]
    for k, (name, n, src, dst, crop) in enumerate(shapes):
        for tag, dt in DTYPES:
            if name.startswith("256"):
                vol = smooth_volume((n,) + src, dt, 900 + k)
            else:
                vol = volume((n,) + src, dt, 100 + 10 * (5 if name == "37x41_to_50x33" else k) + len(tag))   # (the crop case's volume)
                if name.startswith("overshoot"):
                    vol = (np.abs(vol.astype(np.float64)) + 1).astype(dt) if dt != np.uint8 else np.maximum(vol, 1)   # no zero at the edge
            yield "%s_%s" % (tag, name), vol, dst[0], dst[1], crop


def label_cases():
    raw = discs((0, 200, 500, 600), np.int16)
    for zh, zw in ((25, 29), (31, 37), (17, 19)):
        yield "i16_discs_to_%dx%d" % (zh, zw), raw, zh, zw, 4, REMAP, 0
    yield "i16_discs_to_31x37_crop24", raw, 31, 37, 4, REMAP, 24
    yield "u8_discs5_to_31x37", discs((0, 1, 4, 2), np.uint8), 31, 37, 5, (), 0
    pair = overshoot_pairs()[0]
    edge = np.full((1, pair[0], 5), 600, np.int16)
    edge[0, :, 2:] = 200
    yield "i16_overshoot_rows_%dx5_to_%dx7" % pair, edge, pair[1], 7, 4, REMAP, 0


def stat_cases():
    """standardize: (name, volume, zh, zw, crop).  The fp32 volumes of the first kind hold multiples of 2^-10 in [64, 256): their
    zoomed values are multiples of 2^-17 below 2^8, so a float64 sum of fewer than 2^28 of them is exact in any order."""
    rng = np.random.default_rng(77)
    yield "i16_256x256_to_267x267_crop224", smooth_volume((2, 256, 256), np.int16, 31), 267, 267, 224
    yield "i16_37x41_to_50x33_crop24", volume((3, 37, 41), np.int16, 32), 50, 33, 24
    yield "u8_20x24_to_21x25", volume((2, 20, 24), np.uint8, 33), 21, 25, 0
    yield "i16_constant", np.full((2, 9, 9), -7, np.int16), 12, 12, 8
    exact = (rng.integers(64 * 1024, 256 * 1024, (2, 37, 41)) / 1024.0).astype(np.float32)
    yield "f32_exact_sums_37x41_to_50x33_crop24", exact, 50, 33, 24
    yield "f32_mixed_sign_20x24_to_21x25", volume((2, 20, 24), np.float32, 34), 21, 25, 0


# ---------------------------------------------------------------------------------------------- the file
def build(verbose=False):
    import scipy
    say = print if verbose else (lambda *a: None)
    out = {"scipy_version": np.array(scipy.__version__), "numpy_version": np.array(np.__version__)}
    pairs = overshoot_pairs()
    if not pairs:
        raise SystemExit("no (in, out) pair up to 512 overshoots: say so in DESIGN.md and drop the overshoot cases")
    say("overshooting (in, out) pairs with sizes 2..512: %d, the smallest %s: scipy returns cval = 0 there, not the edge value"
        % (len(pairs), pairs[0]))
    out["overshoot_pair"], out["overshoot_pairs_up_to_512"] = np.array(pairs[0]), np.array(len(pairs))
    names = []
    for name, vol, zh, zw, crop in zoom_cases():
        want, mine = zoom_scipy(vol, zh, zw, crop), zoom_rule(vol, zh, zw, crop)
        if not bit_equal(want, mine):
            raise SystemExit("zoom case %s: the restatement differs from scipy in %d values" % (name, np.count_nonzero(want != mine)))
        if "overshoot" in name:
            edge = want[:, -1, :] if "rows" in name else want[:, :, -1]
            assert not edge.any() and vol.min() > 0, name
        out["zoom/%s/in" % name], out["zoom/%s/scipy" % name], out["zoom/%s/rule" % name] = vol, want, mine
        out["zoom/%s/geom" % name] = np.array([zh, zw, crop])
        names.append(name)
    out["zoom_cases"] = np.array(names)
    names = []
    for name, raw, zh, zw, ncls, remap, crop in label_cases():
        want, masks = labels_scipy(raw, zh, zw, ncls, remap, crop)
        mine, stray = label_rule(raw, zh, zw, ncls, remap, crop)
        if not bit_equal(want, mine) or stray:
            raise SystemExit("label case %s: the fused rule differs from argmax(zoom(onehot)) in %d pixels" % (name, np.count_nonzero(want != mine)))
        if "discs_to" in name and not crop:
            near = nearest_scipy(remap_rule(raw, remap), zh, zw)
            differ, none, two = (int(np.count_nonzero(near != want)), int(np.count_nonzero(masks.sum(1) == 0)),
                                 int(np.count_nonzero(masks.sum(1) >= 2)))
            say("%s: %d pixels differ from nearest-neighbour zoom, %d have all channels 0, %d have two channels 1" % (name, differ, none, two))
            assert differ >= 10 and two >= 1, name
            assert none >= 1 or (zh, zw) == (17, 19), name
            out["labels/%s/counts" % name] = np.array([differ, none, two])
        out["labels/%s/in" % name], out["labels/%s/scipy" % name], out["labels/%s/rule" % name] = raw, want, mine
        out["labels/%s/geom" % name] = np.array([zh, zw, crop, ncls])
        out["labels/%s/remap" % name] = np.array(remap, np.int64).reshape(-1, 2)
        names.append(name)
    out["label_cases"] = np.array(names)
    names = []
    for name, vol, zh, zw, crop in stat_cases():
        z = zoom_scipy(vol, zh, zw, crop)
        assert bit_equal(z, zoom_rule(vol, zh, zw, crop)), name
        if vol.dtype == np.float32:
            mean, std = f32_stats(z)
            d = z.astype(np.float64)
            ref_mean, ref_std = float(np.mean(d)), float(np.std(d))
            if "exact" in name:
                from fractions import Fraction
                s = sum(Fraction(float(v)) for v in d.ravel())
                assert s == Fraction(float(np.sum(d))) == Fraction(math.fsum(d.ravel())), "the sum is exact in float64 in any order"
                assert mean == ref_mean, name
            assert abs(mean - ref_mean) <= d.size * 2.0 ** -53 * float(np.mean(np.abs(d))), name
        else:
            mean, std = int_stats(z)
            ref_mean, ref_std = float(np.mean(z)), float(np.std(z))       # the reference: image.mean(), image.std()
            if mean != ref_mean:
                raise SystemExit("stat case %s: the integer mean differs from numpy.mean" % name)
        if abs(std - ref_std) > z.size * 2.0 ** -53 * ref_std:
            raise SystemExit("stat case %s: std %r against numpy's %r" % (name, std, ref_std))
        with np.errstate(divide="ignore", invalid="ignore"):
            numpy_out = ((z - ref_mean) / ref_std).astype(np.float32) if vol.dtype != np.float32 else standardize_rule(z, ref_mean, ref_std)
        mine = standardize_rule(z, mean, std)
        differ = int(np.count_nonzero(mine.view(np.uint32) != numpy_out.view(np.uint32)))
        say("%s: mean %r std %r (numpy's %r %r), %d of %d fp32 outputs differ from numpy's" % (name, mean, std, ref_mean, ref_std, differ, z.size))
        if std > 0 and differ * 100 > z.size:
            raise SystemExit("stat case %s: more than 1 %% of the outputs differ from numpy's" % name)
        out["stats/%s/in" % name], out["stats/%s/geom" % name] = vol, np.array([zh, zw, crop])
        out["stats/%s/numpy_stats" % name], out["stats/%s/rule_stats" % name] = np.array([ref_mean, ref_std]), np.array([mean, std])
        out["stats/%s/numpy" % name], out["stats/%s/rule" % name] = numpy_out, mine
        names.append(name)
    out["stat_cases"] = np.array(names)
    return out


def load_cases(g):
    """-> (zoom cases, label cases, stat cases) as lists of dicts"""
    zoom = [dict(name=str(n), vol=g["zoom/%s/in" % n], scipy=g["zoom/%s/scipy" % n], rule=g["zoom/%s/rule" % n],
                 zh=int(g["zoom/%s/geom" % n][0]), zw=int(g["zoom/%s/geom" % n][1]), crop=int(g["zoom/%s/geom" % n][2]))
            for n in g["zoom_cases"]]
    labels = [dict(name=str(n), raw=g["labels/%s/in" % n], scipy=g["labels/%s/scipy" % n], rule=g["labels/%s/rule" % n],
                   zh=int(g["labels/%s/geom" % n][0]), zw=int(g["labels/%s/geom" % n][1]), crop=int(g["labels/%s/geom" % n][2]),
                   num_classes=int(g["labels/%s/geom" % n][3]), remap=tuple((int(a), int(b)) for a, b in g["labels/%s/remap" % n]),
                   counts=g["labels/%s/counts" % n] if "labels/%s/counts" % n in g else None)
              for n in g["label_cases"]]
    stats = [dict(name=str(n), vol=g["stats/%s/in" % n], zh=int(g["stats/%s/geom" % n][0]), zw=int(g["stats/%s/geom" % n][1]),
                  crop=int(g["stats/%s/geom" % n][2]), numpy_stats=g["stats/%s/numpy_stats" % n], rule_stats=g["stats/%s/rule_stats" % n],
                  numpy=g["stats/%s/numpy" % n], rule=g["stats/%s/rule" % n])
             for n in g["stat_cases"]]
    return zoom, labels, stats


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_file():
    """regenerates every array and compares it with the file's -> the number of arrays compared"""
    new, old = build(), np.load(PATH)
    keys = [k for k in new if not k.endswith("_version")]
    assert sorted(k for k in old.files if not k.endswith("_version")) == sorted(keys)
    for k in keys:
        assert bit_equal(new[k], old[k]), k
    return len(keys)


# ---------------------------------------------------------------------------------------------- the second file: dispatch edges
# tests/golden/resample_edges.npz holds the shapes at which the kernels of csrc/resample.hip take a branch that no case of
# resample.npz reaches: more than one band of rows of labels, real ties and four classes under a pixel, eight classes and eight
# remap pairs, a statistics reduce that loops, a variance numerator beyond 64 bits, the capped second pass of the fp32
# statistics, weights of exactly 0.5, rows wider than 1024 columns, one output column, an input axis of one sample.  The same
# discipline: the expected arrays are scipy's / numpy's own outputs and the file is written only if the restatement equals them
# bit for bit.  The statistics cases do not store the zoomed or standardised arrays (they would not fit): the file holds the
# input (or the generator builds it from an integer formula), numpy's mean() and std() as doubles and a SHA-256 of scipy's
# zoomed bytes; a test recomputes the arrays with zoom_rule and checks the digest before it trusts them.
EDGES_PATH = os.path.join(ROOT, "tests", "golden", "resample_edges.npz")
# eight pairs onto the classes 0..7 (class 0 is the raw code 0); the first two chain: 7 -> 200 -> 1.  (421, 7) stands after
# (7, 200), so a 421 stays class 7.
REMAP8 = ((7, 200), (200, 1), (500, 2), (600, 3), (820, 4), (-5, 5), (1000, 6), (421, 7))
REMAP8_CODES = (0, 200, 500, 600, 820, -5, 1000, 421)


def accumulator(vol, zh, zw, crop=0):
    """the float64 value of every output pixel before it is rounded into the volume's dtype"""
    return _accumulate(*_taps(vol, zh, zw, crop))


def half_ties(vol, zh, zw, crop=0):
    """-> (outputs whose float64 accumulator has a fraction of exactly 0.5, those of them that are negative)"""
    acc = accumulator(vol, zh, zw, crop)
    tie = np.abs(acc - np.trunc(acc)) == 0.5
    return int(np.count_nonzero(tie)), int(np.count_nonzero(tie & (acc < 0)))


def channel_counts(raw, zh, zw, num_classes, remap=(), crop=0):
    """of the fused rule's rounded channels inside the crop window -> (pixels with every channel 0, pixels with two or more at 1)"""
    v = remap_rule(raw, remap)
    ones = sum(_round_to(accumulator((v == c).astype(np.float64), zh, zw, crop), np.uint8).astype(np.int64) for c in range(num_classes))
    return int(np.count_nonzero(ones == 0)), int(np.count_nonzero(ones >= 2))


def sha256_hex(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def int_sums(x):
    """(n, Sx, Sxx) of an integer array as Python integers"""
    flat = [int(v) for v in x.ravel()]
    return len(flat), sum(flat), sum(v * v for v in flat)


def blocks8(n=3):
    """n slices of 40x44 made of 4x4 blocks of the classes 0..7; a block's four neighbours and its diagonal ones all differ from it"""
    by, bx = np.mgrid[0:40, 0:44] // 4
    return np.stack([(bx + 3 * by + 5 * k) % 8 for k in range(n)]).astype(np.uint8)


def noise8(shape, seed=5):
    """per-pixel random classes 0..7"""
    return np.random.default_rng(seed).integers(0, 8, shape).astype(np.uint8)


def noise8_raw_codes(shape, seed=5):
    """the same noise as int16 raw codes of REMAP8; class 1 is written as 7 (which chains through 200) in every other place"""
    cls = noise8(shape, seed).astype(np.int64)
    raw = np.array(REMAP8_CODES, np.int64)[cls]
    flat = raw.ravel()
    ones = np.flatnonzero(flat == 200)
    flat[ones[::2]] = 7
    return flat.reshape(shape).astype(np.int16)


def fullscale_volume(seed=6):
    """3 slices of 32x32 int16, magnitudes 28000..32767, positive left of column 14 and negative elsewhere"""
    mag = np.random.default_rng(seed).integers(28000, 32768, (3, 32, 32))
    mag[:, :, 14:] *= -1
    return mag.astype(np.int16)


def nearconstant_volume():
    v = np.full((4, 32, 32), 30000, np.int16)
    v[1, 16, 16] = 29999
    return v


def exact_volume(shape=(42, 64, 64)):
    """fp32 multiples of 2^-10 in [64, 256) by an integer formula (no random numbers): a test rebuilds it instead of reading it"""
    k, i, j = (a.astype(np.int64) for a in np.indices(shape))
    q = 64 * 1024 + (k * 1299709 + i * 104729 + j * 7919 + i * j * 31 + k * k * 17) % (192 * 1024)
    return (q / 1024.0).astype(np.float32)


def exact_sum_scaled(z):
    """the proof that a float64 sum of the fp32 values z is exact in any order: scaled by 2^17 they are non-negative integers
    whose sum stays below 2^53 -> that sum, a Python integer"""
    q = z.astype(np.float64) * 2.0 ** 17
    assert np.all(q == np.floor(q)) and np.all(q >= 0) and float(q.max()) < 2.0 ** 26, "multiples of 2^-17 below 2^9"
    total = sum(int(v) for v in q.astype(np.int64).ravel())
    assert total < 2 ** 53
    return total


def edge_zoom_cases():
    shapes = [("9x5_to_17x17", 2, (9, 5), (17, 17)), ("3x300_to_5x1030", 1, (3, 300), (5, 1030)), ("3x300_to_5x1028", 1, (3, 300), (5, 1028)),
              ("6x1_to_9x4", 2, (6, 1), (9, 4)), ("1x6_to_4x9", 2, (1, 6), (4, 9)), ("6x7_to_40x1", 2, (6, 7), (40, 1))]
    for k, (name, n, src, dst) in enumerate(shapes):
        for tag, dt in DTYPES:
            yield "%s_%s" % (tag, name), volume((n,) + src, dt, 300 + 10 * k + len(tag)), dst[0], dst[1], 0
    limits = np.array([[[-32768, 32767], [32767, -32768]], [[32767, 32767], [-32768, -32768]]], np.int16)
    yield "i16_2x2_to_9x9_limits", limits, 9, 9, 0


def edge_label_cases():
    """(name, raw, zh, zw, classes, remap, crop, (least number of all-zero pixels, of pixels with two channels at 1) or None)"""
    yield "u8_blocks8_to_267x267_crop224", blocks8(), 267, 267, 8, (), 224, (100, 100)
    noise = noise8((2, 40, 44))
    yield "u8_noise8_to_70x76_crop64", noise, 70, 76, 8, (), 64, None
    yield "u8_noise8_to_70x75", noise, 70, 75, 8, (), 0, None
    yield "i16_noise_remap8_to_70x76_crop64", noise8_raw_codes((2, 40, 44)), 70, 76, 8, REMAP8, 64, None
    yield "u8_noise8_9x11_to_17x21", noise8((2, 9, 11), 51), 17, 21, 8, (), 0, (20, 100)
    yield "u8_noise8_1x9_to_3x17", noise8((2, 1, 9), 52), 3, 17, 8, (), 0, None
    yield "u8_noise8_9x1_to_17x3", noise8((2, 9, 1), 53), 17, 3, 8, (), 0, None
    yield "u8_noise8_3x300_to_5x1030", noise8((1, 3, 300), 54), 5, 1030, 8, (), 0, None


def edge_stat_cases():
    for k, (tag, dt) in enumerate(DTYPES):
        yield "%s_many_520x3x3_to_33x4" % tag, volume((520, 3, 3), dt, 400 + k), 33, 4, 0
    yield "i16_fullscale_3x32x32_to_267x267_crop224", fullscale_volume(), 267, 267, 224
    yield "i16_nearconstant_4x32x32_to_267x267_crop224", nearconstant_volume(), 267, 267, 224
    yield "f32_exact_42x64x64_to_267x267_crop224", exact_volume(), 267, 267, 224


def build_edges(verbose=False):
    import scipy
    say = print if verbose else (lambda *a: None)
    out = {"scipy_version": np.array(scipy.__version__), "numpy_version": np.array(np.__version__)}
    names = []
    for name, vol, zh, zw, crop in edge_zoom_cases():
        want, mine = zoom_scipy(vol, zh, zw, crop), zoom_rule(vol, zh, zw, crop)
        if not bit_equal(want, mine):
            raise SystemExit("zoom case %s: the restatement differs from scipy in %d values" % (name, np.count_nonzero(want != mine)))
        if "9x5_to_17x17" in name and vol.dtype != np.float32:
            half, negative = half_ties(vol, zh, zw, crop)
            say("%s: %d accumulators with a fraction of exactly 0.5, %d of them negative" % (name, half, negative))
            assert half >= 100 and (vol.dtype != np.int16 or negative >= 20), name
            out["zoom/%s/ties" % name] = np.array([half, negative])
        if "limits" in name:
            assert sorted(np.unique(vol).tolist()) == [-32768, 32767] and want.min() == -32768 and want.max() == 32767, name
        out["zoom/%s/in" % name], out["zoom/%s/scipy" % name] = vol, want
        out["zoom/%s/geom" % name] = np.array([zh, zw, crop])
        names.append(name)
    out["zoom_cases"] = np.array(names)
    names = []
    for name, raw, zh, zw, ncls, remap, crop, least in edge_label_cases():
        want, masks = labels_scipy(raw, zh, zw, ncls, remap, crop)
        mine, stray = label_rule(raw, zh, zw, ncls, remap, crop)
        if not bit_equal(want, mine) or stray:
            raise SystemExit("label case %s: the fused rule differs from argmax(zoom(onehot)) in %d pixels" % (name, np.count_nonzero(want != mine)))
        y0, x0, oh, ow = crop_window(zh, zw, crop)
        ones = masks[:, :, y0:y0 + oh, x0:x0 + ow].astype(np.int64).sum(1)
        none, two = int(np.count_nonzero(ones == 0)), int(np.count_nonzero(ones >= 2))
        assert (none, two) == channel_counts(raw, zh, zw, ncls, remap, crop), name
        say("%s: of %d pixels %d have all channels 0, %d have two or more channels 1" % (name, want.size, none, two))
        if least:
            assert none >= least[0] and two >= least[1], (name, none, two)
        classes = np.unique(remap_rule(raw, remap)).tolist()
        assert set(classes) <= set(range(8)) and 7 in classes and (raw.size < 64 or classes == list(range(8))), name
        out["labels/%s/in" % name], out["labels/%s/scipy" % name] = raw, want
        out["labels/%s/geom" % name] = np.array([zh, zw, crop, ncls])
        out["labels/%s/remap" % name] = np.array(remap, np.int64).reshape(-1, 2)
        out["labels/%s/counts" % name] = np.array([none, two])
        names.append(name)
    out["label_cases"] = np.array(names)
    names = []
    for name, vol, zh, zw, crop in edge_stat_cases():
        z = zoom_scipy(vol, zh, zw, crop)
        assert bit_equal(z, zoom_rule(vol, zh, zw, crop)), name
        if vol.dtype == np.float32:
            mean, std = f32_stats(z)
            d = z.astype(np.float64)
            ref_mean, ref_std = float(np.mean(d)), float(np.std(d))
            if "exact" in name:
                total = exact_sum_scaled(z)
                assert mean == ref_mean == float(total) / 2.0 ** 17 / z.size, name
            assert abs(mean - ref_mean) <= d.size * 2.0 ** -53 * float(np.mean(np.abs(d))), name
        else:
            mean, std = int_stats(z)
            ref_mean, ref_std = float(np.mean(z)), float(np.std(z))       # the reference: image.mean(), image.std()
            if mean != ref_mean:
                raise SystemExit("stat case %s: the integer mean differs from numpy.mean" % name)
            n, s1, s2 = int_sums(z)
            bits = (n * s2).bit_length(), (n * s2 - s1 * s1).bit_length()
            say("%s: n Sxx needs %d bits, the numerator n Sxx - Sx Sx %d, Sx = %d" % (name, bits[0], bits[1], s1))
            if "fullscale" in name:
                assert n * s2 - s1 * s1 >= 2 ** 64 and n * s2 >= 2 ** 64 and s1 < 0, name
            if "nearconstant" in name:
                assert bits == (65, 24) and abs(std - 0.01497) < 1e-5, (name, bits, std)
            out["stats/%s/bits" % name] = np.array(bits + (-1 if s1 < 0 else 1,))
        if abs(std - ref_std) > z.size * 2.0 ** -53 * ref_std:
            raise SystemExit("stat case %s: std %r against numpy's %r" % (name, std, ref_std))
        numpy_out = ((z - ref_mean) / ref_std).astype(np.float32) if vol.dtype != np.float32 else standardize_rule(z, ref_mean, ref_std)
        differ = int(np.count_nonzero(standardize_rule(z, mean, std).view(np.uint32) != numpy_out.view(np.uint32)))
        say("%s: mean %r std %r (numpy's %r %r), %d of %d fp32 outputs differ from numpy's" % (name, mean, std, ref_mean, ref_std, differ, z.size))
        if differ * 100 > z.size:
            raise SystemExit("stat case %s: more than 1 %% of the outputs differ from numpy's" % name)
        if "exact" in name:
            assert bit_equal(vol, exact_volume()), "rebuilt by the test, not stored"
        else:
            out["stats/%s/in" % name] = vol
        out["stats/%s/geom" % name] = np.array([zh, zw, crop])
        out["stats/%s/numpy_stats" % name], out["stats/%s/rule_stats" % name] = np.array([ref_mean, ref_std]), np.array([mean, std])
        out["stats/%s/sha256" % name], out["stats/%s/differ" % name] = np.array(sha256_hex(z)), np.array(differ)
        names.append(name)
    out["stat_cases"] = np.array(names)
    return out


def load_edge_cases(g):
    """-> (zoom cases, label cases, stat cases) of the second file as lists of dicts; a statistics case holds no expected array
    (expected_stat_arrays rebuilds them) and the exact-sum fp32 volume comes from exact_volume()"""
    zoom = [dict(name=str(n), vol=g["zoom/%s/in" % n], scipy=g["zoom/%s/scipy" % n], zh=int(g["zoom/%s/geom" % n][0]),
                 zw=int(g["zoom/%s/geom" % n][1]), crop=int(g["zoom/%s/geom" % n][2]),
                 ties=g["zoom/%s/ties" % n] if "zoom/%s/ties" % n in g else None)
            for n in g["zoom_cases"]]
    labels = [dict(name=str(n), raw=g["labels/%s/in" % n], scipy=g["labels/%s/scipy" % n], zh=int(g["labels/%s/geom" % n][0]),
                   zw=int(g["labels/%s/geom" % n][1]), crop=int(g["labels/%s/geom" % n][2]), num_classes=int(g["labels/%s/geom" % n][3]),
                   remap=tuple((int(a), int(b)) for a, b in g["labels/%s/remap" % n]), counts=g["labels/%s/counts" % n])
              for n in g["label_cases"]]
    stats = [dict(name=str(n), vol=g["stats/%s/in" % n] if "stats/%s/in" % n in g else exact_volume(), zh=int(g["stats/%s/geom" % n][0]),
                  zw=int(g["stats/%s/geom" % n][1]), crop=int(g["stats/%s/geom" % n][2]), numpy_stats=g["stats/%s/numpy_stats" % n],
                  rule_stats=g["stats/%s/rule_stats" % n], sha256=str(g["stats/%s/sha256" % n]), differ=int(g["stats/%s/differ" % n]),
                  bits=g["stats/%s/bits" % n] if "stats/%s/bits" % n in g else None)
             for n in g["stat_cases"]]
    return zoom, labels, stats


def expected_stat_arrays(case):
    """a statistics case of the second file -> (zoomed values, numpy's standardised fp32 outputs).  The zoomed values are the
    restatement's and are trusted only because their SHA-256 equals the one taken of scipy's bytes when the file was made."""
    z = np.ascontiguousarray(zoom_rule(case["vol"], case["zh"], case["zw"], case["crop"]))
    if sha256_hex(z) != case["sha256"]:
        raise AssertionError("%s: the restatement's zoomed values are not the ones scipy gave" % case["name"])
    ref_mean, ref_std = (float(v) for v in case["numpy_stats"])
    if z.dtype == np.float32:
        return z, standardize_rule(z, ref_mean, ref_std)
    return z, ((z - ref_mean) / ref_std).astype(np.float32)


def check_edges_file():
    """regenerates every array of the second file and compares it with the file's -> the number of arrays compared"""
    new, old = build_edges(), np.load(EDGES_PATH)
    keys = [k for k in new if not k.endswith("_version")]
    assert sorted(k for k in old.files if not k.endswith("_version")) == sorted(keys)
    for k in keys:
        assert bit_equal(new[k], old[k]), k
    return len(keys)


if __name__ == "__main__":
    if "--check" in sys.argv[1:]:
        print("%d arrays equal the file's" % check_file())
        print("%d arrays equal those of %s" % (check_edges_file(), os.path.relpath(EDGES_PATH, ROOT)))
    else:
        for path, arrays in ((PATH, build(verbose=True)), (EDGES_PATH, build_edges(verbose=True))):
            if os.path.exists(path):
                old = np.load(path)
                if sorted(old.files) == sorted(arrays) and all(bit_equal(arrays[k], old[k]) for k in arrays):
                    print("%s already holds these %d arrays: left as it is" % (os.path.relpath(path, ROOT), len(arrays)))
                    continue
            np.savez_compressed(path, **arrays)
            print("wrote %s: %d arrays, %d bytes" % (os.path.relpath(path, ROOT), len(arrays), os.path.getsize(path)))
