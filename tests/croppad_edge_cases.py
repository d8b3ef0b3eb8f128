"""The case table of the CropAndPad edge tests (tests/test_croppad_edges.py, tests/test_croppad_edges_gpu.py) and of
``scripts/make_croppad_golden.py --edges``: plain data plus seeded input builders, numpy and the generator's restatement only.

tests/golden/croppad.npz stops at 64 x 48 and C in {1, 3}; csrc/croppad.hip takes other paths above that.  Every case below is
the smallest shape at which one of them is first reached:

  two_tiles_tail   18 x 65 (C = 1, 3)   tiles_x = 2 with a one-pixel second tile, two y tiles, the byte tail
  two_tiles_full   17 x 128 x 1         two full x tiles; 32-bit image stores and 16-byte label stores
  c2_vec_tail      20 x 66 x 2          W C % 4 == 0 with W % 4 == 2: word stores plus a partial last lane group
  c4               19 x 65, 16 x 64     C = 4 (the word path), with and without a row tail
  long_lines       80 x 70 x 3          cropped rows and columns above 64: a second trip of every wave loop (sum, max, min, the
                                        median's histogram), more than four lines per workgroup over both kinds of line
  max_pad          130 x 90 x 3         pads of exactly 64 on all four sides (Hi = H + 128); Wc C = 270 and Hc C = 390 edge values,
                                        a second trip of the ramp-flag loops
  production       256 x 256 x 3, 224 x 224 x 1   the workload: four x tiles, 16 and 14 y tiles

A case of kind "modes" runs all ten modes in one batch, once per side set: batch r gives mode m the side set (r + m) % S, so
every mode meets every set.  The kinds "stats" and "ramp" hold the images built for one kernel path (see their builders).
A row is (top, right, bottom, left, mode, cval) and passes ``G.sides_valid``."""
import hashlib
import importlib.util
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _load("make_croppad_golden")
JSON_PATH = os.path.join(ROOT, "tests", "golden", "croppad_edges.json")
LOOPS_BELOW = 100                      # the Python-loop twin of the resize runs where H and W are both below this
LABEL_VALUES = (-7, 0, 4, 70000, -2 ** 31 + 1)

# name, H, W, C, image: () -> uint8 [H, W, C], rows, kind ("modes" / "stats" / "ramp"), sets: the side sets behind the rows
Case = namedtuple("Case", "name h w c image rows kind sets")


def digest(a):
    """sha256 of an array's bytes (C order)"""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------- input builders
def few_values_image(h, w, c, seed):
    """only the grey levels 0, 131 and 255, their shares drawn per column: medians tie inside one histogram bin, and the bins 0
    and 255 (the first and the last lane's) are hit"""
    rng = np.random.default_rng(seed)
    share = rng.dirichlet((1.0, 1.0, 1.0), size=(w, c))                       # [W, C, 3]
    u = rng.random((h, w, c))
    idx = (u > share[None, :, :, 0]).astype(np.int64) + (u > share[None, :, :, 0] + share[None, :, :, 1])
    img = np.array([0, 131, 255], dtype=np.uint8)[idx]
    img[0, 0], img[1, 0], img[2, 0] = 0, 131, 255
    return img


def constant_image(h, w, c):
    """one value per channel: 77, 0, 255, 1"""
    return np.broadcast_to(np.array([77, 0, 255, 1], dtype=np.uint8)[:c], (h, w, c)).copy()


def half_image_66(h, w, c, axis):
    """G.half_image() at length 66: along `axis` the first 66 texels of line j (channel k) hold v and v + 1 33 times each
    (shuffled), v = (3 j + 50 k) % 200, so mean and median over them are v + 0.5 for even and odd v.  The texels behind the
    66th hold v + 40: a crop that keeps them changes every statistic"""
    assert (h, w)[axis] >= 66
    rng = np.random.default_rng(66 + axis)
    n_lines, n_len = ((w, h) if axis == 0 else (h, w))
    img = np.zeros((n_lines, n_len, c), dtype=np.uint8)                       # [line, position, channel]
    for j in range(n_lines):
        for k in range(c):
            v = (3 * j + 50 * k) % 200
            img[j, :66, k] = v + rng.permutation(np.arange(66) % 2)
            img[j, 66:, k] = v + 40
    return np.ascontiguousarray(img.transpose(1, 0, 2)) if axis == 0 else img


# The two forms of linspace differ only where k delta / width is an integer that one of them misses by rounding: never at
# a width of 64 (k / 64 and delta / 64 are exact), at width 55 and end value 0 for 49 pairs (k, edge value)
RAMP_CVAL = 0
RAMP_ALL, RAMP_LR = (55, 55, 55, 55), (0, 55, 0, 55)
# side -> (the planted texel (y, x, channel), the side set it is used with).  With a top or bottom pad the outermost pad row is
# cval itself, so left and right take the k / width form anyway: the left and right texels are planted under a pure
# left / right pad.  Flat index in the side's flag loop: x C + k for top / bottom, y C + k for left / right, all >= 256
RAMP_PLANTS = {"top": ((0, 88, 2), RAMP_ALL), "bottom": ((129, 86, 1), RAMP_ALL),
               "left": ((120, 0, 1), RAMP_LR), "right": ((100, 89, 0), RAMP_LR)}


def ramp_base_image():
    """130 x 90 x 3 noise in 1..255 (RAMP_CVAL = 0 occurs nowhere)"""
    return np.random.default_rng(130).integers(1, 256, (130, 90, 3)).astype(np.uint8)


def ramp_image(side):
    """the base image with exactly one texel equal to RAMP_CVAL: an edge texel of `side` behind flat index 256 of that side"""
    img = ramp_base_image()
    if side is not None:
        img[RAMP_PLANTS[side][0]] = RAMP_CVAL
    return img


def side_band(side, shape, sides):
    """boolean mask of the padded array I: the pad region of one side (its corners included)"""
    pt, pb, pl, pr = G.split_sides(0, 0, *sides)[4:]
    m = np.zeros(shape, dtype=bool)
    if side == "top":
        m[:pt] = True
    elif side == "bottom":
        m[shape[0] - pb:] = True
    elif side == "left":
        m[:, :pl] = True
    else:
        m[:, shape[1] - pr:] = True
    return m


def ramp_output_regions(side):
    """two boolean [130, 90] masks of the OUTPUT of a planted ramp case: the texels whose four neighbours in I all lie in that
    side's pad region and off the planted texel's own line (there the planted and the unplanted image differ by the form of
    the ramp alone), and the texels that read nothing of that region and not the planted texel (there they are equal)"""
    (y, x, _), sides = RAMP_PLANTS[side]
    pt, pb, pl, pr = G.split_sides(130, 90, *sides)[4:]
    hi, wi = 130 + pt + pb, 90 + pl + pr
    y0, y1 = G._axis_terms(hi, 130)[:2]
    x0, x1 = G._axis_terms(wi, 90)[:2]
    off_y, off_x = (y0 != pt + y) & (y1 != pt + y), (x0 != pl + x) & (x1 != pl + x)
    all_y, all_x = np.ones(130, dtype=bool), np.ones(90, dtype=bool)
    if side == "top":
        ins, outs = (y1 < pt, off_x), (y0 >= pt, all_x)
    elif side == "bottom":
        ins, outs = (y0 >= hi - pb, off_x), (y1 < hi - pb, all_x)
    elif side == "left":
        ins, outs = (off_y, x1 < pl), (all_y, x0 >= pl)
    else:
        ins, outs = (off_y, x0 >= wi - pr), (all_y, x1 < wi - pr)
    inside = ins[0][:, None] & ins[1][None, :]
    outside = outs[0][:, None] & outs[1][None, :] & ~(~off_y[:, None] & ~off_x[None, :])
    assert inside.any() and outside.any() and not (inside & outside).any()
    return inside, outside


def labels_for(h, w, seed=0):
    """int32 [H, W] over LABEL_VALUES, every value present"""
    rng = np.random.default_rng(1000 * h + w + seed)
    lab = np.array(LABEL_VALUES, dtype=np.int32)[rng.integers(0, len(LABEL_VALUES), (h, w))]
    lab.ravel()[:len(LABEL_VALUES)] = LABEL_VALUES
    lab.ravel()[-len(LABEL_VALUES):] = LABEL_VALUES
    return lab


# ---------------------------------------------------------------------------------------------- the table
def percent_pixels(percent, size):
    """signed pixels of one side as the presets draw them: floor(percent size + 0.5)"""
    return int(np.floor(float(percent) * size + 0.5))


def side_sets(h, w, extra=()):
    """pads only, crops only, mixed, the largest valid pad on all four sides; then `extra`"""
    ph, pw = min(G.MAX_PAD, h - 1), min(G.MAX_PAD, w - 1)
    sets = [(3, 2, 1, 4), (-2, -1, -3, -2), (5, -2, -1, 6), (ph, pw, ph, pw)] + list(extra)
    assert len(set(sets)) == len(sets) and all(G.sides_valid(h, w, *s) for s in sets), (h, w, sets)
    return sets


def _mode_rows(sets, combo):
    """batch r, sample m: mode m with the side set (r + m) % S -- build()'s rotation, once per offset"""
    return [tuple(sets[(r + m) % len(sets)]) + (m, (37 * m + 11 * combo + 5 * r) % 256) for r in range(len(sets)) for m in range(10)]


def _cases():
    out = []

    def modes(name, h, w, c, seed, extra=()):
        sets = side_sets(h, w, extra)
        out.append(Case(name, h, w, c, lambda: G.test_image(h, w, c, seed), _mode_rows(sets, len(out)), "modes", sets))

    modes("two_tiles_tail_c1", 18, 65, 1, 301)
    modes("two_tiles_tail_c3", 18, 65, 3, 302)
    modes("two_tiles_full", 17, 128, 1, 303)
    modes("c2_vec_tail", 20, 66, 2, 304)
    modes("c4_tail", 19, 65, 4, 305)
    modes("c4_full", 16, 64, 4, 306)
    modes("long_lines", 80, 70, 3, 307)
    modes("max_pad", 130, 90, 3, 308)
    # the extremes of the recipe's percent range: the pair of the issue at 256, its percentages at 224, and what
    # floor(percent size + 0.5) makes of -5 % and +10 %
    lo, hi = -12 / 256.0, 25 / 256.0
    for name, n, c, seed in (("production_256", 256, 3, 309), ("production_224", 224, 1, 310)):
        a, b = percent_pixels(lo, n), percent_pixels(hi, n)
        a2, b2 = percent_pixels(-0.05, n), percent_pixels(0.1, n)
        modes(name, n, n, c, seed, extra=[(a, b, b, a), (a2, b2, b2, a2)])
    assert out[-2].sets[4] == (-12, 25, 25, -12) and out[-2].sets[5] == (-13, 26, 26, -13)

    # statistics over lines longer than a wave: a pure top / bottom pad (pad rows are statistics of statistics), a pure
    # left / right pad, both; the half images also cropped to 66 along their axis
    h, w, c = 80, 70, 3
    plain = [(9, 0, 7, 0), (0, 6, 0, 11), (5, 3, 4, 6)]

    def stats(name, image, sets):
        assert all(G.sides_valid(h, w, *s) for s in sets)
        rows = [tuple(s) + (m, 0) for s in sets for m in (3, 4, 5, 6)]
        out.append(Case(name, h, w, c, image, rows, "stats", list(sets)))

    stats("long_lines_few", lambda: few_values_image(h, w, c, 311), plain)
    stats("long_lines_const", lambda: constant_image(h, w, c), plain)
    stats("long_lines_half_cols", lambda: half_image_66(h, w, c, 0), plain + [(9, 0, -14, 0), (7, 5, -14, 3)])
    stats("long_lines_half_rows", lambda: half_image_66(h, w, c, 1), plain + [(0, -4, 0, 11), (6, -4, 3, 11)])

    # the ramp flags behind index 256 of their loops: one planted texel per image, plus the unplanted image under both sets
    for side in ("top", "right", "bottom", "left"):
        sides = RAMP_PLANTS[side][1]
        out.append(Case("max_pad_ramp_" + side, 130, 90, 3, (lambda s=side: ramp_image(s)), [sides + (2, RAMP_CVAL)], "ramp", [sides]))
    for tag, sides in (("all", RAMP_ALL), ("lr", RAMP_LR)):
        out.append(Case("max_pad_ramp_none_" + tag, 130, 90, 3, ramp_base_image, [sides + (2, RAMP_CVAL)], "ramp", [sides]))
    for cs in out:
        assert all(G.sides_valid(cs.h, cs.w, *r[:4]) and 0 <= r[4] <= 9 and 0 <= r[5] <= 255 for r in cs.rows), cs.name
    return out


CASES = _cases()
BY_NAME = {cs.name: cs for cs in CASES}
assert len(BY_NAME) == len(CASES)


def _check_ramp_plants():
    """each planted texel is the only edge value equal to RAMP_CVAL, sits behind flat index 256 of its side's loop, and the two
    forms of the ramp differ somewhere on that side for these values (as ramp_pair() does with 63 against 62)"""
    base = ramp_base_image()
    edges = np.concatenate([base[0].ravel(), base[-1].ravel(), base[:, 0].ravel(), base[:, -1].ravel()])
    assert not np.any(edges == RAMP_CVAL)
    for side, ((y, x, k), sides) in RAMP_PLANTS.items():
        assert (x if side in ("top", "bottom") else y) * 3 + k >= 256, side
        assert {"top": y == 0, "bottom": y == 129, "left": x == 0, "right": x == 89}[side]
        assert not (side in ("left", "right") and (y in (0, 129))) and not (side in ("top", "bottom") and x in (0, 89))
        pt, pb, pl, pr = G.split_sides(130, 90, *sides)[4:]
        planted = G.pad_restated(ramp_image(side), pt, pb, pl, pr, 2, RAMP_CVAL)
        plain = G.pad_restated(base, pt, pb, pl, pr, 2, RAMP_CVAL)
        diff = planted != plain
        band = side_band(side, diff.shape[:2], sides)
        # away from the planted texel's own line the edge values are the same: a difference there is the other form
        line = np.zeros(diff.shape[:2], dtype=bool)
        if side in ("top", "bottom"):
            line[:, pl + x] = True
        else:
            line[pt + y] = True
        assert np.any(diff[band & ~line]), side
        inside = np.zeros(diff.shape[:2], dtype=bool)
        inside[pt + y, pl + x] = True
        assert not np.any(diff[~band & ~inside]), side


_check_ramp_plants()


# ---------------------------------------------------------------------------------------------- expected values (computed once)
_CACHE = {}


def image_of(case):
    key = ("img", case.name)
    if key not in _CACHE:
        img = case.image()
        assert img.dtype == np.uint8 and img.shape == (case.h, case.w, case.c), case.name
        img.setflags(write=False)
        _CACHE[key] = img
    return _CACHE[key]


def expected_rows(case):
    """the live restatement of every row: a list of (I, output), read-only and shared by all tests"""
    key = ("rows", case.name)
    if key not in _CACHE:
        res = []
        for row in case.rows:
            big, out = G.crop_pad_restated(image_of(case), *row)
            big.setflags(write=False)
            out.setflags(write=False)
            res.append((big, out))
        _CACHE[key] = res
    return _CACHE[key]


def labels_of(case):
    key = ("lab", case.h, case.w)
    if key not in _CACHE:
        lab = labels_for(case.h, case.w)
        lab.setflags(write=False)
        _CACHE[key] = lab
    return _CACHE[key]


def expected_labels(case):
    """G.labels_restated per side set of the case"""
    key = ("labout", case.name)
    if key not in _CACHE:
        res = [G.labels_restated(labels_of(case), *s) for s in case.sets]
        for a in res:
            a.setflags(write=False)
        _CACHE[key] = res
    return _CACHE[key]


def digests_of(case):
    """what tests/golden/croppad_edges.json records of a case"""
    return {"shape": [case.h, case.w, case.c], "rows": [digest(o) for _, o in expected_rows(case)],
            "labels": [digest(a) for a in expected_labels(case)]}
