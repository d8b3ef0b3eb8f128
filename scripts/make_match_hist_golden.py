"""Generator of tests/golden/match_hist.npz: the expected values of the device-side histogram matching
(pointcloududa_amd/utils/histmatch.py, csrc/histmatch.hip).

skimage is not a dependency; its algorithm (skimage.exposure.match_histograms 0.16-0.18, multichannel=True) is restated twice
in plain numpy, and the two forms must agree BIT FOR BIT, in float64 and after the cast to the image's dtype:

* ``match_unique``: np.unique(return_inverse, return_counts) / np.cumsum / np.interp, the library's own lines
* ``match_sorted``: np.sort + np.searchsorted(.., 'right') for the count of values <= s, the template's distinct values from
  the run ends of its sorted plane, and np.interp's arithmetic written out with array operations

The cast: fp32 images round to nearest even (``astype(np.float32)``), uint8 images truncate toward zero (numpy's assignment
into a uint8 array).

    python scripts/make_match_hist_golden.py            # writes tests/golden/match_hist.npz
    python scripts/make_match_hist_golden.py --check    # regenerates and compares the array contents with the file"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "match_hist.npz")


# ------------------------------------------------------------------------------------------ restatement 1
def _plane_unique(s, t):
    """float64 result for one source plane ``s`` against one template plane ``t`` (any shapes)"""
    sv, inv, sc = np.unique(s.ravel(), return_inverse=True, return_counts=True)
    tv, tc = np.unique(t.ravel(), return_counts=True)
    sq = np.cumsum(sc) / s.size
    tq = np.cumsum(tc) / t.size
    return np.interp(sq, tq, tv)[inv.ravel()].reshape(s.shape)


# ------------------------------------------------------------------------------------------ restatement 2
def _plane_sorted(s, t):
    flat = s.ravel()
    cnt = np.searchsorted(np.sort(flat), flat, side="right")              # values <= s (-0.0 == +0.0)
    q = cnt.astype(np.float64) / np.float64(flat.size)
    ts = np.sort(t.ravel())
    last = np.concatenate([ts[1:] != ts[:-1], [True]])                      # the last element of every run of equal values
    tv = ts[last].astype(np.float64)
    tq = (np.flatnonzero(last) + 1).astype(np.float64) / np.float64(ts.size)
    n = len(tv)
    j = np.searchsorted(tq, q, side="right") - 1                            # the last index with tq[j] <= q
    j0 = np.clip(j, 0, n - 1)
    j1 = np.minimum(j0 + 1, n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (tv[j1] - tv[j0]) / (tq[j1] - tq[j0])
        r = slope * (q - tq[j0]) + tv[j0]
    r = np.where((j < 0) | (j >= n - 1) | (tq[j0] == q), tv[j0], r)
    return r.reshape(s.shape)


def _apply(plane_fn, images, reference):
    """float64 ``[B,H,W,C]`` (or ``[H,W,C]``) result of ``plane_fn`` per sample and channel"""
    images, reference = np.asarray(images), np.asarray(reference)
    if images.ndim == 3:
        return _apply(plane_fn, images[None], reference)[0]
    if images.shape[-1] != reference.shape[-1]:
        raise ValueError("number of channels in the input image and the reference image must match")
    out = np.empty(images.shape, dtype=np.float64)
    for b in range(images.shape[0]):
        for c in range(images.shape[-1]):
            out[b, ..., c] = plane_fn(images[b, ..., c], reference[..., c])
    return out


def cast(r64, dtype):
    """the float64 result as the image's dtype: what ``out[..., c] = r`` does for an ``out`` of that dtype"""
    out = np.empty(r64.shape, dtype=dtype)
    out[...] = r64
    return out


def match_unique64(images, reference):
    return _apply(_plane_unique, images, reference)


def match_sorted64(images, reference):
    return _apply(_plane_sorted, images, reference)


def match_unique(images, reference):
    return cast(match_unique64(images, reference), np.asarray(images).dtype)


def match_sorted(images, reference):
    return cast(match_sorted64(images, reference), np.asarray(images).dtype)


# ------------------------------------------------------------------------------------------ inputs
def normal_f32(shape, seed, loc=0.0, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale + loc).astype(np.float32)


def levels_f32(shape, seed, levels=37):
    rng = np.random.default_rng(seed)
    table = np.sort(rng.standard_normal(levels) * 100.0).astype(np.float32)
    return table[rng.integers(0, levels, shape)]


def key_coverage_f32(shape, seed):
    """negatives and positives, 1e-30 .. 1e30, subnormals, both zeros, +-inf, and random bit patterns (no NaN): every byte
    of the sort key varies"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    nan = ((bits >> 23) & 0xFF == 0xFF) & (bits & 0x7FFFFF != 0)
    bits[nan] &= np.uint32(0xFF800000)                                      # a NaN becomes +-inf
    v = bits.view(np.float32).copy()
    k = n // 2
    v[:k] = (np.sign(rng.standard_normal(k)) * 10.0 ** rng.uniform(-30.0, 30.0, k)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 3e-39, 1e-30, -1e-30, 1e30, -1e30, 0.0,
                        -0.0, np.inf, -np.inf], dtype=np.float32)
    at = rng.choice(n, 3 * len(special), replace=False)
    v[at] = np.tile(special, 3)
    return v.reshape(shape)


def random_u8(shape, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def smooth_u8(shape, seed):
    """a low-frequency uint8 image with a skewed histogram (what the stage meets in front of the photometric path)"""
    b, h, w, c = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty(shape, dtype=np.uint8)
    for i in range(b):
        for ch in range(c):
            f = rng.uniform(0.02, 0.2, 2)
            p = rng.uniform(0, 6.28, 2)
            v = (np.sin(f[0] * y + p[0]) * np.cos(f[1] * x + p[1]) * 0.5 + 0.5) ** 2
            out[i, ..., ch] = np.clip(v * 255.0 + rng.standard_normal((h, w)) * 4.0, 0, 255).astype(np.uint8)
    return out


def case_inputs():
    """(name, images [B,H,W,C], reference [Ht,Wt,C]) of every fixture case"""
    f32 = np.float32
    return [
        ("f32_normal_b3_64x64x3", normal_f32((3, 64, 64, 3), 1, 10.0, 50.0), normal_f32((48, 80, 3), 2, -5.0, 20.0)),
        ("f32_normal_33x47x3_ref50x20", normal_f32((1, 33, 47, 3), 3), normal_f32((50, 20, 3), 4, 1.0, 3.0)),
        ("f32_keys_40x24x2", key_coverage_f32((1, 40, 24, 2), 5), normal_f32((31, 17, 2), 6, 0.0, 1000.0)),
        ("f32_ties_33x47x3", levels_f32((1, 33, 47, 3), 7), levels_f32((50, 20, 3), 8, 11)),
        ("f32_constant_16x16x1", np.full((1, 16, 16, 1), 3.25, dtype=f32), normal_f32((9, 9, 1), 9)),
        ("f32_zeros_8x8x1", np.where(np.arange(64).reshape(1, 8, 8, 1) % 3 == 0, f32(-0.0), np.where(
            np.arange(64).reshape(1, 8, 8, 1) % 3 == 1, f32(0.0), f32(1.5))).astype(f32), normal_f32((7, 5, 1), 10)),
        ("f32_tiny_1x1x1", np.full((1, 1, 1, 1), -2.0, dtype=f32), normal_f32((3, 4, 1), 11)),
        ("f32_tiny_5x3x1", normal_f32((2, 5, 3, 1), 12), normal_f32((1, 1, 1), 13)),
        ("f32_ragged_63x65x1", normal_f32((1, 63, 65, 1), 14), levels_f32((20, 20, 1), 15, 5)),
        ("u8_random_64x64x3", random_u8((2, 64, 64, 3), 16), smooth_u8((1, 48, 80, 3), 17)[0]),
        ("u8_smooth_33x47x1", smooth_u8((1, 33, 47, 1), 18), random_u8((50, 20, 1), 19, 30, 200)),
        ("u8_constant_16x16x3", np.full((1, 16, 16, 3), 77, dtype=np.uint8), random_u8((12, 12, 3), 20)),
    ]


def build():
    """the fixture's arrays: per case ``<i>_name``, ``<i>_images``, ``<i>_reference``, ``<i>_expected``"""
    g = {}
    for i, (name, images, reference) in enumerate(case_inputs()):
        k = "%02d_" % i
        g[k + "name"] = np.array(name)
        g[k + "images"] = images
        g[k + "reference"] = reference
        g[k + "expected"] = match_unique(images, reference)
    return g


def load_cases(g):
    """the cases of a loaded fixture: dicts with ``name``, ``images`` [B,H,W,C], ``reference`` [Ht,Wt,C], ``expected``"""
    return [dict(name=str(g[k + "name"]), images=g[k + "images"], reference=g[k + "reference"], expected=g[k + "expected"])
            for k in sorted(f[:-4] for f in g.files if f.endswith("_name"))]


def bit_equal(a, b):
    """same dtype, shape and values; zeros of either sign are one value (np.unique compares them equal)"""
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(a, b))


def check_restatement(cases=None):
    """both restatements on every case, in float64 and after the cast; returns the number of values compared"""
    total = 0
    for name, images, reference in (case_inputs() if cases is None else cases):
        a64, b64 = match_unique64(images, reference), match_sorted64(images, reference)
        assert bit_equal(a64, b64), name
        assert bit_equal(cast(a64, images.dtype), cast(b64, images.dtype)), name
        total += a64.size
    return total


def check_file():
    g = np.load(OUT)
    new = build()
    assert sorted(g.files) == sorted(new), "the fixture's array names differ"
    for k in new:
        a, b = np.asarray(new[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    return len(new)


if __name__ == "__main__":
    print("restatements agree on %d values" % check_restatement())
    if "--check" in sys.argv[1:]:
        print("%s: %d arrays regenerate exactly" % (OUT, check_file()))
    else:
        g = build()
        np.savez_compressed(OUT, **g)
        print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays")
