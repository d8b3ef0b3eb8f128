"""Generator of tests/golden/augment.npz: the expected values of the device-side light augmentation
(pointcloududa_amd/utils/augment.py, csrc/augment.hip).

The convention is restated here in numpy + scipy, independently of the package: the matrix is composed from the documented
formula, every channel is warped with ``scipy.ndimage.affine_transform(..., order, mode="grid-constant", cval)`` on float64
and rounded with ``floor(v + 0.5)``; masks take order 0 and fill 0; the fp32 rescales are written exactly as the
reference's lines (data_generator_mmwhs.py:246-254, data_generator_mscmrseg.py:310).  ``warp_np`` is a plain-numpy
bilinear / nearest restatement (no scipy) that pins the scipy one (``check_restatement``).

Inputs are rebuilt from seeds on both sides (``case_inputs``: smooth fields and nested ellipses,
``oracle.synth.synth_batch`` masks for the 256x256 cases); the fixture stores the parameters, the helper's own inverse
matrices, the expected uint8 warp, the expected masks, fp32 outputs of both rescale paths for some cases, the vertices of
the full-size warped mask, and per case the list of EXCUSABLE pixels: pixels where the pre-rounding value lies within 1e-9
of a rounding boundary (order 1) or a source coordinate lies within 1e-9 of a half-integer (order 0, masks).  The builder
asserts that they are at most 1e-5 of all pixels (they are expected to be none).

    python scripts/make_augment_golden.py        # writes tests/golden/augment.npz

scipy is imported inside the functions that need it: the GPU tests import this module for ``case_inputs`` only."""
from __future__ import annotations

import functools
import itertools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "augment.npz")
EPS = 1e-9                      # half-width of the excusable band around a rounding boundary
EXCUSED_CAP = 1e-5              # of all pixels of the case set
PARAM_KEYS = ("flip_lr", "flip_ud", "affine_on", "scale_x", "scale_y", "translate_x", "translate_y", "rotate", "shear", "order",
              "cval")
P = {"mmwhs_light": (0.2, 0.2, 0.3), "mscmrseg_simple": (0.3, 0.3, 0.45)}


# ------------------------------------------------------------------------------------------------ inputs
def smooth_images(b, h, w, c, seed):
    """float32 [B,H,W,C]: a few low-frequency waves and one soft ellipse per channel, roughly in [-2, 3]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((b, h, w, c), dtype=np.float64)
    for i in range(b):
        for ch in range(c):
            f = np.zeros((h, w))
            for _ in range(3):
                fy, fx = rng.uniform(0.5, 3.0, 2) * rng.choice([-1.0, 1.0], 2)
                f += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fy * yy / h + fx * xx / w) + rng.uniform(0, 2 * np.pi))
            cy, cx = h * rng.uniform(0.3, 0.7), w * rng.uniform(0.3, 0.7)
            f += 1.5 * np.exp(-(((yy - cy) / (0.2 * h)) ** 2 + ((xx - cx) / (0.15 * w)) ** 2))
            out[i, :, :, ch] = f
    return out.astype(np.float32)


def ellipse_labels(b, h, w, k, seed):
    """integer labels [B,H,W]: label j = the j-th of k-1 nested ellipses (oracle.synth.synth_labels for any h x w)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    lab = np.zeros((b, h, w), dtype=np.int64)
    for i in range(b):
        cy, cx = h * (0.5 + 0.08 * (rng.random() - 0.5)), w * (0.5 + 0.08 * (rng.random() - 0.5))
        for j in range(1, k):
            ry, rx = h * 0.36 * (k - j) / (k - 1), w * 0.28 * (k - j) / (k - 1)
            lab[i][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = j
    return lab


def quantise(x):
    """data_generator_mmwhs.py:246-249 in fp32 -> (uint8 images, min, max)"""
    x = np.asarray(x, dtype=np.float32)
    mn, mx = x.min(), x.max()
    q = (x - mn) * np.float32(255.) / (mx - mn)
    return np.array(q, dtype=np.uint8), mn, mx


def dequantise(q, mn, mx):
    """data_generator_mmwhs.py:254"""
    return mn + q.astype(np.float32) * (mx - mn) / np.float32(255.)


def div255(q):
    """data_generator_mscmrseg.py:310"""
    return np.array(q, np.float32) / np.float32(255.)


# ------------------------------------------------------------------------------------------------ parameters, cases
def draw(b, preset, rng, force_affine=False):
    p_lr, p_ud, p_aff = P[preset]
    d = dict(flip_lr=rng.random(b) < p_lr, flip_ud=rng.random(b) < p_ud, affine_on=rng.random(b) < p_aff,
             scale_x=rng.uniform(0.8, 1.2, b), scale_y=rng.uniform(0.8, 1.2, b), translate_x=rng.uniform(-0.1, 0.05, b),
             translate_y=rng.uniform(-0.1, 0.1, b), rotate=rng.uniform(-10, 10, b), shear=rng.uniform(-12, 12, b),
             order=rng.integers(0, 2, b), cval=rng.integers(0, 256, b))
    if force_affine:
        d["affine_on"][:] = True
    return d


def explicit(b, **kw):
    d = dict(flip_lr=np.zeros(b, bool), flip_ud=np.zeros(b, bool), affine_on=np.ones(b, bool), scale_x=np.ones(b),
             scale_y=np.ones(b), translate_x=np.zeros(b), translate_y=np.zeros(b), rotate=np.zeros(b), shear=np.zeros(b),
             order=np.zeros(b, np.int64), cval=np.zeros(b, np.int64))
    for k, v in kw.items():
        d[k] = np.asarray(v, dtype=d[k].dtype)
        assert d[k].shape == (b,), k
    return d


def cases():
    """list of dicts: name, b, h, w, c, k, seed, synth (masks from oracle.synth.synth_batch), params, op_order, f32 (store
    the fp32 outputs of both rescale paths), verts (store the vertices of the full-size warped mask)"""
    cs = []
    rng = np.random.default_rng(20260)
    # 256 x 256, light ranges of both presets, every sample warped, orders 0 and 1, C = 3 and 1, oracle.synth masks
    p = draw(2, "mmwhs_light", rng, force_affine=True)
    p["order"][:] = [0, 1]
    p["flip_lr"][:] = [True, False]
    cs.append(dict(name="light256_c3", b=2, h=256, w=256, c=3, k=5, seed=101, synth=True, params=p, op_order=(0, 1, 2),
                   f32=False, verts=True))
    p = draw(2, "mscmrseg_simple", rng, force_affine=True)
    p["order"][:] = [1, 0]
    p["flip_ud"][:] = [False, True]
    cs.append(dict(name="simple256_c1", b=2, h=256, w=256, c=1, k=4, seed=102, synth=True, params=p, op_order=(2, 0, 1),
                   f32=False, verts=True))
    # one non-square odd size with the corners of the heavy ranges
    cs.append(dict(name="heavy_200x231", b=3, h=200, w=231, c=1, k=5, seed=103, synth=False, op_order=(1, 2, 0), f32=False,
                   verts=False,
                   params=explicit(3, rotate=[45, -45, 45], translate_x=[0.2, -0.2, -0.2], translate_y=[-0.2, 0.2, 0.2],
                                   scale_x=[0.8, 1.2, 1.2], scale_y=[1.2, 0.8, 1.2], shear=[16, -16, 0], order=[1, 0, 1],
                                   cval=[255, 7, 128], flip_lr=[True, False, True], flip_ud=[False, True, True])))
    # all six operation orders, B = 5, parameters from both presets (flips and affine as the presets draw them, but at
    # least two samples warped), C alternating
    for i, oo in enumerate(itertools.permutations((0, 1, 2))):
        preset = ("mmwhs_light", "mscmrseg_simple")[i % 2]
        p = draw(5, preset, rng)
        p["affine_on"][[0, 3]] = True
        p["flip_lr"][1] = True
        p["flip_ud"][3] = True
        p["order"][[0, 3]] = [i % 2, 1 - i % 2]
        cs.append(dict(name="ops_%d%d%d_%s" % (oo + (preset,)), b=5, h=96, w=80, c=3 if i == 0 else 1, k=5, seed=110 + i,
                       synth=False, params=p, op_order=oo, f32=i in (1, 3), verts=False))
    # a small C = 3 case for the fp32 rescale paths
    p = draw(2, "mmwhs_light", rng, force_affine=True)
    p["order"][:] = [1, 0]
    cs.append(dict(name="rescale_c3", b=2, h=48, w=40, c=3, k=5, seed=119, synth=False, params=p, op_order=(1, 0, 2), f32=True,
                   verts=False))
    # heavy corners on the small size, B = 5
    cs.append(dict(name="heavy_96x80", b=5, h=96, w=80, c=1, k=5, seed=120, synth=False, op_order=(0, 1, 2), f32=True, verts=False,
                   params=explicit(5, rotate=[45, -45, 45, -45, 0], translate_x=[0.2, 0.2, -0.2, -0.2, 0.0],
                                   translate_y=[0.2, -0.2, 0.2, -0.2, 0.0], scale_x=[0.8, 1.2, 0.8, 1.2, 1.0],
                                   scale_y=[0.8, 0.8, 1.2, 1.2, 1.0], shear=[0, 12, -12, 16, -16], order=[1, 1, 0, 0, 1],
                                   cval=[0, 255, 100, 31, 200])))
    # translated almost out of the frame: <= 50 foreground pixels stay, the sampler gives zeros
    # (the third sample stays in view)
    cs.append(dict(name="out_of_frame", b=3, h=256, w=256, c=1, k=4, seed=121, synth=True, op_order=(0, 1, 2), f32=False, verts=True,
                   params=explicit(3, translate_x=[0.8, -0.743, 0.3], translate_y=[0.05, -0.1, 0.0], rotate=[5, -3, 8],
                                   order=[1, 0, 1], cval=[9, 250, 77])))
    return cs


def case_inputs(case):
    """(fp32 images [B,H,W,C], uint8 images = their min-max quantisation, min, max, integer labels [B,H,W]) of a case,
    rebuilt from its seed (numpy only)"""
    b, h, w, c, k, seed = (int(case[n]) for n in ("b", "h", "w", "c", "k", "seed"))
    x = smooth_images(b, h, w, c, seed)
    if case["synth"]:
        from oracle.synth import synth_batch
        assert h == w
        lab = np.argmax(synth_batch(b, 1, k, h, seed=seed)[1], axis=1).astype(np.int64)
    else:
        lab = ellipse_labels(b, h, w, k, seed + 1000)
    q, mn, mx = quantise(x)
    return x, q, mn, mx, lab


# ------------------------------------------------------------------------------------------------ the convention
def _t(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype=np.float64)


def compose_inverse(params, op_order, h, w):
    """float64 [B,2,3]: output pixel (x, y) -> source coordinate.  centre c = ((W-1)/2, (H-1)/2);
    A = T(c + (tx W, ty H)) . R(rotate) . Sh(shear) . S(sx, sy) . T(-c); flips x -> W-1-x, y -> H-1-y; the maps are
    multiplied in application order and the product is inverted"""
    b = len(params["flip_lr"])
    out = np.empty((b, 2, 3))
    c = np.array([(w - 1) / 2, (h - 1) / 2])
    for i in range(b):
        maps = []
        for op in op_order:
            if op == 0 and params["flip_lr"][i]:
                maps.append(np.array([[-1, 0, w - 1], [0, 1, 0], [0, 0, 1]], dtype=np.float64))
            if op == 1 and params["flip_ud"][i]:
                maps.append(np.array([[1, 0, 0], [0, -1, h - 1], [0, 0, 1]], dtype=np.float64))
            if op == 2 and params["affine_on"][i]:
                th, sh = math.radians(params["rotate"][i]), math.radians(params["shear"][i])
                rot = np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]])
                shm = np.array([[1, math.tan(sh), 0], [0, 1, 0], [0, 0, 1]])
                scm = np.array([[params["scale_x"][i], 0, 0], [0, params["scale_y"][i], 0], [0, 0, 1]])
                maps.append(_t(c[0] + params["translate_x"][i] * w, c[1] + params["translate_y"][i] * h) @ rot @ shm @ scm
                            @ _t(-c[0], -c[1]))
        fwd = functools.reduce(lambda acc, m: m @ acc, maps, np.eye(3))      # first applied = rightmost
        out[i] = np.linalg.inv(fwd)[:2]
    return out


def effective(params):
    """order / cval only act where the affine is on (a flip alone maps integer pixels to integer pixels)"""
    on = np.asarray(params["affine_on"], bool)
    return np.where(on, params["order"], 0).astype(np.int64), np.where(on, params["cval"], 0).astype(np.int64)


def source_coords(inv, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return inv[0, 0] * xx + inv[0, 1] * yy + inv[0, 2], inv[1, 0] * xx + inv[1, 1] * yy + inv[1, 2]


def warp_np(img, inv, order, cval):
    """plain-numpy restatement: float64 [H,W] -> the pre-rounding float64 [H,W]"""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape
    sx, sy = source_coords(inv, h, w)

    def tex(yi, xi):
        ok = (yi >= 0) & (yi < h) & (xi >= 0) & (xi < w)
        return np.where(ok, img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], float(cval))
    if order == 0:
        return tex(np.floor(sy + 0.5).astype(np.int64), np.floor(sx + 0.5).astype(np.int64))
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    return (tex(y0, x0) * (1 - fy) * (1 - fx) + tex(y0, x0 + 1) * (1 - fy) * fx + tex(y0 + 1, x0) * fy * (1 - fx)
            + tex(y0 + 1, x0 + 1) * fy * fx)


def warp_scipy(img, inv, order, cval):
    """the same through scipy.ndimage.affine_transform (array axes are (y, x): the matrix is transposed accordingly)"""
    from scipy.ndimage import affine_transform
    m = np.array([[inv[1, 1], inv[1, 0]], [inv[0, 1], inv[0, 0]]])
    return affine_transform(np.asarray(img, dtype=np.float64), m, offset=[inv[1, 2], inv[0, 2]], output=np.float64,
                            order=int(order), mode="grid-constant", cval=float(cval), prefilter=False)


def to_u8(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def near_half_coord(inv, h, w):
    """bool [H,W]: a source coordinate within EPS of a half-integer (where order 0 may pick the neighbour)"""
    sx, sy = source_coords(inv, h, w)
    d = lambda s: np.abs((s + 0.5) - np.round(s + 0.5))
    return (d(sx) <= EPS) | (d(sy) <= EPS)


def near_half_value(v):
    """bool: a pre-rounding value within EPS of k + 1/2"""
    return np.abs((v + 0.5) - np.round(v + 0.5)) <= EPS


def expected(case, warp=None):
    """-> dict: inv [B,2,3], u8 [B,H,W,C], mask uint8 [B,H,W], exc_img int32 [n,4] (b, y, x, c), exc_mask int32 [n,3]"""
    warp = warp or warp_scipy
    x, q, mn, mx, lab = case_inputs(case)
    b, h, w, c = q.shape
    inv = compose_inverse(case["params"], case["op_order"], h, w)
    order, cval = effective(case["params"])
    u8, mask = np.empty_like(q), np.empty((b, h, w), dtype=np.uint8)
    exc_img, exc_mask = [], []
    for i in range(b):
        coord = near_half_coord(inv[i], h, w)
        for ch in range(c):
            v = warp(q[i, :, :, ch], inv[i], order[i], cval[i])
            u8[i, :, :, ch] = to_u8(v)
            e = coord if order[i] == 0 else near_half_value(v)
            exc_img += [(i, yy, xx, ch) for yy, xx in zip(*np.nonzero(e))]
        mask[i] = to_u8(warp(lab[i], inv[i], 0, 0))
        exc_mask += [(i, yy, xx) for yy, xx in zip(*np.nonzero(coord))]
    return dict(inv=inv, u8=u8, mask=mask, exc_img=np.array(exc_img, dtype=np.int32).reshape(-1, 4),
                exc_mask=np.array(exc_mask, dtype=np.int32).reshape(-1, 3))


def check_restatement(case_list=None):
    """scipy against plain numpy on every case: pre-rounding values within 1e-9, rounded values equal except at excusable
    pixels, which may differ by one grey level (order 1) -- and excusable pixels at most EXCUSED_CAP of all pixels.
    -> (pixels, excused, largest pre-rounding difference)"""
    tot = exc = 0
    worst = 0.0
    for case in case_list or cases():
        _, q, _, _, lab = case_inputs(case)
        b, h, w, c = q.shape
        inv = compose_inverse(case["params"], case["op_order"], h, w)
        order, cval = effective(case["params"])
        for i in range(b):
            coord = near_half_coord(inv[i], h, w)
            for ch in range(c + 1):
                src, o, cv = (q[i, :, :, ch], order[i], cval[i]) if ch < c else (lab[i], 0, 0)
                a, n = warp_scipy(src, inv[i], o, cv), warp_np(src, inv[i], o, cv)
                e = coord if o == 0 else near_half_value(a) | near_half_value(n)
                tot += a.size
                exc += int(e.sum())
                if o == 1:
                    worst = max(worst, float(np.abs(a - n).max()))
                    assert np.abs(a - n).max() <= EPS, (case["name"], i, ch, np.abs(a - n).max())
                ra, rn = to_u8(a).astype(int), to_u8(n).astype(int)
                assert np.array_equal(ra[~e], rn[~e]), (case["name"], i, ch)
                assert np.abs(ra - rn).max() <= (1 if o == 1 else 255), (case["name"], i, ch)
    assert exc <= EXCUSED_CAP * tot, (exc, tot)
    return tot, exc, worst


def planar(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, 1))


def build():
    from oracle.sampler import mask_to_pointcloud
    g = {}
    tot = exc = 0
    for n, case in enumerate(cases()):
        e = expected(case)
        _, q, mn, mx, _ = case_inputs(case)
        k = "c%02d_" % n
        g[k + "name"] = np.array(case["name"])
        g[k + "dims"] = np.array([case[s] for s in ("b", "h", "w", "c", "k", "seed")], dtype=np.int64)
        g[k + "synth"] = np.array(bool(case["synth"]))
        g[k + "op_order"] = np.array(case["op_order"], dtype=np.int64)
        for p in PARAM_KEYS:
            g[k + p] = np.asarray(case["params"][p])
        for s in ("inv", "mask", "exc_img", "exc_mask"):
            g[k + s] = e[s]
        g[k + "u8"] = planar(e["u8"])      # images are stored [B,C,H,W]: the planes compress better than interleaved channels
        if case["f32"]:
            g[k + "minmax"] = np.array([mn, mx], dtype=np.float32)
            g[k + "minmax_f32"] = planar(dequantise(e["u8"], mn, mx))
            g[k + "div255_f32"] = planar(div255(e["u8"]))
        if case["verts"]:
            assert len(e["exc_mask"]) == 0, "pick another seed: the vertices need a mask without excusable pixels"
            g[k + "verts"] = np.stack([mask_to_pointcloud(e["mask"][i], first=0) for i in range(len(e["mask"]))]).astype(np.int32)
            g[k + "area"] = (e["mask"] > 0).reshape(len(e["mask"]), -1).sum(1).astype(np.int64)
            if case["name"] == "out_of_frame":
                assert np.all((g[k + "area"][:2] > 0) & (g[k + "area"][:2] <= 50)) and g[k + "area"][2] > 50, g[k + "area"]
        tot += e["u8"].size + e["mask"].size
        exc += len(e["exc_img"]) + len(e["exc_mask"])
    assert exc <= EXCUSED_CAP * tot, (exc, tot)
    return g


def load_cases(g):
    """the cases of a loaded fixture (what the tests iterate over): dicts as ``cases()`` gives them plus the expected arrays (images
    [B,H,W,C] again)"""
    out = []
    for k in sorted(f[:-4] for f in g.files if f.endswith("_name")):
        b, h, w, c, kk, seed = (int(v) for v in g[k + "dims"])
        case = dict(name=str(g[k + "name"]), b=b, h=h, w=w, c=c, k=kk, seed=seed, synth=bool(g[k + "synth"]),
                    op_order=tuple(int(v) for v in g[k + "op_order"]), params={p: g[k + p] for p in PARAM_KEYS})
        for s in ("inv", "u8", "mask", "exc_img", "exc_mask", "minmax", "minmax_f32", "div255_f32", "verts", "area"):
            if k + s in g.files:
                case[s] = g[k + s]
        for s in ("u8", "minmax_f32", "div255_f32"):      # back to [B,H,W,C]
            if s in case:
                case[s] = np.ascontiguousarray(np.moveaxis(case[s], 1, -1))
        out.append(case)
    return out


if __name__ == "__main__":
    print("restatement: %d pixels, %d excusable, largest pre-rounding difference %.3g" % check_restatement())
    g = build()
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays")
