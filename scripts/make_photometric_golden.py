"""Generator of tests/golden/photometric.npz: the expected values of the device-side photometric augmentation
(pointcloududa_amd/utils/photometric.py, csrc/photometric.hip).

The convention is restated here twice, independently of the package, as interpreters of a program's arrays
(``opcode [B,S]``, ``iarg [B,S,4]``, ``farg [B,S,16]``, ``seed [B,S]`` as ``PhotoProgram`` holds them):

* ``backend="scipy"``: ``scipy.ndimage.gaussian_filter(float64, (sigma, sigma, 0), mode="mirror")``,
  ``median_filter(size=(k, k, 1), mode="nearest")``, ``correlate(.., mode="mirror")`` for the average and the 3x3 kernels
* ``backend="numpy"``: ``np.pad`` + explicit sums in the documented order, ``sliding_window_view`` + sort for the median

and both share the plain-numpy Philox4x32-10 / Box-Muller of this file (``philox4x32_10``; the test suite checks it against
a scalar implementation of its own).  The numpy backend needs no scipy: the GPU tests use it at the production size.

Inputs are rebuilt from seeds on both sides (``case_inputs``: random uint8, f6's smooth fields quantised to uint8, and a
grey smooth image replicated to three channels, which is what MS-CMRSeg PNGs are).  The fixture stores the programs, the
expected uint8 images and per case the EXCUSABLE pixels: where a float64 operator's pre-rounding value lies within 1e-9
of a rounding boundary the pixel may differ by one grey level, and in a chain every pixel whose dependency window holds
such a pixel is excusable too.  The builder asserts that they are at most 1e-5 of all pixels and that the chains have
none.  The integer operators (average, median, dropouts, invert, add) have no band.

    python scripts/make_photometric_golden.py        # writes tests/golden/photometric.npz
    python scripts/make_photometric_golden.py --edges    # writes tests/golden/photometric_edges.json (see edges)"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from make_augment_golden import quantise, smooth_images  # noqa: E402  (f6's smooth fields; numpy only)

OUT = os.path.join(ROOT, "tests", "golden", "photometric.npz")
EPS = 1e-9                      # half-width of the excusable band around a rounding boundary
EXCUSED_CAP = 1e-5              # of all pixels of the case set
(NOP, GAUSSIAN_BLUR, AVERAGE_BLUR, MEDIAN_BLUR, CONV3X3, GAUSSIAN_NOISE, DROPOUT, COARSE_DROPOUT, INVERT, ADD, MULTIPLY,
 GRAYSCALE) = range(12)
NAMES = ("nop", "gaussian_blur", "average_blur", "median_blur", "conv3x3", "gaussian_noise", "dropout", "coarse_dropout",
         "invert", "add", "multiply", "grayscale")
INTEGER_OPS = (NOP, AVERAGE_BLUR, MEDIAN_BLUR, DROPOUT, COARSE_DROPOUT, INVERT, ADD)
SLOTS, IARGS, FARGS = 5, 4, 16
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ random numbers
def philox4x32_10(key, counter):
    """Philox4x32-10 as implemented here: key = a 64-bit integer (low word k0, high word k1), counter = (c, 0, 0, 0) for
    every c of the uint32 array ``counter``; ten rounds
    ``(c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))`` with M0 = 0xD2511F53,
    M1 = 0xCD9E8D57, the key bumped by (0x9E3779B9, 0xBB67AE85) between rounds -> four uint32 arrays"""
    k0, k1 = np.uint64(int(key) & 0xFFFFFFFF), np.uint64(int(key) >> 32)
    c0 = np.asarray(counter).astype(np.uint64)
    c1, c2, c3 = np.zeros_like(c0), np.zeros_like(c0), np.zeros_like(c0)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def normal_draws(key, counter):
    """Box-Muller in float64 from the first two words: u = (x + 0.5) 2^-32, z = sqrt(-2 log u1) cos(2 pi u2)"""
    x0, x1, _, _ = philox4x32_10(key, counter)
    u1, u2 = (x0.astype(np.float64) + 0.5) * 2.0 ** -32, (x1.astype(np.float64) + 0.5) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def element_index(h, w, c, per_channel):
    """uint32 [H,W,C]: the element's index inside its sample; the pixel index (shared by the channels) when not per_channel"""
    pix = np.arange(h * w, dtype=np.int64).reshape(h, w, 1)
    return (pix * c + np.arange(c)).astype(np.uint32) if per_channel else np.broadcast_to(pix, (h, w, c)).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ operators
def gaussian_weights(sigma):
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return (phi / phi.sum())[r:]


def _symmetric_pass(x, wts, axis):
    """t = x[0] w[0]; for d = r..1: t += (x[-d] + x[+d]) w[d], reflect-101 border"""
    r = len(wts) - 1
    pad = [(0, 0)] * x.ndim
    pad[axis] = (r, r)
    p = np.pad(x, pad, mode="reflect")
    n = x.shape[axis]
    sl = lambda o: tuple(slice(r + o, r + o + n) if a == axis else slice(None) for a in range(x.ndim))
    t = p[sl(0)] * wts[0]
    for d in range(r, 0, -1):
        t = t + (p[sl(-d)] + p[sl(d)]) * wts[d]
    return t


def _shifted(p, dy, dx, h, w, r):
    return p[r + dy:r + dy + h, r + dx:r + dx + w]


def op_values(img, op, ia, fa, seed, backend):
    """one slot on one uint8 sample [H,W,C] -> (float64 pre-rounding values or an integer array, halo of the operator,
    mixes channels).  Integer results are exact."""
    h, w, c = img.shape
    x = img.astype(np.float64)
    if op == GAUSSIAN_BLUR:
        r = int(ia[0])
        if backend == "scipy":
            from scipy.ndimage import gaussian_filter
            sigma = float(fa[15])
            assert int(4.0 * sigma + 0.5) == r
            return gaussian_filter(x, (sigma, sigma, 0), mode="mirror"), r, False
        wts = np.asarray(fa[:r + 1], dtype=np.float64)
        return _symmetric_pass(_symmetric_pass(x, wts, 0), wts, 1), r, False
    if op == AVERAGE_BLUR:
        k = int(ia[0])
        lo, hi = -(k // 2), k - k // 2 - 1
        if backend == "scipy":
            from scipy.ndimage import correlate
            s = correlate(img.astype(np.int64), np.ones((k, k, 1), dtype=np.int64), mode="mirror")
        else:
            r = k // 2
            p = np.pad(img.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="reflect")
            s = np.zeros((h, w, c), dtype=np.int64)
            for dy in range(lo, hi + 1):
                for dx in range(lo, hi + 1):
                    s += _shifted(p, dy, dx, h, w, r)
        return (2 * s + k * k) // (2 * k * k), k // 2, False
    if op == MEDIAN_BLUR:
        k = int(ia[0])
        if backend == "scipy":
            from scipy.ndimage import median_filter
            return median_filter(img, size=(k, k, 1), mode="nearest").astype(np.int64), k // 2, False
        r = k // 2
        p = np.pad(img, ((r, r), (r, r), (0, 0)), mode="edge")
        win = np.lib.stride_tricks.sliding_window_view(p, (k, k), axis=(0, 1)).reshape(h, w, c, k * k)
        return np.sort(win, axis=-1)[..., (k * k - 1) // 2].astype(np.int64), r, False
    if op == CONV3X3:
        wts = np.asarray(fa[:9], dtype=np.float64)
        if backend == "scipy":
            from scipy.ndimage import correlate
            return correlate(x, wts.reshape(3, 3, 1), mode="mirror"), 1, False
        p = np.pad(x, ((1, 1), (1, 1), (0, 0)), mode="reflect")
        t = np.zeros((h, w, c), dtype=np.float64)
        for i in range(9):
            t = t + _shifted(p, i // 3 - 1, i % 3 - 1, h, w, 1) * wts[i]
        return t, 1, False
    if op == GAUSSIAN_NOISE:
        z = normal_draws(seed, element_index(h, w, c, bool(ia[0])))
        return x + float(fa[0]) * z, 0, False
    if op == DROPOUT:
        thr = min(int(np.floor(float(fa[0]) * 2.0 ** 32)), 2 ** 32 - 1)
        x0 = philox4x32_10(seed, element_index(h, w, c, bool(ia[0])))[0]
        return np.where(x0 < np.uint32(thr), 0, img).astype(np.int64), 0, False
    if op == COARSE_DROPOUT:
        thr = min(int(np.floor(float(fa[0]) * 2.0 ** 32)), 2 ** 32 - 1)
        gh, gw = max(1, int(np.floor(h * float(fa[1]) + 0.5))), max(1, int(np.floor(w * float(fa[1]) + 0.5)))
        x0 = philox4x32_10(seed, element_index(gh, gw, c, bool(ia[0])))[0]
        cy, cx = (np.arange(h) * gh) // h, (np.arange(w) * gw) // w
        return np.where(x0[cy][:, cx] < np.uint32(thr), 0, img).astype(np.int64), 0, False
    if op == INVERT:
        on = np.array([(int(ia[0]) >> ch) & 1 for ch in range(c)], dtype=bool)
        return np.where(on, 255 - img.astype(np.int64), img.astype(np.int64)), 0, False
    if op == ADD:
        return np.clip(img.astype(np.int64) + np.asarray(ia[:c], dtype=np.int64), 0, 255), 0, False
    if op == MULTIPLY:
        return x * np.asarray(fa[:c], dtype=np.float64), 0, False
    if op == GRAYSCALE:
        if c == 1:
            return img.astype(np.int64), 0, False
        assert c == 3, "GRAYSCALE takes 3 channels"
        g = 0.299 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]
        a = float(fa[0])
        return (1.0 - a) * x + a * g[..., None], 0, True
    assert op == NOP, op
    return img.astype(np.int64), 0, False


def to_u8(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def near_boundary(v):
    """bool: a pre-rounding value within EPS of k + 1/2"""
    return np.abs((v + 0.5) - np.round(v + 0.5)) <= EPS


def dilate(exc, r, across_channels):
    """bool [H,W,C]: True where the (2r + 1)^2 window (and, for a channel-mixing operator, any channel) holds a True"""
    if not exc.any():
        return exc
    if across_channels:
        exc = np.broadcast_to(exc.any(-1, keepdims=True), exc.shape)
    if r == 0:
        return np.array(exc)
    h, w, _ = exc.shape
    p = np.pad(exc, ((r, r), (r, r), (0, 0)), mode="edge")
    out = np.zeros_like(exc)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out |= _shifted(p, dy, dx, h, w, r)
    return out


def run_program(images, opcode, iarg, farg, seed, backend="numpy"):
    """uint8 [B,H,W,C] + a program -> (uint8 [B,H,W,C], excusable bool [B,H,W,C]); uint8 again between two slots"""
    out = np.empty_like(images)
    exc = np.zeros(images.shape, dtype=bool)
    for i in range(images.shape[0]):
        cur, e = images[i], np.zeros(images.shape[1:], dtype=bool)
        for s in range(opcode.shape[1]):
            op = int(opcode[i, s])
            if op == NOP:
                continue
            v, halo, mixes = op_values(cur, op, iarg[i, s], farg[i, s], int(seed[i, s]), backend)
            e = dilate(e, halo, mixes)
            if v.dtype == np.float64:
                e = e | near_boundary(v)
                cur = to_u8(v)
            else:
                cur = v.astype(np.uint8)
        out[i], exc[i] = cur, e
    return out, exc


# ------------------------------------------------------------------------------------------------ programs, cases
class Prog:
    """the generator's own encoder of a program's arrays (the package's PhotoProgram.set_* are checked against it)"""

    def __init__(self, b, slots=SLOTS):
        self.opcode = np.zeros((b, slots), dtype=np.int32)
        self.iarg = np.zeros((b, slots, IARGS), dtype=np.int32)
        self.farg = np.zeros((b, slots, FARGS), dtype=np.float64)
        self.seed = np.zeros((b, slots), dtype=np.uint64)

    def put(self, i, s, op, **kw):
        self.opcode[i, s] = op
        ia, fa = self.iarg[i, s], self.farg[i, s]
        if op == GAUSSIAN_BLUR:
            wts = gaussian_weights(kw["sigma"])
            if len(wts) == 1:
                self.opcode[i, s] = NOP
            else:
                ia[0], fa[:len(wts)], fa[15] = len(wts) - 1, wts, kw["sigma"]
        elif op in (AVERAGE_BLUR, MEDIAN_BLUR):
            ia[0] = kw["k"]
        elif op == CONV3X3:
            fa[:9] = np.asarray(kw["weights"], dtype=np.float64).reshape(9)
        elif op == GAUSSIAN_NOISE:
            fa[0], ia[0], self.seed[i, s] = kw["scale"], int(kw["per_channel"]), kw["seed"]
        elif op == DROPOUT:
            fa[0], ia[0], self.seed[i, s] = kw["p"], int(kw["per_channel"]), kw["seed"]
        elif op == COARSE_DROPOUT:
            fa[0], fa[1], ia[0], self.seed[i, s] = kw["p"], kw["size_percent"], int(kw["per_channel"]), kw["seed"]
        elif op == INVERT:
            ia[0] = sum(1 << ch for ch, on in enumerate(kw["channels"]) if on)
        elif op == ADD:
            ia[:] = np.broadcast_to(kw["values"], (IARGS,))
        elif op == MULTIPLY:
            fa[:IARGS] = np.broadcast_to(kw["factors"], (IARGS,))
        elif op == GRAYSCALE:
            fa[0] = kw["alpha"]


def sharpen(alpha, lightness):
    ident = np.zeros((3, 3)); ident[1, 1] = 1.0
    m = -np.ones((3, 3)); m[1, 1] = 8.0 + lightness
    return (1.0 - alpha) * ident + alpha * m


def emboss(alpha, strength):
    ident = np.zeros((3, 3)); ident[1, 1] = 1.0
    s = strength
    m = np.array([[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]], dtype=np.float64)
    return (1.0 - alpha) * ident + alpha * m


def _near(rng, lo, hi, end):
    """a continuous parameter within 2 % of an end of its range (not the round value itself)"""
    t = rng.uniform(0.0, 0.02)
    return lo + t * (hi - lo) if end == 0 else hi - t * (hi - lo)


def corner_slots(op, rng):
    """the parameter corners of an opcode: a list of keyword dicts, one per sample"""
    sd = lambda: int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    u = lambda lo, hi: float(rng.uniform(lo, hi))
    if op == GAUSSIAN_BLUR:
        return [dict(sigma=3.0), dict(sigma=_near(rng, 0.125, 3.0, 0)), dict(sigma=u(0.5, 2.5))]
    if op == AVERAGE_BLUR:
        return [dict(k=2), dict(k=7), dict(k=4)]
    if op == MEDIAN_BLUR:
        return [dict(k=3), dict(k=11), dict(k=7)]
    if op == CONV3X3:
        return [dict(weights=sharpen(_near(rng, 0, 1, 1), _near(rng, 0.75, 1.5, 1))),
                dict(weights=sharpen(_near(rng, 0, 1, 0), _near(rng, 0.75, 1.5, 0))),
                dict(weights=emboss(_near(rng, 0, 1, 1), _near(rng, 0, 2, 1))),
                dict(weights=emboss(u(0.2, 0.8), _near(rng, 0, 2, 0)))]
    if op == GAUSSIAN_NOISE:
        return [dict(scale=_near(rng, 0, 12.75, 1), per_channel=True, seed=sd()),
                dict(scale=_near(rng, 0, 12.75, 1), per_channel=False, seed=sd()),
                dict(scale=_near(rng, 0, 12.75, 0), per_channel=True, seed=sd())]
    if op == DROPOUT:
        return [dict(p=_near(rng, 0.01, 0.1, 1), per_channel=True, seed=sd()),
                dict(p=_near(rng, 0.01, 0.1, 0), per_channel=False, seed=sd())]
    if op == COARSE_DROPOUT:
        return [dict(p=_near(rng, 0.03, 0.15, 1), size_percent=_near(rng, 0.02, 0.05, 1), per_channel=True, seed=sd()),
                dict(p=_near(rng, 0.03, 0.15, 0), size_percent=_near(rng, 0.02, 0.05, 0), per_channel=False, seed=sd()),
                dict(p=_near(rng, 0.03, 0.15, 1), size_percent=_near(rng, 0.02, 0.05, 1), per_channel=False, seed=sd())]
    if op == INVERT:
        return [dict(channels=(1, 0, 1, 0)), dict(channels=(1, 1, 1, 1)), dict(channels=(0, 0, 0, 0))]
    if op == ADD:
        return [dict(values=(-10, 10, 3, 0)), dict(values=10), dict(values=-10)]
    if op == MULTIPLY:
        return [dict(factors=(_near(rng, 0.5, 1.5, 0), _near(rng, 0.5, 1.5, 1), u(0.5, 1.5), 1.0)),
                dict(factors=_near(rng, 0.5, 1.5, 1)), dict(factors=_near(rng, 0.5, 1.5, 0))]
    assert op == GRAYSCALE
    return [dict(alpha=_near(rng, 0, 1, 0)), dict(alpha=_near(rng, 0, 1, 1)), dict(alpha=u(0.2, 0.8))]


def random_slot(op, rng):
    """one slot with continuous parameters drawn from the reference's ranges"""
    sd = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    u = lambda lo, hi: float(rng.uniform(lo, hi))
    pc = bool(rng.integers(0, 2))
    return {GAUSSIAN_BLUR: lambda: dict(sigma=u(0.2, 3.0)), AVERAGE_BLUR: lambda: dict(k=int(rng.integers(2, 8))),
            MEDIAN_BLUR: lambda: dict(k=2 * int(rng.integers(1, 6)) + 1),
            CONV3X3: lambda: dict(weights=sharpen(u(0, 1), u(0.75, 1.5)) if pc else emboss(u(0, 1), u(0, 2))),
            GAUSSIAN_NOISE: lambda: dict(scale=u(0, 12.75), per_channel=pc, seed=sd),
            DROPOUT: lambda: dict(p=u(0.01, 0.1), per_channel=pc, seed=sd),
            COARSE_DROPOUT: lambda: dict(p=u(0.03, 0.15), size_percent=u(0.02, 0.05), per_channel=pc, seed=sd),
            INVERT: lambda: dict(channels=tuple(int(v) for v in rng.integers(0, 2, 4))),
            ADD: lambda: dict(values=tuple(int(v) for v in rng.integers(-10, 11, 4)) if pc else int(rng.integers(-10, 11))),
            MULTIPLY: lambda: dict(factors=tuple(rng.uniform(0.5, 1.5, 4)) if pc else u(0.5, 1.5)),
            GRAYSCALE: lambda: dict(alpha=u(0, 1))}[op]()


KINDS = ("random", "smooth", "grey3")


def cases():
    """list of dicts: name, b, h, w, c, seed, kind, chain, program arrays"""
    cs = []
    rng = np.random.default_rng(20267)
    n = 0
    for op in range(GAUSSIAN_BLUR, GRAYSCALE + 1):
        for (h, w), c in (((64, 48), 1), ((64, 48), 3), ((96, 80), 1), ((96, 80), 3)):
            slots = corner_slots(op, rng)
            if (h, w) == (96, 80):                  # the two ends of the ranges only: the fixture stays under 1 MB
                slots = [slots[0], slots[2]] if op == CONV3X3 else slots[:2]
            kind = ("smooth", "random")[op % 2] if c == 1 else ("grey3", "smooth", "random")[(op + (h > 64)) % 3]
            if kind == "random" and (h, w) == (96, 80):
                kind = "smooth"
            prog = Prog(len(slots), 1)
            for i, kw in enumerate(slots):
                prog.put(i, 0, op, **kw)
            cs.append(dict(name="%s_%dx%d_c%d" % (NAMES[op], h, w, c), b=len(slots), h=h, w=w, c=c, seed=300 + n, kind=kind,
                           chain=False, prog=prog))
            n += 1
    # chains of five slots: every sample its own order; every operator occurs, per_channel on and off
    pool = list(range(GAUSSIAN_BLUR, GRAYSCALE + 1))
    for j, ((h, w), c, kind) in enumerate((((96, 80), 3, "grey3"), ((64, 48), 1, "smooth"), ((64, 48), 3, "random"))):
        b = 4
        prog = Prog(b, SLOTS)
        for i in range(b):
            ops = rng.permutation(pool)[:SLOTS] if (i + j) % 2 else np.roll(pool, -(3 * i + 5 * j))[:SLOTS]
            for s, op in enumerate(ops):
                prog.put(i, s, int(op), **random_slot(int(op), rng))
        cs.append(dict(name="chain%d_%dx%d_c%d" % (j, h, w, c), b=b, h=h, w=w, c=c, seed=400 + j, kind=kind, chain=True,
                       prog=prog))
    return cs


def make_images(kind, b, h, w, c, seed):
    """uint8 [B,H,W,C] of an input kind, from a seed (numpy only)"""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (b, h, w, c), dtype=np.uint8)
    if kind == "smooth":
        return quantise(smooth_images(b, h, w, c, seed))[0]
    assert kind == "grey3" and c == 3
    return np.ascontiguousarray(np.repeat(quantise(smooth_images(b, h, w, 1, seed))[0], 3, axis=-1))


def case_inputs(case):
    return make_images(case["kind"], *(int(case[k]) for k in ("b", "h", "w", "c", "seed")))


def _arrays(case):
    p = case["prog"]
    return p.opcode, p.iarg, p.farg, p.seed


def check_restatement(case_list=None):
    """scipy against plain numpy on every case: 0 rounded mismatches, excusable pixels at most EXCUSED_CAP of all pixels.
    -> (pixels, excused)"""
    tot = exc = 0
    for case in case_list or cases():
        x = case_inputs(case)
        a, ea = run_program(x, *_arrays(case), backend="scipy")
        n, en = run_program(x, *_arrays(case), backend="numpy")
        assert np.array_equal(a, n), (case["name"], int((a != n).sum()))
        tot += a.size
        exc += int((ea | en).sum())
    assert exc <= EXCUSED_CAP * tot, (exc, tot)
    return tot, exc


def planar(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, 1))


def build():
    g = {}
    tot = exc = 0
    for n, case in enumerate(cases()):
        out, e = run_program(case_inputs(case), *_arrays(case), backend="scipy")
        k = "c%02d_" % n
        g[k + "name"] = np.array(case["name"])
        g[k + "kind"] = np.array(case["kind"])
        g[k + "dims"] = np.array([case[s] for s in ("b", "h", "w", "c", "seed")], dtype=np.int64)
        g[k + "chain"] = np.array(bool(case["chain"]))
        g[k + "opcode"], g[k + "iarg"], g[k + "farg"], g[k + "seed"] = _arrays(case)
        g[k + "u8"] = planar(out)       # stored [B,C,H,W]: the planes compress better than interleaved channels
        g[k + "exc"] = np.argwhere(e).astype(np.int32).reshape(-1, 4)
        if case["chain"]:
            assert not e.any(), "pick another seed: the chains are meant to have no excusable pixel (%s)" % case["name"]
        if np.all(np.isin(case["prog"].opcode, INTEGER_OPS)):
            assert not e.any(), case["name"]
        tot += out.size
        exc += int(e.sum())
    assert exc <= EXCUSED_CAP * tot, (exc, tot)
    return g


def load_cases(g):
    """the cases of a loaded fixture: dicts with the program arrays, the expected images ([B,H,W,C] again) and ``exc``"""
    out = []
    for k in sorted(f[:-4] for f in g.files if f.endswith("_name")):
        b, h, w, c, seed = (int(v) for v in g[k + "dims"])
        case = dict(name=str(g[k + "name"]), kind=str(g[k + "kind"]), b=b, h=h, w=w, c=c, seed=seed, chain=bool(g[k + "chain"]),
                    opcode=g[k + "opcode"], iarg=g[k + "iarg"], farg=g[k + "farg"], seed_arr=g[k + "seed"], exc=g[k + "exc"],
                    u8=np.ascontiguousarray(np.moveaxis(g[k + "u8"], 1, -1)))
        out.append(case)
    return out


# ------------------------------------------------------------------------------------------------ the edge shapes
EDGES = os.path.join(ROOT, "tests", "golden", "photometric_edges.json")


def edges():
    """tests/photometric_edge_cases.py's table (more than one tile, C = 2 and 4, both store paths, images below the halo, 224 x 224 x 1):
    per case the shape, the batch and one sha256 of the expected batch.  Nothing is recorded unless the scipy backend equals the
    numpy backend on every case and no case has an excusable pixel in either: the table is band-free, and the GPU test
    demands equality"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("photometric_edge_cases", os.path.join(ROOT, "tests", "photometric_edge_cases.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    recorded = {}
    for cs in t.CASES:
        (a, ea), (n, en) = t.expected(cs, "scipy"), t.expected(cs, "numpy")
        if not np.array_equal(a, n):
            raise SystemExit("the scipy and the numpy backend differ on %s: %d elements" % (cs.name, int((a != n).sum())))
        if ea.any() or en.any():
            raise SystemExit("%s has %d excusable pixels: change its seed" % (cs.name, int((ea | en).sum())))
        recorded[cs.name] = t.digests_of(cs)
    return {"numpy_version": np.__version__, "cases": recorded}


if __name__ == "__main__":
    if "--edges" in sys.argv:
        import json
        data = edges()
        with open(EDGES, "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote %s: %d cases, %d bytes" % (EDGES, len(data["cases"]), os.path.getsize(EDGES)))
        sys.exit(0)
    print("restatement: %d pixels, %d excusable" % check_restatement())
    g = build()
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays")
