"""Device-side "stylize" augmentation for the loader path: the three entries of the reference's
``SomeOf`` lists that f7 and f8 left out -- ``Superpixels`` (``src/data_generator_mscmrseg.py:46`` / ``:98``),
``SimplexNoiseAlpha(EdgeDetect | DirectedEdgeDetect)`` (``:57-60`` / ``:108-111``) and ``AddToHueAndSaturation`` (``:69`` /
``:120``) -- as a per-sample PROGRAM that one HIP entry point (``csrc/stylize.hip``) runs over uint8 ``[B,H,W,C]`` images.  Masks
and stored vertices are untouched by all three.

A program has ``S`` slots per sample (``S <= 8``); slot ``s`` of sample ``i`` is ``opcode[i, s]`` with ``iarg[i, s, :12]`` (int32),
``farg[i, s, :16]`` (float64), ``table[i, s, :768]`` (float64: three coarse grids of up to 16 x 16 values) and ``seed[i, s]``
(uint64).  ``rdiv(a, b) = floor((2 a + b) / (2 b))``, a true floor.

==========================  ==================================================================================
``OP_NOP``                  copy
``OP_HUE_SATURATION``       C = 3, channel 0 = red; ``iarg[0]`` = dh (hue is 0..179), ``iarg[1]`` = ds; integers only:
                            ``V = max``, ``d = V - min``, ``S = rdiv(255 d, V)``, ``H = (base + rdiv(30 num, d)) mod 180`` with
                            (base, num) = (0, g - b) | (60, b - r) | (120, r - g) by the first of r, g, b that equals V; ``H' =
                            (H + dh) mod 180``, ``S' = clip(S + ds, 0, 255)``; back through ``p = rdiv(V (255 - S'), 255)``,
                            ``q = rdiv(V (7650 - S' F), 7650)``, ``t = rdiv(V (7650 - S' (30 - F)), 7650)``, ``F = H' % 30``, by
                            sector ``H' // 30``: (V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q)
``OP_NOISE_ALPHA_CONV3X3``  ``iarg[0]`` = n (1..3 grids), ``iarg[1]`` = upscale (``UPSCALE_NEAREST`` | ``UPSCALE_BILINEAR`` | ``UPSCALE_CUBIC``),
                            ``iarg[2]`` = aggregation (``AGG_MIN`` | ``AGG_MEAN`` | ``AGG_MAX``), ``iarg[3]`` = sigmoid on,
                            ``iarg[4 + 2 k : 6 + 2 k]`` = (h', w') of grid k (2..16 each), ``table[256 k + y w' + x]`` = its values
                            in [0, 1] (``simplex_grid``, evaluated HERE in float64, as f7 evaluates the Gaussian's weights),
                            ``farg[0..8]`` = 3x3 correlation weights (``edge_detect_weights``, ``directed_edge_weights``),
                            ``farg[9]`` = the sigmoid's threshold t.  Each grid is upscaled to H x W (nearest: cell
                            ``((y h') // H, (x w') // W)``; bilinear: source ``(y + 0.5) h' / H - 0.5`` clamped to
                            ``[0, h' - 1]``; cubic (``UPSCALE_CUBIC = 3``, f8b): the same source coordinate UNCLAMPED, the
                            Keys weights (A = -0.75) and summation order of ``utils/geometric.py``'s order 3 over the taps
                            ``floor(s) - 1 .. floor(s) + 2``, each tap index clamped into the grid, the upscaled value
                            clipped to [0, 1]), the n masks are aggregated (the mean sums in grid order), optionally
                            ``m = 1 / (1 + exp(-(20 (m - 0.5) - t)))``; ``e = to_u8(f7's CONV3X3)`` (reflect-101 border),
                            ``out = to_u8((1 - m) x + m e)``; float64 in this order, one m for all channels
``OP_SUPERPIXELS``          ``iarg[0:2]`` = (gy, gx), ``gy gx <= 256``; ``iarg[2]`` = updates (0..10), ``iarg[3]`` = M2 =
                            ``floor(compactness^2 + 0.5)``, ``farg[0]`` = p_replace (the kernel gets ``floor(p 2^32)`` in
                            ``iarg[4]``), ``farg[1]`` = compactness, ``seed``.  A grid SLIC in integers only: centre
                            ``k = j gx + i`` starts at ``(((2j+1) H) // (2 gy), ((2i+1) W) // (2 gx))`` with that pixel's colour; a pixel
                            takes, among the centres of the 3x3 grid cells around its own cell ``((y gy) // H, (x gx) // W)``
                            that exist, the smallest ``D = dc2 S2 + M2 ds2`` (``S2 = max(1, (H W) // (gy gx))``), ties to the
                            lowest k; update: centre = ``rdiv(sum, n)`` of colour, y and x, a centre without pixels stays; after
                            the updates and one last assignment, segment k takes its mean colour ``rdiv(sum, n)`` iff the first
                            word of f7's Philox4x32-10 (key = ``seed``, counter = k) is below the threshold, else it is copied
==========================  ==================================================================================

Connected superpixels (f9b, ``csrc/spx_connect.hip``, opt-in): ``iarg[5]`` = ``min_size`` of a SUPERPIXELS slot.  0 is the slot
above, bit for bit.  With ``min_size >= 1`` the 4-connected components of equal labels (label 0 is an ordinary label) get as id
the index ``r = y W + x`` of their raster-first pixel; a component is small iff its own pixel count is below ``min_size`` and
``r != 0``; a small component's target is the component of pixel ``r - 1`` if ``x > 0``, else of pixel ``r - W``; targets are
followed until a component that is not small, which gives every pixel its final id (merged pixels count towards nobody's
size).  A final segment is 4-connected; it takes ``rdiv(sum, n)`` over its pixels iff the first Philox word for counter = final
id is below the threshold.  ``superpixel_min_size(gy, gx, H, W) = max(1, (H W) // (2 gy gx))`` is skimage's
``min_size_factor = 0.5``; the presets ``"heavy_connected_device"`` and ``"mscmrseg_aug2_connected_device"`` are the ``_refpad_``
presets with it on every Superpixels slot.  ``stylize_aug`` takes the connected entry point iff ``program.needs_connect()``.
skimage is not installed next to the reference: parity with ``_enforce_label_connectivity_cython`` is unpinned, the rule is
this build's own (``tests/golden/spx_connect.npz``, ``scripts/make_spx_connect_golden.py``); skimage's ``max_size_factor`` split
and 8-connectivity are not built.

Superpixels at a working size (f9c, ``csrc/spx_scale.hip``, opt-in): ``iarg[6]`` = ``max_size`` = m of a SUPERPIXELS slot, the
counterpart of imgaug's ``max_size=128`` (``SUPERPIXELS_MAX_SIZE``).  The slot is *scaled* iff ``m >= 1`` and ``L = max(H, W) > m``;
otherwise (0 is what ``_clear`` leaves) it is the slot above, with or without ``min_size``, bit for bit.  A scaled slot works
on ``h' x w' = superpixel_working_size(H, W, m) = (max(1, (H m) // L), max(1, (W m) // L))`` (imgaug computes ``int(H * (m / L))``
in floating point; the integer form makes the longer side exactly m).  The linear resize ``R(src[Sh x Sw x C] -> Dh x Dw)``
is, per axis with source size S, destination size D and destination index d: ``a = clip((2 d + 1) S - D, 0, 2 D (S - 1))``
(the coordinate ``(d + 0.5) S / D - 0.5`` times ``2 D``, clamped into the image), ``i0 = a // (2 D)``, ``t = a - 2 D i0``, ``i1 =
min(i0 + 1, S - 1)``; ``num = (2 Dh - ty) ((2 Dw - tx) p00 + tx p01) + ty ((2 Dw - tx) p10 + tx p11)``, ``den = 4 Dh Dw``, value =
``floor((2 num + den) / (2 den))``: two taps per axis, half-pixel centres, round half up, 64-bit integers and no float (a
float64 restatement of the same formula differs by a grey level where rounding error decides a tie).  ``small = R(slot input
-> h' x w')``; the grid SLIC above runs on ``small`` with ``h', w'`` in place of ``H, W`` everywhere; ``min_size >= 1`` runs f9b's
rule on the working-size label plane (ids and Philox counters ``r = y w' + x``); the repaint with ``rdiv(sum, n)`` over the
pixels of ``small`` gives ``painted``; ``out = R(painted -> H x W)`` -- unless no final segment that holds a pixel is
replaced: then the sample's output is the slot's input bit for bit, not the blurred round trip (recalled as imgaug's own
shortcut, which cannot be checked here: this build's choice).  For a scaled slot ``validate`` and ``encode_style(..,
scaled=True)`` measure ``gy``, ``gx`` and ``min_size`` against the working size.  The presets ``"heavy_scaled_device"`` and
``"mscmrseg_aug2_scaled_device"`` are the ``_connected_`` presets with ``max_size = 128`` on every Superpixels slot.
``stylize_aug`` takes the scaled entry point iff ``program.needs_scale(H, W)``.  imgaug, cv2 and skimage are not installed
next to the reference: parity with their resize and with imgaug's shortcut is unpinned, the rule is this build's own
(``tests/golden/spx_scaled.npz``, ``scripts/make_spx_scaled_golden.py``).

The value is uint8 again between two slots.  imgaug / cv2 / skimage are not vendored by the reference: parity with imgaug is
unpinned, the convention is this build's own and is pinned by ``tests/golden/stylize.npz`` (``scripts/make_stylize_golden.py``:
a vectorised numpy restatement and an independent one -- plain Python integers for hue and superpixels, scipy for
noise-alpha).  Divergences from imgaug: hue / saturation follow the integer formulas above (cv2's uint8 HSV tables differ by
a grey level in places) and one value moves both (``per_channel`` is not built); the simplex noise is this file's (gradient
from Philox, grids of at most 16 x 16; the cubic upscale is the Keys kernel in float64, not cv2's fixed-point tables, and the
samplers draw it only with ``interp="cubic"``, for a share of ``NOISE_CUBIC_P`` of the slots); the superpixels are a grid SLIC, at
full resolution unless ``max_size`` asks for imgaug's working size, and without a connectivity pass unless ``min_size`` asks
for one (above).  The string ``"heavy"`` keeps raising (imgaug's parameter
stream is not reproduced)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import kernels as K
from ._program import SlotProgram, upload

OP_NOP, OP_HUE_SATURATION, OP_NOISE_ALPHA_CONV3X3, OP_SUPERPIXELS = range(4)
OP_NAMES = ("NOP", "HUE_SATURATION", "NOISE_ALPHA_CONV3X3", "SUPERPIXELS")
MAX_SLOTS, IARGS, FARGS = 8, 12, 16
GRID_VALUES, MAX_GRIDS = 256, 3
TABLE = MAX_GRIDS * GRID_VALUES
UPSCALE_NEAREST, UPSCALE_BILINEAR, UPSCALE_CUBIC = 0, 1, 3      # (2 is no upscale and keeps raising)
AGG_MIN, AGG_MEAN, AGG_MAX = 0, 1, 2
MAX_SEGMENTS, MAX_UPDATES = 256, 10
MAX_CONNECT_PIXELS = 1 << 24      # connected slots: the segment sums are 32-bit

# data_generator_mscmrseg.py:46, 57-60, 69
(ENTRY_SUPERPIXELS, ENTRY_NOISE_ALPHA, ENTRY_HUE) = range(3)
STYLE_ENTRY_NAMES = ("superpixels", "simplex_noise_alpha", "hue_saturation")
SUPERPIXELS_P_REPLACE, SUPERPIXELS_SEGMENTS = (0.0, 1.0), (20, 200)
SUPERPIXELS_UPDATES, SUPERPIXELS_COMPACTNESS = 5, 10
SUPERPIXELS_MAX_SIZE = 128        # imgaug's default max_size (f9c): what the _scaled_ presets put into iarg[6]
EDGE_ALPHA, EDGE_DIRECTION = (0.5, 1.0), (0.0, 1.0)
HUE_VALUE = (-20, 20)
# this build's own (imgaug's defaults where it has one): 1..3 grids of 2..16 cells per side, nearest or bilinear with equal
# probability, min / mean / max with equal probability, the sigmoid always on with a threshold drawn from N(0, 5)
NOISE_ITERATIONS, NOISE_SIZE, NOISE_SIGMOID_P, NOISE_THRESH_SIGMA = (1, 3), (2, 16), 1.0, 5.0
# interp="cubic" (f8b): the share of noise-alpha slots whose upscale becomes cubic.  This build's choice: recalled as the
# weight imgaug's default upscale_method gives "cubic", which cannot be checked here (imgaug is not installed)
NOISE_CUBIC_P = 0.35

_M32 = np.uint64(0xFFFFFFFF)
_F2, _G2 = 0.5 * (math.sqrt(3.0) - 1.0), (3.0 - math.sqrt(3.0)) / 6.0
# eight gradients, two squares turned against the axes and the diagonals: with Perlin's (+-1, +-1), (+-1, 0), (0, +-1) the three corner
# terms cancel to ~1e-14 on whole families of integer points, which puts the mask within rounding error of exactly 1/2
_GRAD = ((1.0, 0.3), (-0.3, 1.0), (-1.0, -0.3), (0.3, -1.0), (0.8, 0.7), (-0.7, 0.8), (-0.8, -0.7), (0.7, -0.8))


def philox_word0(key: int, counter) -> np.ndarray:
    """uint32: the first word of Philox4x32-10 as ``csrc/photometric.hip`` implements it, key = a 64-bit integer, counter
    ``(c, 0, 0, 0)`` for every c of the array"""
    k0, k1 = np.uint64(int(key) & 0xFFFFFFFF), np.uint64(int(key) >> 32)
    c0 = np.asarray(counter).astype(np.uint64)
    c1, c2, c3 = np.zeros_like(c0), np.zeros_like(c0), np.zeros_like(c0)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0.astype(np.uint32)


def _philox_word0_scalar(key: int, c: int) -> int:
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    c0, c1, c2, c3 = c & 0xFFFFFFFF, 0, 0, 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def threshold(p: float) -> int:
    """``floor(p 2^32)``, at most ``2^32 - 1``: a segment is replaced iff its 32-bit draw is below it"""
    return min(int(np.floor(float(p) * 4294967296.0)), 4294967295)


def edge_detect_weights(alpha: float) -> np.ndarray:
    """float64 ``[3,3]``: ``(1 - a) I + a [[0,1,0],[1,-4,1],[0,1,0]]`` (imgaug's EdgeDetect)"""
    ident = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float64)
    eff = np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]], dtype=np.float64)
    return (1.0 - float(alpha)) * ident + float(alpha) * eff


def directed_edge_weights(alpha: float, direction: float) -> np.ndarray:
    """float64 ``[3,3]``: imgaug's DirectedEdgeDetect construction.  ``direction`` in turns (0 = up, clockwise): the unit
    vector ``(cos(a - pi / 2), sin(a - pi / 2))``, ``a = 2 pi direction``; the similarity of neighbour ``(x, y)`` is
    ``(1 - angle / 180)^4`` with the angle between the two vectors in degrees; the similarities are normalised to sum 1,
    the centre is -1, and the result is blended with the identity by alpha (imgaug truncates the direction to whole
    degrees; this does not)"""
    rad = 2.0 * math.pi * float(direction)
    dx, dy = math.cos(rad - 0.5 * math.pi), math.sin(rad - 0.5 * math.pi)
    eff = np.zeros((3, 3), dtype=np.float64)
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            if (x, y) != (0, 0):
                norm = math.sqrt(float(x * x + y * y))
                cosine = min(1.0, max(-1.0, (x * dx + y * dy) / norm))
                eff[y + 1, x + 1] = (1.0 - math.degrees(math.acos(cosine)) / 180.0) ** 4
    eff = eff / eff.sum()
    eff[1, 1] = -1.0
    ident = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float64)
    return (1.0 - float(alpha)) * ident + float(alpha) * eff


def simplex_grid(h2: int, w2: int, seed: int) -> np.ndarray:
    """float64 ``[h2,w2]`` in [0, 1]: 2-D simplex noise (Gustavson's formulation: skew ``F2 = (sqrt 3 - 1) / 2``, unskew
    ``G2 = (3 - sqrt 3) / 6``, three corners with ``max(0, 0.5 - x^2 - y^2)^4 (g . (x, y))``, times 70) at the integer points
    ``(x, y) = (column + ox, row + oy)``, where the offsets ``ox, oy = 1 + (word & 0xFFF)`` come from the first Philox words for the
    counters 0xFFFFFFFF and 0xFFFFFFFE (the noise is exactly 0 at the origin; away from it no mask value is exactly 1/2, so
    no blend sits exactly on a rounding boundary); the gradient of the simplex lattice point ``(i, j)`` is one of eight directions (``_GRAD``), index = the
    low three bits of the first Philox word for counter ``(i & 0xFFFF) << 16 | (j & 0xFFFF)`` under ``seed``; the value is
    ``clip((n + 1) / 2, 0, 1)``.  ``simplex_grid_scalar`` is the same in plain Python floats."""
    ox, oy = (1.0 + float(int(v) & 0xFFF) for v in philox_word0(seed, np.array([0xFFFFFFFF, 0xFFFFFFFE], dtype=np.uint32)))
    y, x = np.meshgrid(np.arange(h2, dtype=np.float64) + oy, np.arange(w2, dtype=np.float64) + ox, indexing="ij")
    s = (x + y) * _F2
    i, j = np.floor(x + s), np.floor(y + s)
    t = (i + j) * _G2
    x0, y0 = x - (i - t), y - (j - t)
    i1 = (x0 > y0).astype(np.float64)
    j1 = 1.0 - i1
    grad = np.array(_GRAD, dtype=np.float64)
    total = np.zeros((h2, w2), dtype=np.float64)
    for di, dj, xk, yk in ((0.0, 0.0, x0, y0), (i1, j1, x0 - i1 + _G2, y0 - j1 + _G2),
                           (1.0, 1.0, x0 - 1.0 + 2.0 * _G2, y0 - 1.0 + 2.0 * _G2)):
        ii, jj = (i + di).astype(np.int64), (j + dj).astype(np.int64)
        g = grad[philox_word0(seed, ((ii & 0xFFFF) << 16) | (jj & 0xFFFF)) & np.uint32(7)]
        tt = 0.5 - xk * xk - yk * yk
        t2 = tt * tt
        total = total + np.where(tt < 0.0, 0.0, t2 * t2 * (g[..., 0] * xk + g[..., 1] * yk))
    return np.clip((70.0 * total + 1.0) * 0.5, 0.0, 1.0)


def simplex_grid_scalar(h2: int, w2: int, seed: int) -> np.ndarray:
    out = np.zeros((h2, w2), dtype=np.float64)
    ox = 1.0 + float(_philox_word0_scalar(int(seed), 0xFFFFFFFF) & 0xFFF)
    oy = 1.0 + float(_philox_word0_scalar(int(seed), 0xFFFFFFFE) & 0xFFF)
    for row in range(h2):
        for col in range(w2):
            x, y = float(col) + ox, float(row) + oy
            s = (x + y) * _F2
            i, j = math.floor(x + s), math.floor(y + s)
            t = (i + j) * _G2
            x0, y0 = x - (i - t), y - (j - t)
            i1, j1 = (1, 0) if x0 > y0 else (0, 1)
            total = 0.0
            for di, dj, xk, yk in ((0, 0, x0, y0), (i1, j1, x0 - i1 + _G2, y0 - j1 + _G2),
                                   (1, 1, x0 - 1.0 + 2.0 * _G2, y0 - 1.0 + 2.0 * _G2)):
                gx, gy = _GRAD[_philox_word0_scalar(int(seed), (((i + di) & 0xFFFF) << 16) | ((j + dj) & 0xFFFF)) & 7]
                tt = 0.5 - xk * xk - yk * yk
                t2 = tt * tt
                total = total + (0.0 if tt < 0.0 else t2 * t2 * (gx * xk + gy * yk))
            out[row, col] = min(1.0, max(0.0, (70.0 * total + 1.0) * 0.5))
    return out


def superpixel_grid(n_segments: int, h: int, w: int):
    """(gy, gx) for about ``n_segments`` square cells: ``gy = max(1, floor(sqrt(n h / w) + 0.5))``, ``gx = max(1, floor(n / gy +
    0.5))``, at most one cell per pixel row / column, the larger side reduced until ``gy gx <= 256``"""
    n = float(n_segments)
    gy = min(h, max(1, int(math.floor(math.sqrt(n * h / w) + 0.5))))
    gx = min(w, max(1, int(math.floor(n / gy + 0.5))))
    while gy * gx > MAX_SEGMENTS:
        if gy >= gx:
            gy -= 1
        else:
            gx -= 1
    return gy, gx


def superpixel_min_size(gy: int, gx: int, h: int, w: int) -> int:
    """``max(1, (H W) // (2 gy gx))``: half the mean segment size, skimage's ``min_size_factor = 0.5`` (f9b)"""
    return max(1, (int(h) * int(w)) // (2 * int(gy) * int(gx)))


def superpixel_working_size(h: int, w: int, max_size: int):
    """(h', w') a SUPERPIXELS slot with ``max_size`` works on (f9c): ``(max(1, (h m) // L), max(1, (w m) // L))`` with ``L = max(h,
    w)`` iff ``m >= 1`` and ``L > m`` (the longer side becomes exactly m), else ``(h, w)``.  Integers only, this build's own
    (imgaug computes ``int(h * (m / L))`` in floating point; parity is unpinned)"""
    h, w, m = int(h), int(w), int(max_size)
    big = max(h, w)
    if m < 1 or big <= m:
        return h, w
    return max(1, (h * m) // big), max(1, (w * m) // big)


@dataclass
class StyleProgram(SlotProgram):
    """``opcode`` int32 ``[B,S]``, ``iarg`` int32 ``[B,S,12]``, ``farg`` float64 ``[B,S,16]``, ``table`` float64 ``[B,S,768]``, ``seed``
    uint64 ``[B,S]`` (numpy, on the host; the module docstring says what each opcode reads).  The ``set_*`` methods encode slot
    ``s`` of sample ``i``."""
    opcode: np.ndarray
    iarg: np.ndarray
    farg: np.ndarray
    table: np.ndarray
    seed: np.ndarray
    COLUMNS = (("iarg", np.int32, IARGS), ("farg", np.float64, FARGS), ("table", np.float64, TABLE))

    def set_hue_saturation(self, i, s, dh, ds):
        self._clear(i, s, OP_HUE_SATURATION)
        self.iarg[i, s, 0], self.iarg[i, s, 1] = int(dh), int(ds)

    def set_noise_alpha(self, i, s, weights3x3, grids, upscale=UPSCALE_BILINEAR, aggregation=AGG_MAX, sigmoid=True, thresh=0.0):
        """``grids``: 1..3 arrays ``[h', w']`` (2..16 per side) of mask values in [0, 1] (``simplex_grid``)"""
        grids = [np.asarray(g, dtype=np.float64) for g in grids]
        if not 1 <= len(grids) <= MAX_GRIDS or any(g.ndim != 2 or g.size > GRID_VALUES for g in grids):
            raise ValueError("set_noise_alpha: 1..3 grids of at most 16 x 16 values")
        self._clear(i, s, OP_NOISE_ALPHA_CONV3X3)
        self.iarg[i, s, :4] = (len(grids), int(upscale), int(aggregation), int(bool(sigmoid)))
        for k, g in enumerate(grids):
            self.iarg[i, s, 4 + 2 * k:6 + 2 * k] = g.shape
            self.table[i, s, GRID_VALUES * k:GRID_VALUES * k + g.size] = g.reshape(-1)
        self.farg[i, s, :9] = np.asarray(weights3x3, dtype=np.float64).reshape(9)
        self.farg[i, s, 9] = thresh

    def set_superpixels(self, i, s, gy, gx, p_replace, seed, iters=SUPERPIXELS_UPDATES, compactness=SUPERPIXELS_COMPACTNESS,
                        min_size=0, max_size=0):
        """``min_size`` (``iarg[5]``): 0 = f9's slot; >= 1 = connected segments (f9b, ``superpixel_min_size``).  ``max_size``
        (``iarg[6]``): 0 = at full resolution; >= 1 = at the working size wherever the image's longer side exceeds it (f9c;
        ``gy``, ``gx`` and ``min_size`` then belong to ``superpixel_working_size(h, w, max_size)``)"""
        self._clear(i, s, OP_SUPERPIXELS)
        self.iarg[i, s, :4] = (int(gy), int(gx), int(iters), int(math.floor(float(compactness) ** 2 + 0.5)))
        self.iarg[i, s, 5], self.iarg[i, s, 6] = int(min_size), int(max_size)
        self.farg[i, s, 0], self.farg[i, s, 1] = p_replace, compactness
        self.seed[i, s] = seed

    def needs_connect(self) -> bool:
        """any SUPERPIXELS slot with ``iarg[5] > 0`` (a host-side look at the program)"""
        return bool(np.any((self.opcode == OP_SUPERPIXELS) & (self.iarg[..., 5] > 0)))

    def needs_scale(self, h: int, w: int) -> bool:
        """any SUPERPIXELS slot that is scaled on ``h x w`` images: ``1 <= iarg[6] < max(h, w)`` (a host-side look)"""
        m = self.iarg[..., 6]
        return bool(np.any((self.opcode == OP_SUPERPIXELS) & (m >= 1) & (m < max(int(h), int(w)))))

    def validate(self, h: Optional[int] = None, w: Optional[int] = None, channels: Optional[int] = None) -> None:
        """Raises ``ValueError`` (naming the field) for a program the kernels are not defined on: shapes and dtypes, more
        than 8 slots, unknown opcodes, non-finite ``farg`` / ``table``; hue on C other than 3, dh outside [-180, 180] or ds
        outside [-255, 255]; a grid count outside 1..3, a grid side outside 2..16, an unknown upscale or aggregation, a sigmoid
        flag that is not 0 / 1, table values outside [0, 1], a threshold beyond +/-1000; gy or gx below 1 or above H / W,
        ``gy gx > 256``, updates outside 0..10, M2 outside 0..2^20, p_replace outside [0, 1], min_size outside 0..H W, or
        min_size > 0 on more than 2^24 pixels; max_size below 0 and, for a slot that ``max_size`` scales on ``h x w`` (f9c), gy
        or gx above the working size's h' / w', min_size above h' w', or more than 2^24 pixels."""
        self._check_arrays(OP_SUPERPIXELS)
        op, ia, fa, tb = self.opcode, self.iarg, self.farg, self.table
        if channels is not None and not 1 <= channels <= 4:
            raise ValueError("StyleProgram: 1..4 channels, got %d" % channels)
        i = ia[op == OP_HUE_SATURATION]
        if len(i):
            if channels is not None and channels != 3:
                raise ValueError("StyleProgram: HUE_SATURATION takes 3 channels, got %d" % channels)
            if np.any(np.abs(i[:, 0]) > 180):
                raise ValueError("StyleProgram: HUE_SATURATION dh (iarg[0]) must be in [-180, 180]")
            if np.any(np.abs(i[:, 1]) > 255):
                raise ValueError("StyleProgram: HUE_SATURATION ds (iarg[1]) must be in [-255, 255]")
        m = op == OP_NOISE_ALPHA_CONV3X3
        i, f, t = ia[m], fa[m], tb[m]
        if len(i):
            if np.any((i[:, 0] < 1) | (i[:, 0] > MAX_GRIDS)):
                raise ValueError("StyleProgram: NOISE_ALPHA_CONV3X3 grid count (iarg[0]) must be in 1..3")
            if not np.all(np.isin(i[:, 1], (UPSCALE_NEAREST, UPSCALE_BILINEAR, UPSCALE_CUBIC))):
                raise ValueError("StyleProgram: NOISE_ALPHA_CONV3X3 upscale (iarg[1]) must be 0 (nearest), 1 (bilinear) or 3 (cubic)")
            if np.any((i[:, 2] < AGG_MIN) | (i[:, 2] > AGG_MAX)):
                raise ValueError("StyleProgram: NOISE_ALPHA_CONV3X3 aggregation (iarg[2]) must be 0 (min), 1 (mean) or 2 (max)")
            if np.any((i[:, 3] != 0) & (i[:, 3] != 1)):
                raise ValueError("StyleProgram: NOISE_ALPHA_CONV3X3 sigmoid (iarg[3]) must be 0 or 1")
            live = np.repeat(np.arange(MAX_GRIDS)[None, :] < i[:, 0:1], 2, axis=1)
            sides = i[:, 4:4 + 2 * MAX_GRIDS]
            if np.any(((sides < 2) | (sides > 16)) & live):
                raise ValueError("StyleProgram: NOISE_ALPHA_CONV3X3 grid sides (iarg[4:10]) must be in 2..16")
            if np.any((t < 0.0) | (t > 1.0)):
                raise ValueError("StyleProgram.table: NOISE_ALPHA_CONV3X3 mask values must be in [0, 1]")
            if np.any(np.abs(f[:, 9]) > 1000.0):
                raise ValueError("StyleProgram: NOISE_ALPHA_CONV3X3 sigmoid threshold (farg[9]) must be in [-1000, 1000]")
        m = op == OP_SUPERPIXELS
        i, f = ia[m], fa[m]
        if len(i):
            if np.any(i[:, 6] < 0):
                raise ValueError("StyleProgram: SUPERPIXELS max_size (iarg[6]) must be at least 0")
            if h is not None and w is not None:      # f9c: a scaled slot's grid and min_size belong to its working size
                big, m = max(h, w), i[:, 6].astype(np.int64)
                sc = (m >= 1) & (big > m)
                if h * w > MAX_CONNECT_PIXELS and np.any(sc):
                    raise ValueError("StyleProgram: SUPERPIXELS max_size (iarg[6]) below the longer side takes images of at most "
                                     "2^24 pixels, got %d x %d" % (h, w))
                hs, ws = np.maximum(1, (h * m) // big), np.maximum(1, (w * m) // big)
                if np.any(sc & ((i[:, 0] > hs) | (i[:, 1] > ws))):
                    raise ValueError("StyleProgram: SUPERPIXELS gy, gx (iarg[0:2]) must be in 1..h', 1..w' of the working size "
                                     "that max_size (iarg[6]) gives")
                if np.any(sc & (i[:, 5].astype(np.int64) > hs * ws)):
                    raise ValueError("StyleProgram: SUPERPIXELS min_size (iarg[5]) must be in 0..h' w' of the working size that "
                                     "max_size (iarg[6]) gives")
            if np.any(i[:, 0] < 1) or np.any(i[:, 1] < 1) or (h is not None and np.any(i[:, 0] > h)) or \
                    (w is not None and np.any(i[:, 1] > w)):
                raise ValueError("StyleProgram: SUPERPIXELS gy, gx (iarg[0:2]) must be in 1..H, 1..W")
            if np.any(i[:, 0].astype(np.int64) * i[:, 1] > MAX_SEGMENTS):
                raise ValueError("StyleProgram: SUPERPIXELS gy gx must be at most %d" % MAX_SEGMENTS)
            if np.any((i[:, 2] < 0) | (i[:, 2] > MAX_UPDATES)):
                raise ValueError("StyleProgram: SUPERPIXELS updates (iarg[2]) must be in 0..%d" % MAX_UPDATES)
            if np.any((i[:, 3] < 0) | (i[:, 3] > (1 << 20))):
                raise ValueError("StyleProgram: SUPERPIXELS M2 (iarg[3], compactness squared) must be in 0..2^20")
            if np.any((f[:, 0] < 0) | (f[:, 0] > 1)):
                raise ValueError("StyleProgram: SUPERPIXELS p_replace (farg[0]) must be in [0, 1]")
            if np.any(i[:, 5] < 0) or (h is not None and w is not None and np.any(i[:, 5].astype(np.int64) > h * w)):
                raise ValueError("StyleProgram: SUPERPIXELS min_size (iarg[5]) must be in 0..H W")
            if h is not None and w is not None and h * w > MAX_CONNECT_PIXELS and np.any(i[:, 5] > 0):
                raise ValueError("StyleProgram: SUPERPIXELS min_size (iarg[5]) > 0 takes images of at most 2^24 pixels, got %d x %d"
                                 % (h, w))

    def kernel_arrays(self, h: int, w: int, channels: Optional[int] = None):
        """(opcode, iarg, farg, table, seed as int64 bits) as the kernel takes them: validated for ``h x w x channels``
        images, with the replacement thresholds in ``iarg[4]``"""
        self.validate(h, w, channels)
        ia = self.iarg.copy()
        for i, s in zip(*np.nonzero(self.opcode == OP_SUPERPIXELS)):
            ia[i, s, 4] = np.array(threshold(self.farg[i, s, 0]), dtype=np.uint32).view(np.int32)      # (the bits)
        return self.opcode, ia, self.farg, self.table, self.seed.view(np.int64)

    def apply(self, images, masks):
        return stylize_aug(images, self), masks


# ------------------------------------------------------------------------------------------------ sampling
def draw_style(b: int, rng: np.random.Generator):
    """the parameters of the three entries for every sample of a batch (the reference's ranges; the module constants say
    what this build chose where imgaug leaves a default)"""
    u = lambda lo_hi, *shape: rng.uniform(lo_hi[0], lo_hi[1], (b,) + shape)
    return dict(
        sp_p=u(SUPERPIXELS_P_REPLACE), sp_n=rng.integers(SUPERPIXELS_SEGMENTS[0], SUPERPIXELS_SEGMENTS[1] + 1, b),
        sp_seed=rng.integers(0, 2 ** 64, b, dtype=np.uint64),
        na_kind=rng.integers(0, 2, b), na_alpha=u(EDGE_ALPHA), na_dir=u(EDGE_DIRECTION),
        na_iters=rng.integers(NOISE_ITERATIONS[0], NOISE_ITERATIONS[1] + 1, b),
        na_size=rng.integers(NOISE_SIZE[0], NOISE_SIZE[1] + 1, (b, MAX_GRIDS, 2)),
        na_up=rng.integers(0, 2, b), na_agg=rng.integers(0, 3, b), na_sig=rng.random(b) < NOISE_SIGMOID_P,
        na_thresh=rng.standard_normal(b) * NOISE_THRESH_SIGMA, na_seed=rng.integers(0, 2 ** 64, (b, MAX_GRIDS), dtype=np.uint64),
        hue=rng.integers(HUE_VALUE[0], HUE_VALUE[1] + 1, b))


def encode_style(prog: StyleProgram, i: int, s: int, entry: int, d, h: int, w: int, connected: bool = False,
                 scaled: bool = False) -> None:
    """``connected``: Superpixels slots get ``min_size = superpixel_min_size(gy, gx, h, w)`` (the ``_connected_`` presets).
    ``scaled``: they get ``max_size = SUPERPIXELS_MAX_SIZE``, and the grid and ``min_size`` are those of the working size
    ``superpixel_working_size(h, w, 128)`` (the ``_scaled_`` presets)"""
    if entry == ENTRY_SUPERPIXELS:
        m = SUPERPIXELS_MAX_SIZE if scaled else 0
        hs, ws = superpixel_working_size(h, w, m)
        gy, gx = superpixel_grid(int(d["sp_n"][i]), hs, ws)
        prog.set_superpixels(i, s, gy, gx, d["sp_p"][i], d["sp_seed"][i],
                             min_size=superpixel_min_size(gy, gx, hs, ws) if connected else 0, max_size=m)
    elif entry == ENTRY_NOISE_ALPHA:
        wts = edge_detect_weights(d["na_alpha"][i]) if d["na_kind"][i] == 0 else directed_edge_weights(d["na_alpha"][i], d["na_dir"][i])
        grids = [simplex_grid(int(d["na_size"][i, k, 0]), int(d["na_size"][i, k, 1]), int(d["na_seed"][i, k]))
                 for k in range(int(d["na_iters"][i]))]
        prog.set_noise_alpha(i, s, wts, grids, int(d["na_up"][i]), int(d["na_agg"][i]), bool(d["na_sig"][i]), d["na_thresh"][i])
    else:
        v = int(d["hue"][i])
        prog.set_hue_saturation(i, s, int(math.floor(v * 180.0 / 255.0 + 0.5)), v)


def upload_style_program(program: StyleProgram, batch: int, h: int, w: int, channels: int, device: torch.device):
    """Validate on the host, then move the kernel's arrays through pinned, non-blocking copies (no synchronisation)."""
    return upload(program, batch, h, w, channels, device=device)


def stylize_aug(images: torch.Tensor, program: Optional[StyleProgram] = None) -> torch.Tensor:
    """uint8 ``[B,H,W,C]`` images on the device -> the stylized uint8 images (a new tensor).  ``program`` is required: build
    it with ``StyleProgram.set_*`` or draw it with ``sample_style_program(B, "heavy_full_device", rng, H, W)``."""
    if program is None:
        raise TypeError("stylize_aug: program is required (sample_style_program(batch, preset, rng, h, w)); there is no silent identity")
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise TypeError("stylize_aug: uint8 [B,H,W,C] images")
    b, h, w, c = images.shape
    arrays = upload_style_program(program, b, h, w, c, images.device)
    if program.needs_scale(h, w):
        return K.stylize_scaled(images, *arrays)
    return K.stylize(images, *arrays, connect=program.needs_connect())
