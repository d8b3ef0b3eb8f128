"""Device-side geometric augmentation for the loader path: the warps of the reference's default
recipe ``ImageProcessor.augmentation`` (``src/data_generator_mscmrseg.py:20-84``, called at ``:305-309``; the MM-WHS generator's
own copy is ``src/data_generator_mmwhs.py:17-84``) -- ``Fliplr``, ``Flipud``, ``CropAndPad``, ``Affine`` over +/-45 degrees and
+/-20 % with every border mode, ``ElasticTransformation``, ``PiecewiseAffine``, ``PerspectiveTransform`` -- as a per-sample
PROGRAM that one HIP entry point (``csrc/geometric.hip``) runs over uint8 ``[B,H,W,C]`` images and integer masks.  All of them
move the mask, and with it the point cloud the sampler draws.

A program has ``S`` slots per sample (``S <= 8``); slot ``s`` of sample ``i`` is ``opcode[i, s]`` with ``iarg[i, s, :4]`` (int32:
interpolation order 0 / 1 / 3, border mode, cval 0..255, one opcode argument), ``farg[i, s, :32]`` (float64) and ``seed[i, s]``
(uint64).  Every slot is one resampling: a source coordinate ``(sx, sy)`` per output pixel ``(x, y)`` in float64, then

* order 0: the texel at ``floor(s + 0.5)``; order 1: bilinear over ``floor(s)`` and ``floor(s) + 1`` per axis, summed in f6's
  order, ``floor(v + 0.5)`` clipped to [0, 255]; the value is uint8 again between two slots
* order 3 (f8b): the Keys cubic convolution with ``A = -0.75`` (the constant OpenCV documents for ``INTER_CUBIC``) over the 4 x 4
  neighbours ``floor(s) - 1 .. floor(s) + 2``.  With ``t = s - floor(s)``, ``u = t + 1``, ``r = 1 - t``, float64, every operation
  rounded on its own: ``wm = ((A u - 5 A) u + 8 A) u - 4 A``, ``w0 = ((A + 2) t - (A + 3)) t t + 1``, ``w1 = ((A + 2) r - (A + 3)) r r
  + 1``, ``w2 = ((1 - wm) - w0) - w1``; a row is ``((p[-1] wxm + p[0] wx0) + p[1] wx1) + p[2] wx2``, the four rows are summed
  likewise with the y weights, ``floor(v + 0.5)`` clipped to [0, 255] (the clip is live: cubic overshoots).  An integer
  coordinate returns the texel's bits.  A program that holds an order-3 slot runs through ``pcuda_geometric_cubic``, a kernel
  instance of its own (``GeoProgram.uses_cubic()``, a host-side look); every other program runs where it always ran
* border mode per neighbour index: ``MODE_CONSTANT`` (``cval``; scipy ``grid-constant``), ``MODE_EDGE`` (``nearest``),
  ``MODE_REFLECT`` (no edge repeat; ``mirror``), ``MODE_SYMMETRIC`` (``reflect``), ``MODE_WRAP`` (``grid-wrap``)
* masks take order 0 and constant 0 at the same coordinate, whatever the image's order, mode and cval are (f6's rule)
* a NaN coordinate or one beyond 2^30 takes ``cval`` in every mode

====================  ==========================================================================================
``OP_NOP``            copy
``OP_HOMOGRAPHY``     ``farg[0..8]`` = the inverse 3x3 map (output pixel -> source coordinate), row-major:
                      ``d = (h6 x + h7 y) + h8``, ``sx = ((h0 x + h1 y) + h2) / d``, ``sy`` likewise.  Flips, the heavy
                      ``Affine``, ``CropAndPad`` and ``PerspectiveTransform`` are encoded as this opcode
``OP_ELASTIC``        ``iarg[3]`` = radius ``int(4 sigma + 0.5)`` (0..4), ``farg[0]`` = alpha, ``farg[1..1+r]`` = f7's
                      ``gaussian_weights(sigma)``, ``farg[31]`` = sigma (a note for the reader; no interpreter uses it); uniform
                      noise in (-1, 1) from f7's Philox4x32-10 (key = ``seed``, counter = the pixel's index, words 0 and 1 for
                      dx and dy, reflect-101 outside the image), blurred along y then x, ``sx = x + alpha bx``
``OP_PIECEWISE``      ``iarg[3]`` = G (2..4): a regular ``G x G`` grid of control points over ``[0, W-1] x [0, H-1]`` whose
                      source positions are ``farg[i G + j]`` (x) and ``farg[16 + i G + j]`` (y); every cell is split along
                      its TL-BR diagonal and interpolated linearly on each triangle
====================  ==========================================================================================

imgaug / skimage / cv2 are not vendored by the reference: parity with imgaug is unpinned, the convention is this build's own
and is pinned by ``tests/golden/geometric.npz`` (``scripts/make_geometric_golden.py``: a scipy ``map_coordinates`` and a
plain-numpy restatement).  One divergence from the reference's recipe is left: imgaug's parameter stream is not reproduced.
``CropAndPad`` with all ten modes of ``numpy.pad`` (``pad_mode=ia.ALL``: the five above plus ``linear_ramp``, ``maximum``,
``mean``, ``median``, ``minimum``) lives in ``utils/croppad.py`` (f14) as a program of its own: the presets
``"heavy_refpad_device"`` and ``"mscmrseg_aug2_refpad_device"`` of ``sample_heavy_plan`` draw it, while ``set_crop_and_pad`` here
and the four older presets keep the five modes above.  Order 3 is pinned by ``tests/golden/geometric_cubic.npz``
(``scripts/make_geometric_cubic_golden.py``: the numpy restatement and one in exact rational arithmetic); it is NOT scipy's
``order=3`` (no spline prefilter) and not cv2's 1/32-pixel fixed-point tables, and the samplers draw it only with
``interp="cubic"`` (every elastic slot; imgaug's elastic default).  NOT built: order 2, 4 and 5; the string ``"heavy"``
keeps raising ``NotImplementedError``.  ``Superpixels``, ``SimplexNoiseAlpha(EdgeDetect | DirectedEdgeDetect)`` and
``AddToHueAndSaturation`` live in ``utils/stylize.py`` (f9): the presets ``"heavy_full_device"`` and
``"mscmrseg_aug2_full_device"`` of ``sample_heavy_plan`` interleave them with the entries of this file and f7's."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import kernels as K
from ._program import SlotProgram, as_labels, like_masks, upload
from .affine import AugmentParams, inverse_matrices
from .photometric import gaussian_weights, photometric_aug  # noqa: F401  (photometric_aug: importable from here as before)

OP_NOP, OP_HOMOGRAPHY, OP_ELASTIC, OP_PIECEWISE = range(4)
OP_NAMES = ("NOP", "HOMOGRAPHY", "ELASTIC", "PIECEWISE_AFFINE")
MODE_CONSTANT, MODE_EDGE, MODE_REFLECT, MODE_SYMMETRIC, MODE_WRAP = range(5)
MODE_NAMES = ("CONSTANT", "EDGE", "REFLECT", "SYMMETRIC", "WRAP")
MAX_SLOTS, IARGS, FARGS = 8, 4, 32
MAX_ELASTIC_RADIUS = 4
ORDERS = (0, 1, 3)                     # nearest, bilinear, Keys cubic (f8b)

# data_generator_mscmrseg.py:25-43, 74-76
FLIP_LR_P, FLIP_UD_P, SOMETIMES_P = 0.5, 0.2, 0.5
CROP_PAD_PERCENT = (-0.05, 0.1)
HEAVY_SCALE = (0.8, 1.2)
HEAVY_TRANSLATE = (-0.2, 0.2)
HEAVY_ROTATE = (-45.0, 45.0)
HEAVY_SHEAR = (-16.0, 16.0)
ELASTIC_ALPHA, ELASTIC_SIGMA = (0.5, 3.5), 0.25
PIECEWISE_SCALE, PIECEWISE_GRID = (0.01, 0.05), 4
PERSPECTIVE_SCALE = (0.01, 0.1)
PERSPECTIVE_MAX_JITTER = 0.45          # two facing corners never cross (imgaug wraps |jitter| instead)
SOMEOF_COUNT = (0, 5)

# the geometric entries of the recipe, in the reference's order
(ENTRY_FLIPLR, ENTRY_FLIPUD, ENTRY_CROP_AND_PAD, ENTRY_AFFINE, ENTRY_ELASTIC, ENTRY_PIECEWISE, ENTRY_PERSPECTIVE) = range(7)
GEO_ENTRY_NAMES = ("fliplr", "flipud", "crop_and_pad", "affine", "elastic", "piecewise", "perspective")


def crop_pad_pixels(percent: float, size: int) -> int:
    """signed pixels of one side: ``floor(percent size + 0.5)``, positive pads"""
    return int(np.floor(float(percent) * size + 0.5))


def perspective_matrix(jitter, h: int, w: int) -> np.ndarray:
    """float64 ``[3,3]``: the map from the output's corners (TL, TR, BR, BL) to the source quad, the four corners moved
    inward by ``|jitter[k]| = (fraction of W, fraction of H)``; ``h8 = 1``, the 8x8 system solved in float64"""
    j = np.abs(np.asarray(jitter, dtype=np.float64)).reshape(4, 2)
    xo = np.array([0.0, w - 1.0, w - 1.0, 0.0])
    yo = np.array([0.0, 0.0, h - 1.0, h - 1.0])
    xs = np.array([j[0, 0] * w, w - 1.0 - j[1, 0] * w, w - 1.0 - j[2, 0] * w, j[3, 0] * w])
    ys = np.array([j[0, 1] * h, j[1, 1] * h, h - 1.0 - j[2, 1] * h, h - 1.0 - j[3, 1] * h])
    a = np.zeros((8, 8), dtype=np.float64)
    rhs = np.zeros(8, dtype=np.float64)
    for k in range(4):
        a[2 * k] = [xo[k], yo[k], 1.0, 0.0, 0.0, 0.0, -xs[k] * xo[k], -xs[k] * yo[k]]
        a[2 * k + 1] = [0.0, 0.0, 0.0, xo[k], yo[k], 1.0, -ys[k] * xo[k], -ys[k] * yo[k]]
        rhs[2 * k], rhs[2 * k + 1] = xs[k], ys[k]
    return np.append(np.linalg.solve(a, rhs), 1.0).reshape(3, 3)


def control_grid(g: int, h: int, w: int):
    """float64 ``[G]`` x and y positions of the control points: ``X_j = j (W - 1) / (G - 1)``, ``Y_i = i (H - 1) / (G - 1)``"""
    k = np.arange(g, dtype=np.float64)
    return k * (w - 1.0) / (g - 1.0), k * (h - 1.0) / (g - 1.0)


@dataclass
class GeoProgram(SlotProgram):
    """``opcode`` int32 ``[B,S]``, ``iarg`` int32 ``[B,S,4]``, ``farg`` float64 ``[B,S,32]``, ``seed`` uint64 ``[B,S]`` (numpy, on
    the host; the module docstring says what each opcode reads).  The ``set_*`` methods encode slot ``s`` of sample ``i``."""
    opcode: np.ndarray
    iarg: np.ndarray
    farg: np.ndarray
    seed: np.ndarray
    COLUMNS = (("iarg", np.int32, IARGS), ("farg", np.float64, FARGS))

    def _clear(self, i, s, op, order=0, mode=MODE_CONSTANT, cval=0):
        self.opcode[i, s] = op
        self.iarg[i, s] = (int(order), int(mode), int(cval), 0)
        self.farg[i, s] = 0.0
        self.seed[i, s] = 0

    def set_homography(self, i, s, matrix, order=1, mode=MODE_CONSTANT, cval=0):
        """``matrix``: the INVERSE 3x3 map, output pixel -> source coordinate"""
        self._clear(i, s, OP_HOMOGRAPHY, order, mode, cval)
        self.farg[i, s, :9] = np.asarray(matrix, dtype=np.float64).reshape(9)

    def set_flip_lr(self, i, s, w):
        self.set_homography(i, s, [[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], order=0)

    def set_flip_ud(self, i, s, h):
        self.set_homography(i, s, [[1.0, 0.0, 0.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]], order=0)

    def set_affine(self, i, s, h, w, scale_x=1.0, scale_y=1.0, translate_x=0.0, translate_y=0.0, rotate=0.0, shear=0.0, order=1,
                   mode=MODE_CONSTANT, cval=0):
        """f6's matrix convention (``utils/affine.py``: ``A = T(c + t) . R . Sh . S . T(-c)`` about the image centre,
        ``translate_*`` fractions of the width / height, ``rotate`` / ``shear`` degrees), its inverse as a homography, plus
        the border mode"""
        p = AugmentParams.identity(1)
        p.affine_on[:] = True
        p.scale_x[:], p.scale_y[:], p.translate_x[:], p.translate_y[:] = scale_x, scale_y, translate_x, translate_y
        p.rotate[:], p.shear[:] = rotate, shear
        inv = inverse_matrices(p, h, w)[0]
        self.set_homography(i, s, np.vstack([inv, [0.0, 0.0, 1.0]]), order, mode, cval)

    def set_crop_and_pad(self, i, s, h, w, top, right, bottom, left, mode=MODE_CONSTANT, cval=0):
        """signed pixels per side, positive pads, negative crops; the output keeps its size: half-pixel-centre resize
        ``sx = (x + 0.5) (W + l + r) / W - 0.5 - l`` and y likewise, order 1"""
        ax, ay = (w + float(left) + float(right)) / w, (h + float(top) + float(bottom)) / h
        self.set_homography(i, s, [[ax, 0.0, 0.5 * ax - 0.5 - float(left)], [0.0, ay, 0.5 * ay - 0.5 - float(top)],
                                   [0.0, 0.0, 1.0]], 1, mode, cval)

    def set_perspective(self, i, s, h, w, jitter):
        """``jitter`` ``[4,2]`` (TL, TR, BR, BL; x, y): ``perspective_matrix``; constant fill 0, order 1"""
        self.set_homography(i, s, perspective_matrix(jitter, h, w), 1, MODE_CONSTANT, 0)

    def set_elastic(self, i, s, alpha, sigma, seed, order=1, mode=MODE_CONSTANT, cval=0):
        wts = gaussian_weights(sigma)
        self._clear(i, s, OP_ELASTIC, order, mode, cval)
        self.iarg[i, s, 3] = len(wts) - 1
        self.farg[i, s, 0] = alpha
        self.farg[i, s, 1:1 + len(wts)] = wts
        self.farg[i, s, 31] = sigma
        self.seed[i, s] = seed

    def set_piecewise(self, i, s, h, w, dx, dy, order=1, mode=MODE_CONSTANT, cval=0):
        """``dx``, ``dy`` ``[G,G]`` (row i, column j): the source position of control point (i, j) is its grid position plus
        ``(dx, dy)`` pixels"""
        dx, dy = np.asarray(dx, dtype=np.float64), np.asarray(dy, dtype=np.float64)
        g = dx.shape[0]
        if dx.shape != (g, g) or dy.shape != (g, g):
            raise ValueError("set_piecewise: dx and dy must be [G,G]")
        gx, gy = control_grid(g, h, w)
        self._clear(i, s, OP_PIECEWISE, order, mode, cval)
        self.iarg[i, s, 3] = g
        self.farg[i, s, :g * g] = (gx[None, :] + dx).reshape(-1)
        self.farg[i, s, 16:16 + g * g] = (gy[:, None] + dy).reshape(-1)

    def uses_cubic(self) -> bool:
        """any live slot of order 3 (a host-side look at the program: it picks the entry point)"""
        return bool(np.any((self.opcode != OP_NOP) & (self.iarg[..., 0] == 3)))

    def validate(self, h: Optional[int] = None, w: Optional[int] = None) -> None:
        """Raises ``ValueError`` for a program the kernel is not defined on: shapes and dtypes, more than 8 slots, unknown
        opcodes, non-finite arguments, an order outside {0, 1, 3}, a mode outside 0..4, a cval outside 0..255, an elastic
        radius above 4, a negative alpha or weights that are not normalised, G outside 2..4, a homography with
        ``|det| <= 1e-12`` or -- when ``h`` and ``w`` are given -- a denominator that is not positive at the four output
        corners; ``h`` or ``w`` below 2."""
        self._check_arrays(OP_PIECEWISE)
        op, ia, fa = self.opcode, self.iarg, self.farg
        if (h is not None and h < 2) or (w is not None and w < 2):
            raise ValueError("GeoProgram: H and W must be at least 2")
        live = op != OP_NOP
        if not np.all(np.isin(ia[live][:, 0], ORDERS)):
            raise ValueError("GeoProgram: order must be 0, 1 or 3 (nearest, bilinear, cubic)")
        if np.any((ia[live][:, 1] < 0) | (ia[live][:, 1] > MODE_WRAP)):
            raise ValueError("GeoProgram: mode must be in 0..4")
        if np.any((ia[live][:, 2] < 0) | (ia[live][:, 2] > 255)):
            raise ValueError("GeoProgram: cval must be in 0..255")
        f = fa[op == OP_HOMOGRAPHY]
        if len(f):
            m = f[:, :9].reshape(-1, 3, 3)
            if not np.all(np.abs(np.linalg.det(m)) > 1e-12):
                raise ValueError("GeoProgram: HOMOGRAPHY is singular (|det| <= 1e-12)")
            if h is not None and w is not None:
                for xc, yc in ((0.0, 0.0), (w - 1.0, 0.0), (w - 1.0, h - 1.0), (0.0, h - 1.0)):
                    if not np.all((m[:, 2, 0] * xc + m[:, 2, 1] * yc) + m[:, 2, 2] > 0):
                        raise ValueError("GeoProgram: HOMOGRAPHY denominator must be positive at the four output corners")
        i, f = ia[op == OP_ELASTIC], fa[op == OP_ELASTIC]
        if len(i):
            if np.any((i[:, 3] < 0) | (i[:, 3] > MAX_ELASTIC_RADIUS)):
                raise ValueError("GeoProgram: ELASTIC radius must be in 0..4 (sigma < 1.125)")
            if np.any(f[:, 0] < 0):
                raise ValueError("GeoProgram: ELASTIC alpha must not be negative")
            on = np.arange(1, MAX_ELASTIC_RADIUS + 1)[None, :] <= i[:, 3:4]
            wsum = f[:, 1] + 2.0 * np.where(on, f[:, 2:2 + MAX_ELASTIC_RADIUS], 0.0).sum(1)
            if np.any(f[:, 1] < 0) or np.any(np.where(on, f[:, 2:2 + MAX_ELASTIC_RADIUS], 0.0) < 0) or np.any(np.abs(wsum - 1.0) > 1e-12):
                raise ValueError("GeoProgram: ELASTIC weights must be non-negative and sum to 1")
        i = ia[op == OP_PIECEWISE]
        if np.any((i[:, 3] < 2) | (i[:, 3] > 4)):
            raise ValueError("GeoProgram: PIECEWISE_AFFINE G must be in 2..4")

    def kernel_arrays(self, h: int, w: int):
        """(opcode, iarg, farg, seed as int64 bits) as the kernel takes them, validated for an ``h x w`` image"""
        self.validate(h, w)
        return self.opcode, self.iarg, self.farg, self.seed.view(np.int64)

    def apply(self, images, masks):
        return geometric_aug(images, masks, self)


def upload_geo_program(program: GeoProgram, batch: int, h: int, w: int, device: torch.device):
    """Validate on the host, then move the kernel's arrays through pinned, non-blocking copies (no synchronisation)."""
    return upload(program, batch, h, w, device=device)


def geometric_aug(images: torch.Tensor, masks: Optional[torch.Tensor], program: Optional[GeoProgram] = None):
    """The warps of ``data_generator_mscmrseg.py:20-84``: uint8 ``[B,H,W,C]`` images and integer masks ``[B,H,W]`` /
    ``[B,H,W,1]`` (or ``None``) on the device -> ``(warped uint8 images, warped masks of the same shape and dtype)``, new
    tensors.  ``program`` is required: draw it with ``sample_geo_program(B, "heavy_device", rng, H, W)``."""
    if program is None:
        raise TypeError("geometric_aug: program is required (sample_geo_program(batch, preset, rng, h, w)); there is no silent identity")
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise TypeError("geometric_aug: uint8 [B,H,W,C] images")
    b, h, w, _ = images.shape
    up = upload_geo_program(program, b, h, w, images.device)
    out, lab_out = K.geometric(images, as_labels(masks), *up, cubic=program.uses_cubic())
    return out, like_masks(lab_out, masks)


# ------------------------------------------------------------------------------------------------ sampling
def _draw_geo(b, rng, h, w):
    u = lambda lo_hi, *shape: rng.uniform(lo_hi[0], lo_hi[1], (b,) + shape)
    g = PIECEWISE_GRID
    pw_scale, ps_scale = u(PIECEWISE_SCALE), u(PERSPECTIVE_SCALE)
    return dict(
        crop=u(CROP_PAD_PERCENT, 4), crop_mode=rng.integers(0, 5, b), crop_cval=rng.integers(0, 256, b),
        scale=u(HEAVY_SCALE, 2), translate=u(HEAVY_TRANSLATE, 2), rotate=u(HEAVY_ROTATE), shear=u(HEAVY_SHEAR),
        order=rng.integers(0, 2, b), cval=rng.integers(0, 256, b), mode=rng.integers(0, 5, b),
        alpha=u(ELASTIC_ALPHA), seed=rng.integers(0, 2 ** 64, b, dtype=np.uint64),
        pw_dx=rng.standard_normal((b, g, g)) * (pw_scale * w)[:, None, None],
        pw_dy=rng.standard_normal((b, g, g)) * (pw_scale * h)[:, None, None],
        jitter=np.clip(rng.standard_normal((b, 4, 2)) * ps_scale[:, None, None], -PERSPECTIVE_MAX_JITTER, PERSPECTIVE_MAX_JITTER))


def _encode_geo(prog, i, s, entry, d, h, w, elastic_order=1):
    if entry == ENTRY_FLIPLR:
        prog.set_flip_lr(i, s, w)
    elif entry == ENTRY_FLIPUD:
        prog.set_flip_ud(i, s, h)
    elif entry == ENTRY_CROP_AND_PAD:
        t, r, bt, l = d["crop"][i]
        prog.set_crop_and_pad(i, s, h, w, crop_pad_pixels(t, h), crop_pad_pixels(r, w), crop_pad_pixels(bt, h),
                              crop_pad_pixels(l, w), int(d["crop_mode"][i]), int(d["crop_cval"][i]))
    elif entry == ENTRY_AFFINE:
        prog.set_affine(i, s, h, w, d["scale"][i, 0], d["scale"][i, 1], d["translate"][i, 0], d["translate"][i, 1],
                        d["rotate"][i], d["shear"][i], int(d["order"][i]), int(d["mode"][i]), int(d["cval"][i]))
    elif entry == ENTRY_ELASTIC:
        prog.set_elastic(i, s, d["alpha"][i], ELASTIC_SIGMA, d["seed"][i], order=elastic_order)
    elif entry == ENTRY_PIECEWISE:
        prog.set_piecewise(i, s, h, w, d["pw_dx"][i], d["pw_dy"][i])
    else:
        prog.set_perspective(i, s, h, w, d["jitter"][i])
