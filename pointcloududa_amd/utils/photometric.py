"""Device-side photometric augmentation for the loader path: the photometric operators of the
reference's ``ImageProcessor.augmentation2`` (``src/data_generator_mscmrseg.py:87-132``, the recipe of the published
``aug2`` checkpoints) as a per-sample PROGRAM that one HIP entry point (``csrc/photometric.hip``) runs over uint8
``[B,H,W,C]`` images.  Masks and stored vertices are untouched by all of these operators.

A program has ``S`` slots per sample (``S <= 8``; the preset uses 5); slot ``s`` of sample ``i`` is ``opcode[i, s]`` with
``iarg[i, s, :4]`` (int32), ``farg[i, s, :16]`` (float64) and ``seed[i, s]`` (uint64):

====================  =========================================================================================
``OP_NOP``            copy
``OP_GAUSSIAN_BLUR``  ``iarg[0]`` = radius ``int(4 sigma + 0.5)`` (0..12), ``farg[0..radius]`` = the normalised weights
                      ``w[|d|]`` computed here (``gaussian_weights``), ``farg[15]`` = sigma; ``sigma < 0.125`` (radius 0) is
                      encoded as ``OP_NOP``; rows first, then columns, no rounding in between
``OP_AVERAGE_BLUR``   ``iarg[0]`` = k in 2..7, window offsets ``-(k // 2) .. k - k // 2 - 1``, ``(2 S + k k) // (2 k k)``
``OP_MEDIAN_BLUR``    ``iarg[0]`` = odd k in 3..11, replicated border
``OP_CONV3X3``        ``farg[0..8]`` = row-major weights of a correlation (``sharpen_weights``, ``emboss_weights``)
``OP_GAUSSIAN_NOISE`` ``farg[0]`` = scale, ``iarg[0]`` = per_channel, ``seed``
``OP_DROPOUT``        ``farg[0]`` = p, ``iarg[0]`` = per_channel, ``seed``; the kernel gets ``floor(p 2^32)`` in ``iarg[1]``
``OP_COARSE_DROPOUT`` ``farg[0]`` = p, ``farg[1]`` = size_percent, ``iarg[0]`` = per_channel, ``seed``; the kernel gets the
                      grid ``max(1, floor(H size_percent + 0.5))`` x likewise for W in ``iarg[2:4]``
``OP_INVERT``         ``iarg[0]`` = bit mask of the inverted channels
``OP_ADD``            ``iarg[ch]`` = the integer added to channel ch
``OP_MULTIPLY``       ``farg[ch]`` = the factor of channel ch
``OP_GRAYSCALE``      ``farg[0]`` = alpha; C = 3 with channel 0 = red (``0.299 c0 + 0.587 c1 + 0.114 c2``; MS-CMRSeg slices
                      are a grey image replicated to three channels, where the order does not matter); C = 1: copy
====================  =========================================================================================

The value is uint8 again between two slots; non-integer arithmetic is float64 in a fixed order, rounded ``floor(v + 0.5)``
and clipped; borders are reflect-101 (the median replicates).  The random operators draw from Philox4x32-10 as implemented
here (key = the slot's seed, counter = the element's index inside its sample), so the result depends on (image, program)
only.  imgaug / cv2 are not vendored by the reference: parity with imgaug is unpinned, the convention is this build's own
and is pinned by ``tests/golden/photometric.npz`` (``scripts/make_photometric_golden.py``: a scipy and a plain-numpy
restatement).

NOT in this program type: ``Superpixels``, ``SimplexNoiseAlpha(EdgeDetect | DirectedEdgeDetect)`` and
``AddToHueAndSaturation`` (the other three ``SomeOf`` entries) live in ``utils/stylize.py`` (f9); ``"heavy"`` keeps raising (imgaug's
parameter stream is not reproduced).  ``CropAndPad`` and the elastic / piecewise / perspective warps of the heavy ``augmentation`` pipeline move the mask:
they live in ``utils/geometric.py`` (f8); ``sample_heavy_plan`` (``utils/heavy.py``) interleaves them with the operators of this
file, whose nine entries it draws and encodes through ``draw_photo`` / ``encode_photo`` here, as ``sample_program`` does."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import kernels as K
from ._program import HEAVY_MESSAGE, SlotProgram, upload

(OP_NOP, OP_GAUSSIAN_BLUR, OP_AVERAGE_BLUR, OP_MEDIAN_BLUR, OP_CONV3X3, OP_GAUSSIAN_NOISE, OP_DROPOUT, OP_COARSE_DROPOUT,
 OP_INVERT, OP_ADD, OP_MULTIPLY, OP_GRAYSCALE) = range(12)
OP_NAMES = ("NOP", "GAUSSIAN_BLUR", "AVERAGE_BLUR", "MEDIAN_BLUR", "CONV3X3", "GAUSSIAN_NOISE", "DROPOUT", "COARSE_DROPOUT",
            "INVERT", "ADD", "MULTIPLY", "GRAYSCALE")
MAX_SLOTS, IARGS, FARGS = 8, 4, 16
SIGMA_NOP = 0.125              # below it the Gaussian's radius int(4 sigma + 0.5) is 0
PHOTOMETRIC_PRESET = "mscmrseg_aug2_photometric"
PRESET_SLOTS = 5

# data_generator_mscmrseg.py:96-124, the nine entries of the SomeOf list that are built, in the reference's order
(ENTRY_BLUR, ENTRY_SHARPEN, ENTRY_EMBOSS, ENTRY_NOISE, ENTRY_DROPOUT, ENTRY_INVERT, ENTRY_ADD, ENTRY_MULTIPLY,
 ENTRY_GRAYSCALE) = range(9)
SIGMA = (0.0, 3.0)
AVERAGE_K = (2, 7)
MEDIAN_K = (3, 11)
SHARPEN_ALPHA, SHARPEN_LIGHTNESS = (0.0, 1.0), (0.75, 1.5)
EMBOSS_ALPHA, EMBOSS_STRENGTH = (0.0, 1.0), (0.0, 2.0)
NOISE_SCALE, NOISE_PER_CHANNEL = (0.0, 0.05 * 255), 0.5
DROPOUT_P, DROPOUT_PER_CHANNEL = (0.01, 0.1), 0.5
COARSE_P, COARSE_SIZE, COARSE_PER_CHANNEL = (0.03, 0.15), (0.02, 0.05), 0.2
INVERT_P = 0.05
ADD, ADD_PER_CHANNEL = (-10, 10), 0.5
MULTIPLY, MULTIPLY_PER_CHANNEL = (0.5, 1.5), 0.5
GRAY_ALPHA = (0.0, 1.0)


def gaussian_weights(sigma: float) -> np.ndarray:
    """float64 ``[radius + 1]``: ``w[d] = exp(-d^2 / (2 sigma^2)) / sum over -radius..radius``, radius ``int(4 sigma + 0.5)``
    (scipy's ``truncate=4.0``); ``w[0]`` is the centre"""
    radius = int(4.0 * float(sigma) + 0.5)
    if radius == 0:
        return np.ones(1, dtype=np.float64)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def sharpen_weights(alpha: float, lightness: float) -> np.ndarray:
    """float64 ``[3,3]``: ``(1 - a) I + a [[-1,-1,-1],[-1,8+l,-1],[-1,-1,-1]]`` (imgaug's Sharpen)"""
    ident = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float64)
    eff = np.array([[-1, -1, -1], [-1, 8 + float(lightness), -1], [-1, -1, -1]], dtype=np.float64)
    return (1.0 - float(alpha)) * ident + float(alpha) * eff


def emboss_weights(alpha: float, strength: float) -> np.ndarray:
    """float64 ``[3,3]``: ``(1 - a) I + a [[-1-s,-s,0],[-s,1,s],[0,s,1+s]]`` (imgaug's Emboss)"""
    s = float(strength)
    ident = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float64)
    eff = np.array([[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]], dtype=np.float64)
    return (1.0 - float(alpha)) * ident + float(alpha) * eff


def dropout_threshold(p: float) -> int:
    """``floor(p 2^32)``, at most ``2^32 - 1``: an element is dropped iff its 32-bit draw is below it"""
    return min(int(np.floor(float(p) * 4294967296.0)), 4294967295)


def coarse_grid(size_percent: float, h: int, w: int):
    return max(1, int(np.floor(h * float(size_percent) + 0.5))), max(1, int(np.floor(w * float(size_percent) + 0.5)))


@dataclass
class PhotoProgram(SlotProgram):
    """``opcode`` int32 ``[B,S]``, ``iarg`` int32 ``[B,S,4]``, ``farg`` float64 ``[B,S,16]``, ``seed`` uint64 ``[B,S]`` (numpy,
    on the host; the module docstring says what each opcode reads).  The ``set_*`` methods encode one slot."""
    opcode: np.ndarray
    iarg: np.ndarray
    farg: np.ndarray
    seed: np.ndarray
    COLUMNS = (("iarg", np.int32, IARGS), ("farg", np.float64, FARGS))
    SLOTS = PRESET_SLOTS

    def set_gaussian_blur(self, i, s, sigma):
        wts = gaussian_weights(sigma)
        self._clear(i, s, OP_GAUSSIAN_BLUR if len(wts) > 1 else OP_NOP)
        if len(wts) > 1:
            self.iarg[i, s, 0] = len(wts) - 1
            self.farg[i, s, :len(wts)] = wts
            self.farg[i, s, 15] = sigma

    def set_average_blur(self, i, s, k):
        self._clear(i, s, OP_AVERAGE_BLUR)
        self.iarg[i, s, 0] = k

    def set_median_blur(self, i, s, k):
        self._clear(i, s, OP_MEDIAN_BLUR)
        self.iarg[i, s, 0] = k

    def set_conv3x3(self, i, s, weights):
        self._clear(i, s, OP_CONV3X3)
        self.farg[i, s, :9] = np.asarray(weights, dtype=np.float64).reshape(9)

    def set_gaussian_noise(self, i, s, scale, per_channel, seed):
        self._clear(i, s, OP_GAUSSIAN_NOISE)
        self.farg[i, s, 0] = scale
        self.iarg[i, s, 0] = int(bool(per_channel))
        self.seed[i, s] = seed

    def set_dropout(self, i, s, p, per_channel, seed):
        self._clear(i, s, OP_DROPOUT)
        self.farg[i, s, 0] = p
        self.iarg[i, s, 0] = int(bool(per_channel))
        self.seed[i, s] = seed

    def set_coarse_dropout(self, i, s, p, size_percent, per_channel, seed):
        self._clear(i, s, OP_COARSE_DROPOUT)
        self.farg[i, s, 0] = p
        self.farg[i, s, 1] = size_percent
        self.iarg[i, s, 0] = int(bool(per_channel))
        self.seed[i, s] = seed

    def set_invert(self, i, s, channels):
        self._clear(i, s, OP_INVERT)
        self.iarg[i, s, 0] = sum(1 << ch for ch, on in enumerate(channels) if on)

    def set_add(self, i, s, values):
        self._clear(i, s, OP_ADD)
        v = np.broadcast_to(np.asarray(values, dtype=np.int64), (IARGS,)) if np.ndim(values) == 0 else np.asarray(values)
        self.iarg[i, s, :len(v)] = v

    def set_multiply(self, i, s, factors):
        self._clear(i, s, OP_MULTIPLY)
        self.farg[i, s, :IARGS] = 1.0
        f = np.broadcast_to(np.asarray(factors, dtype=np.float64), (IARGS,)) if np.ndim(factors) == 0 else np.asarray(factors)
        self.farg[i, s, :len(f)] = f

    def set_grayscale(self, i, s, alpha):
        self._clear(i, s, OP_GRAYSCALE)
        self.farg[i, s, 0] = alpha

    def validate(self, channels: Optional[int] = None) -> None:
        """Raises ``ValueError`` for a program the kernels are not defined on: shapes and dtypes, unknown opcodes, a
        radius outside 1..12 or weights that are not ``gaussian_weights(sigma)``'s shape (finite, summing to 1), k outside
        2..7, an even k or one outside 3..11, non-finite weights, a scale outside [0, 255], p or size_percent outside
        [0, 1], an invert mask outside 0..15, an addend outside [-255, 255], a factor outside [0, 255], alpha outside
        [0, 1], and -- when ``channels`` is given -- more than 4 channels or a grayscale slot on C other than 1 or 3."""
        self._check_arrays(OP_GRAYSCALE)
        op, ia, fa = self.opcode, self.iarg, self.farg
        if channels is not None and not 1 <= channels <= 4:
            raise ValueError("PhotoProgram: 1..4 channels, got %d" % channels)

        def sel(code):
            m = op == code
            return ia[m], fa[m]
        i, f = sel(OP_GAUSSIAN_BLUR)
        if len(i):
            if np.any((i[:, 0] < 1) | (i[:, 0] > 12)):
                raise ValueError("PhotoProgram: GAUSSIAN_BLUR radius must be in 1..12 (sigma in [0.125, 3])")
            live = np.arange(13)[None, :] <= i[:, 0:1]
            wsum = f[:, 0] + 2.0 * np.where(live[:, 1:], f[:, 1:13], 0.0).sum(1)
            if np.any(f[:, :13][live] < 0) or np.any(np.abs(wsum - 1.0) > 1e-12):
                raise ValueError("PhotoProgram: GAUSSIAN_BLUR weights must be non-negative and sum to 1")
        i, f = sel(OP_AVERAGE_BLUR)
        if np.any((i[:, 0] < 2) | (i[:, 0] > 7)):
            raise ValueError("PhotoProgram: AVERAGE_BLUR k must be in 2..7")
        i, f = sel(OP_MEDIAN_BLUR)
        if np.any((i[:, 0] < 3) | (i[:, 0] > 11) | (i[:, 0] % 2 == 0)):
            raise ValueError("PhotoProgram: MEDIAN_BLUR k must be odd and in 3..11")
        i, f = sel(OP_GAUSSIAN_NOISE)
        if np.any((f[:, 0] < 0) | (f[:, 0] > 255)):
            raise ValueError("PhotoProgram: GAUSSIAN_NOISE scale must be in [0, 255]")
        for code in (OP_GAUSSIAN_NOISE, OP_DROPOUT, OP_COARSE_DROPOUT):
            i, f = sel(code)
            if np.any((i[:, 0] != 0) & (i[:, 0] != 1)):
                raise ValueError("PhotoProgram: %s per_channel must be 0 or 1" % OP_NAMES[code])
        for code in (OP_DROPOUT, OP_COARSE_DROPOUT):
            i, f = sel(code)
            if np.any((f[:, 0] < 0) | (f[:, 0] > 1)):
                raise ValueError("PhotoProgram: %s p must be in [0, 1]" % OP_NAMES[code])
        i, f = sel(OP_COARSE_DROPOUT)
        if np.any((f[:, 1] <= 0) | (f[:, 1] > 1)):
            raise ValueError("PhotoProgram: COARSE_DROPOUT size_percent must be in (0, 1]")
        i, f = sel(OP_INVERT)
        if np.any((i[:, 0] < 0) | (i[:, 0] > 15)):
            raise ValueError("PhotoProgram: INVERT channel mask must be in 0..15")
        i, f = sel(OP_ADD)
        if np.any(np.abs(i) > 255):
            raise ValueError("PhotoProgram: ADD values must be in [-255, 255]")
        i, f = sel(OP_MULTIPLY)
        if np.any((f[:, :IARGS] < 0) | (f[:, :IARGS] > 255)):
            raise ValueError("PhotoProgram: MULTIPLY factors must be in [0, 255]")
        i, f = sel(OP_GRAYSCALE)
        if len(i):
            if np.any((f[:, 0] < 0) | (f[:, 0] > 1)):
                raise ValueError("PhotoProgram: GRAYSCALE alpha must be in [0, 1]")
            if channels is not None and channels not in (1, 3):
                raise ValueError("PhotoProgram: GRAYSCALE takes 3 channels (1 channel: a copy), got %d" % channels)

    def kernel_arrays(self, h: int, w: int, channels: Optional[int] = None):
        """(opcode, iarg, farg, seed as int64 bits) as the kernel takes them: validated, with the dropout thresholds in
        ``iarg[1]`` and the coarse grids of an ``h x w`` image in ``iarg[2:4]``"""
        self.validate(channels)
        ia = self.iarg.copy()
        for code in (OP_DROPOUT, OP_COARSE_DROPOUT):
            for i, s in zip(*np.nonzero(self.opcode == code)):
                ia[i, s, 1] = np.array(dropout_threshold(self.farg[i, s, 0]), dtype=np.uint32).view(np.int32)   # (the bits)
                if code == OP_COARSE_DROPOUT:
                    ia[i, s, 2:4] = coarse_grid(self.farg[i, s, 1], h, w)
        return self.opcode, ia, self.farg, self.seed.view(np.int64)

    def apply(self, images, masks):
        return photometric_aug(images, self), masks


def draw_photo(b: int, rng: np.random.Generator, seed_shape):
    """the parameters of the nine entries for every sample of a batch, and ``seed_shape`` seeds drawn last"""
    u = lambda lo_hi, *shape: rng.uniform(lo_hi[0], lo_hi[1], (b,) + shape)
    return dict(
        blur_kind=rng.integers(0, 3, b), sigma=u(SIGMA), avg_k=rng.integers(AVERAGE_K[0], AVERAGE_K[1] + 1, b),
        med_k=2 * rng.integers(MEDIAN_K[0] // 2, MEDIAN_K[1] // 2 + 1, b) + 1,
        sh_a=u(SHARPEN_ALPHA), sh_l=u(SHARPEN_LIGHTNESS), em_a=u(EMBOSS_ALPHA), em_s=u(EMBOSS_STRENGTH),
        no_s=u(NOISE_SCALE), no_pc=rng.random(b) < NOISE_PER_CHANNEL,
        dr_kind=rng.integers(0, 2, b), dr_p=u(DROPOUT_P), dr_pc=rng.random(b) < DROPOUT_PER_CHANNEL,
        co_p=u(COARSE_P), co_s=u(COARSE_SIZE), co_pc=rng.random(b) < COARSE_PER_CHANNEL,
        inv=rng.random((b, IARGS)) < INVERT_P,
        add_pc=rng.random(b) < ADD_PER_CHANNEL, add_v=rng.integers(ADD[0], ADD[1] + 1, (b, IARGS)),
        mul_pc=rng.random(b) < MULTIPLY_PER_CHANNEL, mul_v=u(MULTIPLY, IARGS), gray=u(GRAY_ALPHA),
        seed=rng.integers(0, 2 ** 64, seed_shape, dtype=np.uint64))


def encode_photo(prog: PhotoProgram, i: int, s: int, entry: int, d, seed) -> None:
    """entry ``entry`` of sample ``i`` into slot ``s`` from ``draw_photo``'s ``d``; ``seed`` keys the entry if it is a random one"""
    if entry == ENTRY_BLUR:
        if d["blur_kind"][i] == 0:
            prog.set_gaussian_blur(i, s, d["sigma"][i])
        elif d["blur_kind"][i] == 1:
            prog.set_average_blur(i, s, d["avg_k"][i])
        else:
            prog.set_median_blur(i, s, d["med_k"][i])
    elif entry == ENTRY_SHARPEN:
        prog.set_conv3x3(i, s, sharpen_weights(d["sh_a"][i], d["sh_l"][i]))
    elif entry == ENTRY_EMBOSS:
        prog.set_conv3x3(i, s, emboss_weights(d["em_a"][i], d["em_s"][i]))
    elif entry == ENTRY_NOISE:
        prog.set_gaussian_noise(i, s, d["no_s"][i], d["no_pc"][i], seed)
    elif entry == ENTRY_DROPOUT:
        if d["dr_kind"][i] == 0:
            prog.set_dropout(i, s, d["dr_p"][i], d["dr_pc"][i], seed)
        else:
            prog.set_coarse_dropout(i, s, d["co_p"][i], d["co_s"][i], d["co_pc"][i], seed)
    elif entry == ENTRY_INVERT:
        prog.set_invert(i, s, d["inv"][i])
    elif entry == ENTRY_ADD:
        prog.set_add(i, s, d["add_v"][i] if d["add_pc"][i] else d["add_v"][i, 0])
    elif entry == ENTRY_MULTIPLY:
        prog.set_multiply(i, s, d["mul_v"][i] if d["mul_pc"][i] else d["mul_v"][i, 0])
    else:
        prog.set_grayscale(i, s, d["gray"][i])


def sample_program(batch: int, preset: str, rng: np.random.Generator) -> PhotoProgram:
    """Draw the program of one batch.  ``preset``: ``"mscmrseg_aug2_photometric"``, the ``SomeOf((0, 5), ..,
    random_order=True)`` of ``data_generator_mscmrseg.py:96-127`` over the nine entries that are built: per sample a uniform
    count 0..5 of distinct entries out of {blur OneOf(Gaussian sigma 0-3 | average k 2-7 | median odd k 3-11), sharpen
    (alpha 0-1, lightness 0.75-1.5), emboss (alpha 0-1, strength 0-2), Gaussian noise (scale 0-0.05*255, per_channel 0.5),
    dropout OneOf(p 0.01-0.1, per_channel 0.5 | coarse p 0.03-0.15, size 0.02-0.05, per_channel 0.2), invert (p = 0.05 per
    channel), add (-10..10, per_channel 0.5), multiply (0.5-1.5, per_channel 0.5), grayscale (alpha 0-1)}, applied in one
    random order per batch (as ``sample_params``), 5 slots, seeds drawn from ``rng``.

    Absent from the reference's list: ``Superpixels``, ``SimplexNoiseAlpha(EdgeDetect | DirectedEdgeDetect)`` and
    ``AddToHueAndSaturation`` (``utils/stylize.py``; the preset ``"mscmrseg_aug2_full_device"`` of ``sample_heavy_plan`` holds all
    twelve); so is the ``CropAndPad`` in front of it.  imgaug's own parameter stream is not reproduced
    (parity unpinned)."""
    if preset == "heavy":
        raise NotImplementedError(HEAVY_MESSAGE)
    if preset != PHOTOMETRIC_PRESET:
        raise ValueError("unknown photometric preset %r (have: %s)" % (preset, PHOTOMETRIC_PRESET))
    b = batch
    order = rng.permutation(9)
    count = rng.integers(0, 6, b)
    rank = np.argsort(np.argsort(rng.random((b, 9)), axis=1), axis=1)
    chosen = rank < count[:, None]                                    # [B,9]: `count` distinct entries per sample
    d = draw_photo(b, rng, (b, PRESET_SLOTS))
    prog = PhotoProgram.identity(b, PRESET_SLOTS)
    order, seeds = order.tolist(), d["seed"]                          # (plain ints: the entry is compared up to eight times)
    for i, row in enumerate(chosen[:, order].tolist()):
        s = 0
        for entry, on in zip(order, row):
            if on:
                encode_photo(prog, i, s, entry, d, seeds[i, s])
                s += 1
    return prog


def upload_program(program: PhotoProgram, batch: int, h: int, w: int, channels: int, device: torch.device):
    """Validate on the host, then move the kernel's arrays through pinned, non-blocking copies (no synchronisation)."""
    return upload(program, batch, h, w, channels, device=device)


def photometric_aug(images: torch.Tensor, program: Optional[PhotoProgram] = None) -> torch.Tensor:
    """The photometric part of ``data_generator_mscmrseg.py:87-132``: uint8 ``[B,H,W,C]`` images on the device -> the
    augmented uint8 images (a new tensor).  ``program`` is required: draw it with
    ``sample_program(B, "mscmrseg_aug2_photometric", rng)``."""
    if program is None:
        raise TypeError("photometric_aug: program is required (sample_program(batch, preset, rng)); there is no silent identity")
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise TypeError("photometric_aug: uint8 [B,H,W,C] images")
    b, h, w, c = images.shape
    return K.photometric(images, *upload_program(program, b, h, w, c, images.device))
