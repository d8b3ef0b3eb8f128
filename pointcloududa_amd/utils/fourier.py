"""Device-side Fourier domain adaptation for the loader path.

``HistReferenceBank`` (f10b) aligns first-order intensity statistics of a source image with a target image.  The other
standard image-level alignment of unsupervised domain adaptation is Fourier domain adaptation (FDA): the low-frequency block of
the source image's amplitude spectrum is replaced by the target image's, the source phase is kept.  Here the targets live in a
``FourierBank`` on the device (per plane the float64 amplitudes of the block, built there) and ``fourier_adapt`` adapts every
sample of a batch to the reference its index names (``csrc/fourier.hip``: a partial DFT over the block's bins, no full FFT,
any size).

The rule is this build's own statement of FDA, written with numpy's FFT (``tests/fourier_refs.py``).  Per plane
``(sample, channel)`` of a source ``s[H, W]`` and the same channel of a target ``t[H, W]`` of the SAME size, in float64::

    S, T = np.fft.fft2(s), np.fft.fft2(t)
    # the block: frequencies -b..b on both axes = rows / columns H//2-b .. H//2+b (W likewise) of the fftshift-ed arrays
    S'[k] = |T[k]| * exp(1j * angle(S[k]))      inside the block (angle(0) = 0),        S'[k] = S[k] outside
    v = real(ifft2(S'))

fp32 images store ``float32(v)`` (nearest even; ``clip=(lo, hi)`` clips first, nothing is clipped otherwise), uint8 images store
``uint8(clip(rint(v), 0, 255))`` with ``rint`` rounding half to even.  ``b`` is an integer radius with ``2 b + 1 <= min(H, W)``
(beyond that the bins alias: rejected) and ``b <= 32``; ``fourier_radius(H, W, beta) = floor(min(H, W) * beta)``.

Unpinned: the public FDA code is not vendored by the reference, so parity with it -- its ``beta``-to-``b`` convention, its torch
variant -- is not claimed.  A bin whose ``|S[k]|`` is rounding noise (an image that is constant along one axis) has an arbitrary
phase in numpy and here alike; no floor is added.  NaN and inf are unsupported.  Not here: a general FFT, gradients through
the stage, references of another size than the images, phase or amplitude mixing other than the block swap, float64 / int16
images, a check of device-side indices."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .. import kernels as K
from ._program import to_device

MAX_RADIUS = 32
MAX_SIDE = 4096


def fourier_radius(h: int, w: int, beta: float) -> int:
    """``floor(min(h, w) * beta)``: the block radius of a ``beta`` in [0, 0.5) (this build's convention)"""
    h, w, beta = int(h), int(w), float(beta)
    if h < 1 or w < 1:
        raise ValueError("fourier_radius: sides of at least 1, got %d x %d" % (h, w))
    if not 0.0 <= beta < 0.5:
        raise ValueError("fourier_radius: beta in [0, 0.5), got %r" % (beta,))
    return int(math.floor(min(h, w) * beta))


def check_radius(who: str, radius, h: int, w: int) -> int:
    """an integer block radius that fits ``h x w`` images; raises ``ValueError`` otherwise"""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise TypeError("%s: radius is an integer, got %r" % (who, radius))
    radius = int(radius)
    if radius < 0 or radius > MAX_RADIUS:
        raise ValueError("%s: radius in [0, %d], got %d" % (who, MAX_RADIUS, radius))
    if 2 * radius + 1 > min(h, w):
        raise ValueError("%s: the block of radius %d (2 radius + 1 = %d bins a side) does not fit %d x %d images: its bins "
                         "would alias" % (who, radius, 2 * radius + 1, h, w))
    return radius


def validate_index(index, batch: int, size: int) -> np.ndarray:
    """a host ``index`` (sequence or numpy array of integers) as int32 ``[batch]``: ``histmatch.validate_index``'s rules with
    ``-1`` allowed (the sample passes through); raises unless it holds ``batch`` entries in ``[-1, size)``"""
    arr = np.asarray(index.cpu() if torch.is_tensor(index) else index)
    if arr.dtype.kind not in "iu":
        raise TypeError("fourier_adapt: index holds integers, got %s" % (arr.dtype,))
    if arr.shape != (batch,):
        raise ValueError("fourier_adapt: index must hold one entry per sample (%d), got shape %r" % (batch, arr.shape))
    if arr.size and (arr.min() < -1 or arr.max() >= size):
        raise ValueError("fourier_adapt: index entries must lie in [-1, %d) (-1 passes the sample through), got %d .. %d"
                         % (size, arr.min(), arr.max()))
    return np.ascontiguousarray(arr.astype(np.int32))


def validate_radius(radius, batch: int, bank_radius: int) -> np.ndarray:
    """host per-sample radii as int32 ``[batch]``; raises unless it holds ``batch`` non-negative integers (values above the
    bank's radius are clamped on the device)"""
    arr = np.asarray(radius.cpu() if torch.is_tensor(radius) else radius)
    if arr.dtype.kind not in "iu":
        raise TypeError("fourier_adapt: radius holds integers, got %s" % (arr.dtype,))
    if arr.shape != (batch,):
        raise ValueError("fourier_adapt: radius must hold one entry per sample (%d), got shape %r" % (batch, arr.shape))
    if arr.size and arr.min() < 0:
        raise ValueError("fourier_adapt: radii are non-negative, got %d" % arr.min())
    return np.ascontiguousarray(np.minimum(arr, bank_radius).astype(np.int32))


def _as_set(who, references):
    """the references as a 4-d fp32 / uint8 tensor or numpy array (one [H,W,C] image becomes a set of one)"""
    if not torch.is_tensor(references):
        references = np.asarray(references)
    if references.dtype not in (torch.float32, torch.uint8, np.float32, np.uint8):
        raise TypeError("%s: fp32 or uint8 references, got %s" % (who, references.dtype))
    if references.ndim not in (3, 4):
        raise ValueError("%s: [R,H,W,C] references (or one [H,W,C]), got %d dimensions" % (who, references.ndim))
    return references if references.ndim == 4 else references[None]


class FourierBank:
    """``R`` target images kept on ``device`` as what ``fourier_adapt`` reads: per plane ``(r, c)`` the float64 amplitudes
    ``|T[ky, kx]|`` of the low-frequency block, ``ky = -radius..radius``, ``kx = 0..radius`` (half of the block: the images are
    real), built on the device (``csrc/fourier.hip``).  ``references``: fp32 or uint8 ``[R,H,W,C]`` (or one ``[H,W,C]``), a
    device tensor or a numpy array (uploaded as it lies through a pinned non-blocking copy).  ``radius`` is the block radius
    ``b``; ``None`` takes ``fourier_radius(H, W, beta)``.

    ``size`` = R, ``radius`` = b, ``shape`` = ``(R, H, W, C)``, ``dtype`` the references' numpy dtype (images adapted against
    the bank must have it).  ``rebuild(references)`` refills the same storage from a same-shaped set of the same dtype without
    allocation (for a device tensor) or synchronisation: how a trainer makes this step's target batch the bank."""

    def __init__(self, references, device=None, beta: float = 0.01, radius: Optional[int] = None):
        refs = _as_set("FourierBank", references)
        if torch.is_tensor(refs):
            if device is not None and torch.device(device) != refs.device:
                raise ValueError("FourierBank: the references are on %s, not on %s" % (refs.device, torch.device(device)))
            self.device = refs.device
        else:
            self.device = torch.device("cuda" if device is None else device)
        self.shape = tuple(int(v) for v in refs.shape)
        self.size, self.channels = self.shape[0], self.shape[3]
        self.dtype = np.dtype(np.uint8 if refs.dtype in (torch.uint8, np.uint8) else np.float32)
        if not 1 <= self.channels <= 4 or min(self.shape) < 1:
            raise ValueError("FourierBank: a non-empty [R,H,W,C] set with 1..4 channels, got %r" % (self.shape,))
        h, w = self.shape[1], self.shape[2]
        if max(h, w) > MAX_SIDE:
            raise ValueError("FourierBank: sides up to %d, got %d x %d" % (MAX_SIDE, h, w))
        self.radius = check_radius("FourierBank", fourier_radius(h, w, beta) if radius is None else radius, h, w)
        self._staged = None                     # device copy of host references (numpy input only)
        self._index_cache = {}
        self.bank, self._workspace = K.fourier_bank_storage(*self.shape, self.radius, self.device)
        self.rebuild(refs)

    def rebuild(self, references) -> "FourierBank":
        refs = _as_set("FourierBank.rebuild", references)
        dtype = np.dtype(np.uint8 if refs.dtype in (torch.uint8, np.uint8) else np.float32)
        if tuple(int(v) for v in refs.shape) != self.shape or dtype != self.dtype:
            raise ValueError("FourierBank.rebuild: %s references of shape %r, got %s %r"
                             % (self.dtype, self.shape, dtype, tuple(refs.shape)))
        if torch.is_tensor(refs):
            if refs.device != self.device:
                raise ValueError("FourierBank.rebuild: the references are on %s, the bank on %s" % (refs.device, self.device))
            refs = refs.contiguous()
        else:
            host = torch.from_numpy(np.ascontiguousarray(refs))
            if self._staged is None:
                self._staged = torch.empty(self.shape, dtype=host.dtype, device=self.device)
            self._staged.copy_(host.pin_memory() if self.device.type == "cuda" else host, non_blocking=True)
            refs = self._staged
        K.fourier_bank_build(refs, self.radius, self.bank, self._workspace)
        return self

    def index_tensor(self, index, batch: int) -> torch.Tensor:
        """the int32 ``[batch]`` device tensor of a ``fourier_adapt`` ``index`` argument (see there)"""
        if torch.is_tensor(index) and index.is_cuda:
            if index.dtype != torch.int32 or tuple(index.shape) != (batch,):
                raise TypeError("fourier_adapt: a device index is an int32 [%d] tensor, got %s %r"
                                % (batch, index.dtype, tuple(index.shape)))
            return index.contiguous()                                       # (entries are clamped on the device, not checked)
        if index is None:
            if self.size not in (1, batch):
                raise ValueError("fourier_adapt: index=None needs as many references as samples (%d references, %d samples) "
                                 "or a bank of one" % (self.size, batch))
            if batch not in self._index_cache:
                self._index_cache[batch] = (torch.arange(batch, dtype=torch.int32, device=self.device) if self.size == batch
                                            else torch.zeros(batch, dtype=torch.int32, device=self.device))
            return self._index_cache[batch]
        return to_device((validate_index(index, batch, self.size),), self.device)[0]

    def radius_tensor(self, radius, batch: int) -> Optional[torch.Tensor]:
        """the int32 ``[batch]`` device tensor of a ``fourier_adapt`` ``radius`` argument, or ``None`` for the bank's radius"""
        if radius is None:
            return None
        if torch.is_tensor(radius) and radius.is_cuda:
            if radius.dtype != torch.int32 or tuple(radius.shape) != (batch,):
                raise TypeError("fourier_adapt: a device radius is an int32 [%d] tensor, got %s %r"
                                % (batch, radius.dtype, tuple(radius.shape)))
            return radius.contiguous()                                      # (entries are clamped on the device, not checked)
        if isinstance(radius, (int, np.integer)) and not isinstance(radius, bool):
            if int(radius) >= self.radius:                                  # (clamped: the bank's radius)
                return None
            radius = np.full(batch, int(radius), dtype=np.int64)
        return to_device((validate_radius(radius, batch, self.radius),), self.device)[0]


def check_images(images, bank) -> None:
    """the host-side checks of ``fourier_adapt``'s images against its bank (reads ``bank.shape`` and ``bank.dtype`` only)"""
    if not torch.is_tensor(images) or images.dtype not in (torch.float32, torch.uint8):
        raise TypeError("fourier_adapt: fp32 or uint8 device tensors, got %s" % (getattr(images, "dtype", type(images)),))
    if images.dim() not in (3, 4):
        raise ValueError("fourier_adapt: [B,H,W,C] or [H,W,C] images, got %d dimensions" % images.dim())
    if (images.dtype == torch.uint8) != (bank.dtype == np.uint8):
        raise TypeError("fourier_adapt: %s images against a bank of %s references: the dtypes must match"
                        % (str(images.dtype).replace("torch.", ""), bank.dtype))
    if tuple(int(v) for v in images.shape[-3:]) != tuple(bank.shape[1:]):
        raise ValueError("fourier_adapt: images of size %r against references of size %r: H, W and C must match"
                         % (tuple(images.shape[-3:]), tuple(bank.shape[1:])))


def check_clip(images, clip):
    if clip is None:
        return None
    if images.dtype != torch.float32:
        raise TypeError("fourier_adapt: clip goes with fp32 images (uint8 images are always clipped to 0..255)")
    try:
        lo, hi = (float(v) for v in clip)
    except (TypeError, ValueError):
        raise ValueError("fourier_adapt: clip = (lo, hi), got %r" % (clip,)) from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("fourier_adapt: clip = (lo, hi) with finite lo <= hi, got %r" % (clip,))
    return lo, hi


def fourier_adapt(images: torch.Tensor, bank: FourierBank, index=None, radius=None, clip=None, out=None) -> torch.Tensor:
    """Fourier domain adaptation on the device: ``[B,H,W,C]`` images (or one ``[H,W,C]``), fp32 or uint8, of the bank's
    references' size and dtype -> a new tensor of the same shape and dtype (``out=`` for a ``[B,H,W,C]`` batch).  Sample ``i`` gets
    the low-frequency amplitudes of reference ``index[i]`` and keeps its own phase (the module's rule).

    ``index``: a host sequence or numpy array of ``B`` integers in ``[-1, R)`` (validated here, uploaded through a pinned
    non-blocking copy), or an int32 ``[B]`` device tensor (NOT checked: the kernel clamps entries ``>= R``), or ``None``, which
    needs ``R == B`` (sample ``i`` takes reference ``i``) or ``R == 1``.  A NEGATIVE entry passes its sample through bit for bit.
    ``radius``: ``None`` (the bank's), an int, a host sequence of ``B`` non-negative integers or an int32 ``[B]`` device tensor;
    per sample it is clamped into ``[0, bank.radius]``; 0 swaps the DC bin only (every pixel of a plane moves by the same
    amount).  ``clip = (lo, hi)``: fp32 results are clipped before the store; without it nothing is clipped."""
    if not isinstance(bank, FourierBank):
        raise TypeError("fourier_adapt: bank is a FourierBank (FourierBank(references, device, beta=.. or radius=..))")
    check_images(images, bank)
    clip = check_clip(images, clip)
    batch = images if images.dim() == 4 else images[None]
    b = int(batch.shape[0])
    idx = bank.index_tensor(index, b)
    rad = bank.radius_tensor(radius, b)
    if images.dim() == 3 and out is not None:
        out = out[None]
    res = K.fourier_adapt(batch, bank.bank, bank.size, bank.radius, idx, rad, clip, out=out)
    return res if images.dim() == 4 else res[0]
