"""Device-side histogram matching for the loader path.

The first thing the reference's MM-WHS generator does to every image after the file read, when ``train_mmwhs.py -mh`` is
given (``src/data_generator_mmwhs.py:174-176, 236-237``), is ``match_histograms(img, self._reference_img,
multichannel=True)``: per channel, every value is replaced by the value of the reference image at the same quantile.  It runs
in front of the batch-global min-max, so it changes ``img_min`` / ``img_max`` and everything behind them.  Here the reference
image -- fixed for a whole run -- is sorted once on the host (``reference_tables``) and uploaded (``HistReference``); the
per-batch work is one HIP entry point (``csrc/histmatch.hip``): fp32 images sort each plane's keys on the device and rank
every value by binary search, uint8 images take a 256-bin histogram and a LUT.

The definition is ``skimage.exposure.match_histograms`` of the reference's era (0.16-0.18) restated in plain numpy
(``scripts/make_match_hist_golden.py``, pinned by ``tests/golden/match_hist.npz``), per channel::

    sv, inv, sc = np.unique(s.ravel(), return_inverse=True, return_counts=True)
    tv, tc      = np.unique(t.ravel(), return_counts=True)
    out         = np.interp(np.cumsum(sc) / N, np.cumsum(tc) / M, tv)[inv]      # float64, then cast to the image's dtype

and the device result equals it bit for bit: fp32 images round the float64 result to nearest even, uint8 images truncate
it (numpy's assignment).  NaN in an image is unsupported (the reference's result is garbage there too); a non-finite
reference is refused.

A reference per sample (a source image against a target image drawn from a pool, or against this step's target batch) is
``HistReferenceBank`` / ``match_histograms(images, bank, index=..)`` (``csrc/histmatch_bank.hip``):
the references stay on the device, an fp32 reference plane is sorted there and the sorted plane IS the table (``tv`` its run
ends' values, ``cumsum(tc)`` its run ends), a uint8 plane is 256 counts; same definition, same bits.  A reference's ``-0.0``
is read as ``+0.0`` there.  Not here: other dtypes (int16, float64), ``multichannel=False``, a check of device-side indices."""
from __future__ import annotations

from typing import Tuple, Union

import numpy as np
import torch

from .. import kernels as K
from ._program import to_device


def reference_tables(reference_hwc: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``[H,W,C]`` reference image -> ``(values [C,Nmax] float64, quantiles [C,Nmax] float64, lengths [C] int32)``: per channel
    the sorted distinct values and ``cumsum(counts) / (H W)``; rows shorter than the longest repeat their last entry."""
    ref = np.asarray(reference_hwc)
    if ref.ndim != 3:
        raise ValueError("reference_tables: an [H,W,C] reference image, got %d dimensions" % ref.ndim)
    if ref.size == 0:
        raise ValueError("reference_tables: the reference image is empty")
    if ref.dtype.kind not in "fiub" or not np.all(np.isfinite(ref)):
        raise ValueError("reference_tables: the reference image must be real and finite")
    c = ref.shape[2]
    m = ref.shape[0] * ref.shape[1]
    rows = []
    for ch in range(c):
        tv, tc = np.unique(ref[..., ch].ravel(), return_counts=True)
        rows.append((tv.astype(np.float64), np.cumsum(tc) / m))
    lengths = np.array([len(tv) for tv, _ in rows], dtype=np.int32)
    nmax = int(lengths.max())
    values = np.empty((c, nmax), dtype=np.float64)
    quantiles = np.empty((c, nmax), dtype=np.float64)
    for ch, (tv, tq) in enumerate(rows):
        values[ch, :len(tv)], values[ch, len(tv):] = tv, tv[-1]
        quantiles[ch, :len(tq)], quantiles[ch, len(tq):] = tq, tq[-1]
    return values, quantiles, lengths


class HistReference:
    """The tables of one reference image on ``device`` (uploaded once, through pinned non-blocking copies): ``values``,
    ``quantiles`` float64 ``[C,Nmax]``, ``lengths`` int32 ``[C]``; ``dtype`` is the reference image's numpy dtype and
    ``channels`` its channel count."""

    def __init__(self, reference_hwc: np.ndarray, device):
        ref = np.asarray(reference_hwc)
        tables = reference_tables(ref)
        self.dtype = ref.dtype
        self.channels = int(ref.shape[2])
        self.device = torch.device(device)
        self.values, self.quantiles, self.lengths = to_device(tables, self.device)


class HistReferenceBank:
    """``R`` reference images kept on ``device`` in the form the match reads directly (``csrc/histmatch_bank.hip``), built on the
    device: no host sort, no table upload.  ``references``: fp32 or uint8 ``[R,H,W,C]`` (or one ``[H,W,C]``), a device tensor or
    a numpy array (uploaded as it lies through a pinned non-blocking copy).  An fp32 bank holds every plane's sorted keys (4
    bytes per reference value, next to a build workspace of the same size that the object keeps so that a rebuild allocates
    nothing); a uint8 bank holds 256 counts per plane.  ``float_images=True`` makes a uint8 bank also keep the sorted-key form
    of its references, which fp32 images need (uint8 images always take the counts).

    ``size`` = R, ``channels`` = C, ``dtype`` the references' numpy dtype, ``shape`` = ``(R, H, W, C)``.  A reference's ``-0.0``
    is read as ``+0.0`` (the keys canonicalise it; ``np.unique`` keeps whichever zero comes first -- the two compare equal).
    Non-finite reference values are unsupported: the build leaves a flag on the device, ``check=True`` reads it (ONE host
    synchronisation) and raises as ``reference_tables`` does; the default never synchronises.

    ``rebuild(references)`` refills the same storage from a same-shaped set of the same dtype without allocation (for a device
    tensor) or synchronisation: how a trainer makes this step's target batch the bank."""

    def __init__(self, references, device=None, check: bool = False, float_images: bool = False):
        refs = self._as_set(references)
        if torch.is_tensor(refs):
            if device is not None and torch.device(device) != refs.device:
                raise ValueError("HistReferenceBank: the references are on %s, not on %s" % (refs.device, torch.device(device)))
            self.device = refs.device
        else:
            self.device = torch.device("cuda" if device is None else device)
        self.shape = tuple(int(v) for v in refs.shape)
        self.size, self.channels = self.shape[0], self.shape[3]
        self.dtype = np.dtype(np.uint8 if refs.dtype in (torch.uint8, np.uint8) else np.float32)
        if not 1 <= self.channels <= 4 or min(self.shape) < 1:
            raise ValueError("HistReferenceBank: a non-empty [R,H,W,C] set with 1..4 channels, got %r" % (self.shape,))
        self._staged = None                     # device copy of host references (numpy input only)
        self._index_cache = {}
        is_u8 = self.dtype == np.uint8
        self.bank, self._workspace, self.flag = K.hist_bank_storage(*self.shape, is_u8, self.device)
        self._float_refs = self.float_bank = self._float_workspace = self._float_flag = None
        if is_u8 and float_images:
            self._float_refs = torch.empty(self.shape, dtype=torch.float32, device=self.device)
            self.float_bank, self._float_workspace, self._float_flag = K.hist_bank_storage(*self.shape, False, self.device)
        self.rebuild(refs, check=check)

    @staticmethod
    def _as_set(references):
        """the references as a 4-d fp32 / uint8 tensor or numpy array (one [H,W,C] image becomes a set of one)"""
        if not torch.is_tensor(references):
            references = np.asarray(references)
        if references.dtype not in (torch.float32, torch.uint8, np.float32, np.uint8):
            raise TypeError("HistReferenceBank: fp32 or uint8 references, got %s" % (references.dtype,))
        if references.ndim not in (3, 4):
            raise ValueError("HistReferenceBank: [R,H,W,C] references (or one [H,W,C]), got %d dimensions" % references.ndim)
        return references if references.ndim == 4 else references[None]

    def rebuild(self, references, check: bool = False) -> "HistReferenceBank":
        refs = self._as_set(references)
        dtype = np.dtype(np.uint8 if refs.dtype in (torch.uint8, np.uint8) else np.float32)
        if tuple(int(v) for v in refs.shape) != self.shape or dtype != self.dtype:
            raise ValueError("HistReferenceBank.rebuild: %s references of shape %r, got %s %r"
                             % (self.dtype, self.shape, dtype, tuple(refs.shape)))
        if torch.is_tensor(refs):
            if refs.device != self.device:
                raise ValueError("HistReferenceBank.rebuild: the references are on %s, the bank on %s" % (refs.device, self.device))
            refs = refs.contiguous()
        else:
            host = torch.from_numpy(np.ascontiguousarray(refs))
            if self._staged is None:
                self._staged = torch.empty(self.shape, dtype=host.dtype, device=self.device)
            self._staged.copy_(host.pin_memory() if self.device.type == "cuda" else host, non_blocking=True)
            refs = self._staged
        K.hist_bank_build(refs, self.bank, self._workspace, self.flag)
        if self.float_bank is not None:
            self._float_refs.copy_(refs)                                   # (uint8 -> fp32 is exact)
            K.hist_bank_build(self._float_refs, self.float_bank, self._float_workspace, self._float_flag)
        if check and int(self.flag.item()) != 0:
            raise ValueError("HistReferenceBank: the reference images must be real and finite")
        return self

    def index_tensor(self, index, batch: int) -> torch.Tensor:
        """the int32 ``[batch]`` device tensor of a ``match_histograms`` ``index`` argument (see there)"""
        if torch.is_tensor(index) and index.is_cuda:
            if index.dtype != torch.int32 or tuple(index.shape) != (batch,):
                raise TypeError("match_histograms: a device index is an int32 [%d] tensor, got %s %r"
                                % (batch, index.dtype, tuple(index.shape)))
            return index.contiguous()                                       # (entries are clamped on the device, not checked)
        if index is None:
            if self.size not in (1, batch):
                raise ValueError("match_histograms: index=None needs as many references as samples (%d references, %d samples) "
                                 "or a bank of one" % (self.size, batch))
            if batch not in self._index_cache:
                self._index_cache[batch] = (torch.arange(batch, dtype=torch.int32, device=self.device) if self.size == batch
                                            else torch.zeros(batch, dtype=torch.int32, device=self.device))
            return self._index_cache[batch]
        return to_device((validate_index(index, batch, self.size),), self.device)[0]


def validate_index(index, batch: int, size: int) -> np.ndarray:
    """a host ``index`` (sequence or numpy array of integers) as int32 ``[batch]``; raises unless it holds ``batch`` entries
    in ``[0, size)``"""
    arr = np.asarray(index.cpu() if torch.is_tensor(index) else index)
    if arr.dtype.kind not in "iu":
        raise TypeError("match_histograms: index holds integers, got %s" % (arr.dtype,))
    if arr.shape != (batch,):
        raise ValueError("match_histograms: index must hold one entry per sample (%d), got shape %r" % (batch, arr.shape))
    if arr.size and (arr.min() < 0 or arr.max() >= size):
        raise ValueError("match_histograms: index entries must lie in [0, %d), got %d .. %d" % (size, arr.min(), arr.max()))
    return np.ascontiguousarray(arr.astype(np.int32))


def _match_bank(image: torch.Tensor, bank: HistReferenceBank, index) -> torch.Tensor:
    if image.shape[-1] != bank.channels:
        raise ValueError("match_histograms: number of channels in the input image (%d) and the reference images (%d) must match"
                         % (image.shape[-1], bank.channels))
    if image.dtype == torch.uint8 and bank.dtype != np.uint8:
        raise TypeError("match_histograms: uint8 images take a uint8 bank, got %s" % (bank.dtype,))
    if image.dtype == torch.float32 and bank.dtype == np.uint8 and bank.float_bank is None:
        raise TypeError("match_histograms: fp32 images against a uint8 bank need HistReferenceBank(.., float_images=True)")
    batch = image if image.dim() == 4 else image[None]
    idx = bank.index_tensor(index, int(batch.shape[0]))
    store = bank.bank if (image.dtype == torch.uint8) == (bank.dtype == np.uint8) else bank.float_bank
    out = K.match_hist_bank(batch, store, bank.shape, idx)
    return out if image.dim() == 4 else out[0]


def match_histograms(image: torch.Tensor, reference: Union[HistReference, HistReferenceBank], multichannel: bool = True,
                     index=None) -> torch.Tensor:
    """``skimage.exposure.match_histograms(image, reference, multichannel=True)`` on the device: ``[B,H,W,C]`` images (or the
    reference's single ``[H,W,C]``), fp32 or uint8 -> a new tensor of the same shape and dtype.  uint8 images take a uint8
    reference (the result is then a uint8 value; anything else would wrap in the cast).

    With a ``HistReferenceBank`` sample ``i`` is matched to reference ``index[i]``, the result equal bit for bit to the match
    against that reference alone.  ``index``: a host sequence or numpy array of ``B`` integers in ``[0, R)`` (validated here,
    uploaded through a pinned non-blocking copy), or an int32 ``[B]`` device tensor (NOT checked: the kernel clamps every entry
    into ``[0, R)``), or ``None``, which needs ``R == B`` (sample ``i`` takes reference ``i``) or ``R == 1``.  uint8 images need a
    uint8 bank; fp32 images take an fp32 bank or a uint8 bank built with ``float_images=True``."""
    if not isinstance(reference, (HistReference, HistReferenceBank)):
        raise TypeError("match_histograms: reference is a HistReference (HistReference(reference_hwc, device)) or a "
                        "HistReferenceBank")
    if multichannel is not True:
        raise TypeError("match_histograms: only multichannel=True (the reference's call) is built")
    if not torch.is_tensor(image) or image.dtype not in (torch.float32, torch.uint8):
        raise TypeError("match_histograms: fp32 or uint8 device tensors, got %s" % (getattr(image, "dtype", type(image)),))
    if image.dim() not in (3, 4):
        raise ValueError("match_histograms: [B,H,W,C] or [H,W,C] images, got %d dimensions" % image.dim())
    if isinstance(reference, HistReferenceBank):
        return _match_bank(image, reference, index)
    if index is not None:
        raise TypeError("match_histograms: index goes with a HistReferenceBank (a HistReference is one image for every sample)")
    if image.shape[-1] != reference.channels:
        raise ValueError("match_histograms: number of channels in the input image (%d) and the reference image (%d) must match"
                         % (image.shape[-1], reference.channels))
    if image.dtype == torch.uint8 and reference.dtype != np.uint8:
        raise TypeError("match_histograms: uint8 images take a uint8 reference, got %s" % (reference.dtype,))
    batch = image if image.dim() == 4 else image[None]
    out = K.match_hist(batch, reference.values, reference.quantiles, reference.lengths)
    return out if image.dim() == 4 else out[0]
