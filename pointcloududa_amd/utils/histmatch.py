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
reference is refused.  Not here: other dtypes, ``multichannel=False``, a reference per sample."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .. import kernels as K


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
        values, quantiles, lengths = reference_tables(ref)
        self.dtype = ref.dtype
        self.channels = int(ref.shape[2])
        self.device = torch.device(device)

        def put(a):
            t = torch.from_numpy(np.ascontiguousarray(a))
            if self.device.type == "cuda":
                t = t.pin_memory()
            return t.to(self.device, non_blocking=True)
        self.values, self.quantiles, self.lengths = put(values), put(quantiles), put(lengths)


def match_histograms(image: torch.Tensor, reference: HistReference, multichannel: bool = True) -> torch.Tensor:
    """``skimage.exposure.match_histograms(image, reference, multichannel=True)`` on the device: ``[B,H,W,C]`` images (or the
    reference's single ``[H,W,C]``), fp32 or uint8 -> a new tensor of the same shape and dtype.  uint8 images take a uint8
    reference (the result is then a uint8 value; anything else would wrap in the cast)."""
    if not isinstance(reference, HistReference):
        raise TypeError("match_histograms: reference is a HistReference (HistReference(reference_hwc, device))")
    if multichannel is not True:
        raise TypeError("match_histograms: only multichannel=True (the reference's call) is built")
    if not torch.is_tensor(image) or image.dtype not in (torch.float32, torch.uint8):
        raise TypeError("match_histograms: fp32 or uint8 device tensors, got %s" % (getattr(image, "dtype", type(image)),))
    if image.dim() not in (3, 4):
        raise ValueError("match_histograms: [B,H,W,C] or [H,W,C] images, got %d dimensions" % image.dim())
    if image.shape[-1] != reference.channels:
        raise ValueError("match_histograms: number of channels in the input image (%d) and the reference image (%d) must match"
                         % (image.shape[-1], reference.channels))
    if image.dtype == torch.uint8 and reference.dtype != np.uint8:
        raise TypeError("match_histograms: uint8 images take a uint8 reference, got %s" % (reference.dtype,))
    batch = image if image.dim() == 4 else image[None]
    out = K.match_hist(batch, reference.values, reference.quantiles, reference.lengths)
    return out if image.dim() == 4 else out[0]
