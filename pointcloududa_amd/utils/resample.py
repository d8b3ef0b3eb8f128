"""Device-side spacing resample of the MS-CMRSeg data: the ``.npy`` path of the reference.

``src/utils/read_nii_image.py`` prepares a spacing-normalised variant of the data next to the PNG slices
(``read_*_nii_save_npy``, ``:202-231``; ``read_*_nii_label_save_npy``, ``:234-271``).  Images: ``ndimage.zoom(vol, [1, fy, fx],
order=1)`` to 1.2 mm in-plane spacing, ``crop_volume`` to 224, ``(image - image.mean()) / image.std()`` over the volume.  Labels:
the raw codes ``200 / 500 / 600 -> 1 / 2 / 3``, ``to_categorical(.., 4)``, ``ndimage.zoom(onehot, [1, 1, fy, fx], order=1)``,
``argmax(axis=1)``, ``crop_volume``.  Here each chain is one HIP entry point (``csrc/resample.hip``): ``pcuda_zoom_standardize``
(zoom, crop, the statistics reduced on the device, the map) and ``pcuda_zoom_labels`` (the chain fused, no one-hot tensor);
``pcuda_zoom_linear_crop`` is the zoom and crop on their own.

scipy is not a dependency of this package.  The arithmetic is ``scipy.ndimage.zoom``'s (1.15.3), pinned bit for bit: the
expected arrays of the committed golden file are the outputs of scipy / numpy themselves
(``scripts/make_resample_golden.py`` -> ``tests/golden/resample.npz``), and the convention is written out in
``include/pcuda_hip.h``.  Integer volumes get numpy's mean exactly and its standard deviation to 2e-16; for fp32 volumes the
statistics are this build's own convention (float64 sums of the fp32 zoomed values in a fixed order; numpy's float32 pairwise
accumulation is not reproduced).  NaN in a volume is unsupported.  Not here: NIfTI file I/O and SimpleITK (the caller brings
the array, its size and its spacing), spline orders other than 1, a zoom along the slice axis, scipy's other boundary modes
and ``grid_mode=True``, uint16 volumes, a per-slice standardisation."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from .. import kernels as K

_VOLUME_DTYPES = (torch.float32, torch.int16, torch.uint8)
_LABEL_DTYPES = (torch.int16, torch.uint8)
MSCMRSEG_REMAP = ((200, 1), (500, 2), (600, 3))


def zoom_output_shape(shape_hw: Sequence[int], zoom_yx: Sequence[float]) -> Tuple[int, int]:
    """The size ``scipy.ndimage.zoom`` gives a ``shape_hw`` slice under the factors ``zoom_yx``: ``int(round(dim * factor))`` per axis."""
    try:
        (h, w), (fy, fx) = shape_hw, zoom_yx
        fy, fx = float(fy), float(fx)
    except (TypeError, ValueError):
        raise TypeError("zoom_output_shape: shape_hw is (H, W) and zoom_yx is (fy, fx), got %r, %r" % (shape_hw, zoom_yx))
    if not (fy > 0.0 and fx > 0.0 and np.isfinite(fy) and np.isfinite(fx)):
        raise ValueError("zoom_output_shape: positive finite zoom factors, got %r" % (zoom_yx,))
    return int(round(int(h) * fy)), int(round(int(w) * fx))


def spacing_zoom_factors(size_xy: Sequence[int], spacing_xy: Sequence[float], new_spacing: Sequence[float] = (1.2, 1.2)) -> Tuple[float, float]:
    """The reference's in-plane factors from ``vol.GetSize()[:2]`` and ``vol.GetSpacing()[:2]``: ``resize_factor = spacing /
    new_spacing``, ``new_shape = np.round(shape * resize_factor)``, ``real_resize_factor = new_shape / shape``.  The reference
    hands ``real_resize_factor[0]`` to the first in-plane axis of the array and ``[1]`` to the second, and so does this: the
    result is ``zoom_yx``."""
    shape = np.asarray(size_xy, dtype=np.float64)
    spacing = np.asarray(spacing_xy, dtype=np.float64)
    new = np.asarray(new_spacing, dtype=np.float64)
    if shape.shape != (2,) or spacing.shape != (2,) or new.shape != (2,):
        raise ValueError("spacing_zoom_factors: two in-plane sizes, spacings and new spacings, got %r, %r, %r"
                         % (size_xy, spacing_xy, new_spacing))
    if not (np.all(shape >= 1) and np.all(spacing > 0) and np.all(new > 0)):
        raise ValueError("spacing_zoom_factors: sizes of at least 1 and positive spacings, got %r, %r, %r"
                         % (size_xy, spacing_xy, new_spacing))
    real = np.round(shape * (spacing / new)) / shape
    return float(real[0]), float(real[1])


def _volume(vol, what: str, dtypes=_VOLUME_DTYPES) -> torch.Tensor:
    if not torch.is_tensor(vol) or vol.dtype not in dtypes:
        raise TypeError("%s: a %s device volume, got %s" % (what, " / ".join(str(d).replace("torch.", "") for d in dtypes),
                                                            getattr(vol, "dtype", type(vol))))
    if vol.dim() != 3:
        raise ValueError("%s: a [N,H,W] volume, got %d dimensions" % (what, vol.dim()))
    return vol


def _zoomed(what: str, vol: torch.Tensor, zoom_yx, crop_size) -> Tuple[Tuple[int, int], int]:
    """the host side of the entry points' geometry checks -> ((zh, zw), crop)"""
    h, w = int(vol.shape[1]), int(vol.shape[2])
    if h < 1 or w < 1 or h > 32768 or w > 32768:
        raise ValueError("%s: slices with sides 1..32768, got %dx%d" % (what, h, w))
    zh, zw = zoom_output_shape((h, w), zoom_yx)
    if zh < 1 or zw < 1 or zh > 32768 or zw > 32768:
        raise ValueError("%s: the zoomed slice has sides 1..32768, got %dx%d" % (what, zh, zw))
    crop = int(crop_size)
    half = crop // 2
    if crop < 0 or (crop > 0 and (half < 1 or zh // 2 - half < 0 or zw // 2 - half < 0 or zh // 2 + half > zh or zw // 2 + half > zw)):
        raise ValueError("%s: a centre crop of %d leaves the %dx%d zoomed slice" % (what, crop, zh, zw))
    return (zh, zw), crop


def zoom_linear(volume: torch.Tensor, zoom_yx, crop_size: int = 0) -> torch.Tensor:
    """``scipy.ndimage.zoom(volume, [1, fy, fx], order=1)`` of a fp32, int16 or uint8 device volume ``[N,H,W]``, then the
    reference's ``crop_volume`` to ``crop_size`` (the side of the result; 0: no crop) -> a new tensor of the same dtype."""
    _volume(volume, "zoom_linear")
    zoomed, crop = _zoomed("zoom_linear", volume, zoom_yx, crop_size)
    return K.zoom_linear_crop(volume, zoomed, crop)


def standardize_zoomed(volume: torch.Tensor, zoom_yx, crop_size: int = 224, channels: int = 1, return_stats: bool = False):
    """The image chain: zoom, crop, ``(image - image.mean()) / image.std()`` over the whole cropped zoomed volume -> fp32
    ``[N,crop,crop]``, or with ``channels=3`` ``[N,3,crop,crop]`` holding the same value in all three channels (what
    ``predict_labels`` takes).  The statistics never leave the device; ``return_stats=True`` also returns them as Python floats
    ``(out, mean, std)`` (one synchronisation)."""
    _volume(volume, "standardize_zoomed")
    if channels not in (1, 3):
        raise ValueError("standardize_zoomed: channels is 1 or 3, got %r" % (channels,))
    zoomed, crop = _zoomed("standardize_zoomed", volume, zoom_yx, crop_size)
    out, stats = K.zoom_standardize(volume, zoomed, crop, int(channels))
    if not return_stats:
        return out
    if volume.shape[0] == 0:
        return out, float("nan"), float("nan")
    mean, std = stats.tolist()
    return out, mean, std


def zoom_labels(labels: torch.Tensor, zoom_yx, num_classes: int = 4, remap=MSCMRSEG_REMAP, crop_size: int = 224,
                check: bool = True) -> torch.Tensor:
    """The label chain: the ``(from, to)`` pairs of ``remap`` in order (the reference's chained ``np.where``), ``to_categorical``,
    the zoom of the one-hot tensor, ``argmax`` and the crop, fused -> uint8 ``[N,crop,crop]``.  With ``check`` the device-side
    count of values that are no class is read (one synchronisation) and a ``ValueError`` is raised where the reference's
    ``to_categorical`` would assert; with ``check=False`` such values match no class and nothing synchronises."""
    _volume(labels, "zoom_labels", _LABEL_DTYPES)
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 8:
        raise ValueError("zoom_labels: 2..8 classes, got %r" % (num_classes,))
    try:
        pairs = tuple((int(a), int(b)) for a, b in remap)
    except (TypeError, ValueError):
        raise TypeError("zoom_labels: remap is a sequence of (from, to) pairs, got %r" % (remap,))
    if len(pairs) > 8:
        raise ValueError("zoom_labels: a remap table of at most 8 (from, to) pairs, got %d" % len(pairs))
    zoomed, crop = _zoomed("zoom_labels", labels, zoom_yx, crop_size)
    out, counter = K.zoom_labels(labels, zoomed, num_classes, pairs, crop)
    if check:
        stray = int(counter.item())
        if stray:
            raise ValueError("zoom_labels: %d values of the volume are outside 0..%d after the remap %r (the reference's "
                             "to_categorical asserts)" % (stray, num_classes - 1, pairs))
    return out


def prepare_mscmrseg_npy(raw_volume: torch.Tensor, spacing_xy, new_spacing=(1.2, 1.2), crop_size: int = 224,
                         channels: int = 3) -> torch.Tensor:
    """``read_{lge,bssfp,t2}_nii_save_npy`` on a raw device volume ``[N,H,W]`` with in-plane spacing ``spacing_xy`` (mm): the
    factors of ``spacing_zoom_factors`` (the size is the volume's own: ``GetSize()`` is ``(W, H)``), then ``standardize_zoomed``."""
    _volume(raw_volume, "prepare_mscmrseg_npy")
    factors = spacing_zoom_factors((raw_volume.shape[2], raw_volume.shape[1]), spacing_xy, new_spacing)
    return standardize_zoomed(raw_volume, factors, crop_size, channels)


def prepare_mscmrseg_npy_labels(raw_labels: torch.Tensor, spacing_xy, new_spacing=(1.2, 1.2), crop_size: int = 224,
                                num_classes: int = 4, remap=MSCMRSEG_REMAP, check: bool = True) -> torch.Tensor:
    """``read_*_nii_label_save_npy`` on a raw device label volume: the same factors, then ``zoom_labels``."""
    _volume(raw_labels, "prepare_mscmrseg_npy_labels", _LABEL_DTYPES)
    factors = spacing_zoom_factors((raw_labels.shape[2], raw_labels.shape[1]), spacing_xy, new_spacing)
    return zoom_labels(raw_labels, factors, num_classes, remap, crop_size, check)
