"""Device-side slice preparation of the MS-CMRSeg data.

Every image of the MS-CMRSeg set passes through ``src/utils/read_nii_image.py`` before the networks see it
(``read_*_nii_save_png``, ``:89-181``): ``sitk.RescaleIntensity`` and a cast to uint8, a nearest-neighbour resize to 256x256
(``resize_volume``), the centre crop to 224 (``crop_volume``), and ``preprocess_volume`` (``:60-74``):
``cv2.createCLAHE(clipLimit=2.0, tileGridSize=(4, 4)).apply`` on each uint8 slice.  Here the chain is two HIP entry points
(``csrc/preprocess.hip``): ``pcuda_rescale_resize_crop_u8`` -- the volume's minimum and maximum reduced on the device, then
rescale, resize and crop in one pass over the output -- and ``pcuda_clahe`` -- per-tile histograms, the integer
clip-and-redistribute, a prefix sum, and the four-LUT bilinear blend per pixel.

cv2, skimage, albumentations and SimpleITK are not dependencies of this package, and parity with OpenCV / ITK is unpinned:
the convention (``include/pcuda_hip.h``) is this build's own, written after OpenCV's ``clahe.cpp`` and ITK's
``RescaleIntensityImageFilter``.  It is pinned by two independent restatements in a committed golden file
(``scripts/make_preprocess_golden.py`` -> ``tests/golden/preprocess.npz``), and the device equals them bit for bit.  NaN in
a volume is unsupported.  Not here: ``albumentations.CLAHE`` of the evaluation script (the L channel of LAB, a random clip
limit), 16-bit CLAHE, and NIfTI / PNG file I/O (the ``.npy`` path of ``read_nii_image.py`` is ``utils/resample.py``)."""
from __future__ import annotations

import math
from typing import Tuple

import torch

from .. import kernels as K

_VOLUME_DTYPES = (torch.float32, torch.int16, torch.uint8)


def _check_grid(h: int, w: int, clip_limit: float, tile_grid_size) -> Tuple[int, int]:
    """the host side of ``pcuda_clahe``'s argument checks -> (tiles_x, tiles_y)"""
    try:
        tiles_x, tiles_y = tile_grid_size
        tiles_x, tiles_y = int(tiles_x), int(tiles_y)
    except (TypeError, ValueError):
        raise TypeError("clahe: tile_grid_size is (tiles_x, tiles_y), got %r" % (tile_grid_size,))
    if not (1 <= tiles_x <= 16 and 1 <= tiles_y <= 16):
        raise ValueError("clahe: 1..16 tiles per axis, got (%d, %d)" % (tiles_x, tiles_y))
    if h < 2 or w < 2:
        raise ValueError("clahe: slices of at least 2x2, got %dx%d" % (h, w))
    if isinstance(clip_limit, bool) or not isinstance(clip_limit, (int, float)) or math.isnan(clip_limit):
        raise ValueError("clahe: clip_limit is a real number, got %r" % (clip_limit,))
    eh, ew = h, w
    if w % tiles_x != 0 or h % tiles_y != 0:
        eh, ew = h + (tiles_y - h % tiles_y), w + (tiles_x - w % tiles_x)
    if eh - h > h - 1 or ew - w > w - 1:
        raise ValueError("clahe: the reflected border of a %dx%d slice under a (%d, %d) grid is wider than the slice"
                         % (h, w, tiles_x, tiles_y))
    if (eh // tiles_y) * (ew // tiles_x) >= 1 << 24:
        raise ValueError("clahe: a tile of 2^24 pixels or more")
    return tiles_x, tiles_y


def clahe(images_u8: torch.Tensor, clip_limit: float = 2.0, tile_grid_size=(4, 4), to_float: bool = False) -> torch.Tensor:
    """``cv2.createCLAHE(clip_limit, tile_grid_size).apply`` on uint8 device slices ``[N,H,W]`` (or one ``[H,W]``) -> a new uint8
    tensor of the same shape, or, with ``to_float``, fp32 ``[N,3,H,W]`` holding ``u8 / 255`` in all three channels (what
    ``cv2.imread`` of the grey PNG, ``/ 255.`` and ``moveaxis`` give the networks).  ``tile_grid_size`` is ``(tiles_x, tiles_y)``
    as in cv2."""
    if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8:
        raise TypeError("clahe: uint8 device tensors, got %s" % (getattr(images_u8, "dtype", type(images_u8)),))
    if images_u8.dim() not in (2, 3):
        raise ValueError("clahe: [N,H,W] or [H,W] slices, got %d dimensions" % images_u8.dim())
    tiles_x, tiles_y = _check_grid(int(images_u8.shape[-2]), int(images_u8.shape[-1]), clip_limit, tile_grid_size)
    batch = images_u8 if images_u8.dim() == 3 else images_u8[None]
    out = K.clahe(batch, float(clip_limit), tiles_x, tiles_y, bool(to_float))
    return out if images_u8.dim() == 3 or to_float else out[0]


def preprocess_volume(img_volume: torch.Tensor) -> torch.Tensor:
    """The reference's ``preprocess_volume`` (``read_nii_image.py:60-74``): CLAHE with clip limit 2.0 on a 4x4 grid, slice by slice."""
    return clahe(img_volume, clip_limit=2.0, tile_grid_size=(4, 4))


def _volume(vol, what: str, dtypes=_VOLUME_DTYPES) -> torch.Tensor:
    if not torch.is_tensor(vol) or vol.dtype not in dtypes:
        raise TypeError("%s: a %s device volume, got %s" % (what, " / ".join(str(d).replace("torch.", "") for d in dtypes),
                                                            getattr(vol, "dtype", type(vol))))
    if vol.dim() != 3:
        raise ValueError("%s: a [N,H,W] volume, got %d dimensions" % (what, vol.dim()))
    return vol


def _check_crop(what: str, crop: int, h: int, w: int) -> int:
    crop = int(crop)
    if crop < 0 or (crop > 0 and (crop // 2 < 1 or h // 2 - crop // 2 < 0 or w // 2 - crop // 2 < 0)):
        raise ValueError("%s: a centre crop of %d leaves the %dx%d slice" % (what, crop, h, w))
    return crop


def rescale_intensity_u8(vol: torch.Tensor) -> torch.Tensor:
    """``sitk.Cast(sitk.RescaleIntensity(vol), sitk.sitkUInt8)``: the volume's own minimum .. maximum stretched to 0 .. 255 in
    float64 and truncated; fp32, int16 or uint8 ``[N,H,W]`` -> uint8 ``[N,H,W]``."""
    return K.rescale_resize_crop_u8(_volume(vol, "rescale_intensity_u8"))


def resize_volume(img_volume: torch.Tensor, w: int = 256, h: int = 256) -> torch.Tensor:
    """The reference's ``resize_volume`` on a uint8 volume: ``cv2.resize(.., (w, h), interpolation=cv2.INTER_NEAREST)`` per slice;
    the values are kept as they are."""
    _volume(img_volume, "resize_volume", (torch.uint8,))
    if int(w) < 1 or int(h) < 1:
        raise ValueError("resize_volume: a target of at least 1x1, got %dx%d" % (h, w))
    return K.rescale_resize_crop_u8(img_volume, int(h), int(w), 0, raw=True)


def crop_volume(vol: torch.Tensor, crop_size: int = 112) -> torch.Tensor:
    """The reference's ``crop_volume`` on a uint8 volume: rows and columns ``size // 2 - crop_size .. size // 2 + crop_size``
    (``crop_size`` is HALF the side of the result)."""
    _volume(vol, "crop_volume", (torch.uint8,))
    if int(crop_size) < 1:
        raise ValueError("crop_volume: crop_size >= 1, got %r" % (crop_size,))
    crop = _check_crop("crop_volume", 2 * int(crop_size), int(vol.shape[1]), int(vol.shape[2]))
    return K.rescale_resize_crop_u8(vol, None, None, crop, raw=True)


def prepare_mscmrseg_slices(raw_volume: torch.Tensor, size: int = 256, crop_size: int = 224, clahe: bool = True,
                            to_float: bool = True) -> torch.Tensor:
    """The whole chain of ``read_*_nii_save_png`` (``crop_size`` is the side of the result, as there) in two entry-point calls:
    rescale to uint8, the nearest resize to ``size`` x ``size`` (the identity for a volume of that size already), the centre
    crop, CLAHE (2.0, 4x4) -> fp32 ``[N,3,crop,crop]`` in 0 .. 1, what ``predict_labels`` / ``evaluate_volume`` take; with
    ``to_float=False`` the uint8 ``[N,crop,crop]`` slices the reference writes as PNG files.  ``clahe=False`` is the label
    volumes' path (``read_*_nii_label_save_png``): uint8 out, so it takes ``to_float=False``."""
    _volume(raw_volume, "prepare_mscmrseg_slices")
    size = int(size)
    if size < 1:
        raise ValueError("prepare_mscmrseg_slices: size >= 1, got %d" % size)
    crop = _check_crop("prepare_mscmrseg_slices", crop_size, size, size)
    if not clahe and to_float:
        raise ValueError("prepare_mscmrseg_slices: clahe=False is the uint8 label path of the reference: pass to_float=False")
    side = 2 * (crop // 2) if crop else size
    if clahe:
        _check_grid(side, side, 2.0, (4, 4))
    u8 = K.rescale_resize_crop_u8(raw_volume, size, size, crop)
    if not clahe:
        return u8
    return K.clahe(u8, 2.0, 4, 4, bool(to_float))
