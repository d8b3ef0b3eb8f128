"""Device-side light augmentation for the loader path.

The reference's ``light_aug`` (``src/data_generator_mmwhs.py:87-122``) and ``simple_aug``
(``src/data_generator_mscmrseg.py:135-167``) are ``imgaug`` pipelines: ``Fliplr``, ``Flipud`` and, sometimes, one
``Affine`` (scale, translate, rotate, shear, interpolation order 0 or 1, constant fill), applied in random order.  Here
the per-sample parameters are drawn on the host from a numpy ``Generator``, composed into one inverse 2x3 matrix per
sample in float64, and a single HIP kernel (``csrc/augment.hip``) warps the batch, rescales it and assembles it (centre
crop, channels first, one-hot) -- so the device-side point-cloud sampler finally has a device-side producer.

The sub-pixel convention is this build's own (imgaug / cv2 are not vendored by the reference: parity unpinned) and is
pinned against ``scipy.ndimage.affine_transform`` by ``tests/golden/augment.npz``:

* centre ``c = ((W-1)/2, (H-1)/2)``; forward map in pixel coordinates (x right, y down)
  ``A = T(c + (tx*W, ty*H)) . R(rotate) . Sh(shear) . S(sx, sy) . T(-c)`` with ``R = [[cos, -sin], [sin, cos]]`` and
  ``Sh = [[1, tan(shear)], [0, 1]]``; flips are ``x -> W-1-x`` and ``y -> H-1-y``; the maps are multiplied in application
  order; the kernel receives the inverse (output pixel -> source coordinate)
* coordinates and interpolation in float64; order 0 takes the texel at ``floor(coord + 0.5)``, order 1 is bilinear with
  ``cval`` for a neighbour outside the image; the result is ``floor(v + 0.5)`` clipped to [0, 255]
* masks take order 0 and fill 0 whatever the image's order and ``cval`` are

imgaug's own parameter stream of the heavy pipeline (``augmentation``) is not reproduced: the string ``"heavy"`` keeps
raising.  The photometric operators of ``augmentation2`` (blurs, sharpen / emboss, noise, dropouts, invert, add, multiply,
grayscale) live in ``utils/photometric.py`` (f7) and are re-exported here; ``augment_batch(.., photometric=program)`` and
``AugmentedBatches(.., photometric_preset=..)`` apply them to uint8 images in front of the warp.  The warps of the heavy
pipeline (``CropAndPad``, the +/-45 degree ``Affine`` with every border mode, elastic, piecewise affine, perspective) live in
``utils/geometric.py`` (f8) and are re-exported here too; ``augment_batch(.., heavy=plan)`` and
``AugmentedBatches(.., heavy_preset="heavy_device")`` run a whole plan (photometric and geometric stages interleaved) on the uint8
images and the masks in front of the f6 launch.  ``Superpixels``, ``SimplexNoiseAlpha(EdgeDetect | DirectedEdgeDetect)`` and
``AddToHueAndSaturation`` live in ``utils/stylize.py`` (f9) and are re-exported here as well: the presets
``"heavy_full_device"`` and ``"mscmrseg_aug2_full_device"`` hold all fifteen / twelve ``SomeOf`` entries of the two recipes, while
``"heavy_device"`` and ``"mscmrseg_aug2_device"`` keep drawing what they drew without the three.  ``CropAndPad`` with all ten
modes of ``numpy.pad`` (``pad_mode=ia.ALL``) lives in ``utils/croppad.py`` (f14) and is re-exported here (``CropPadProgram``,
``crop_pad_aug``, ``MODE_NAMES``): the presets ``"heavy_refpad_device"`` and ``"mscmrseg_aug2_refpad_device"`` are the two full
recipes with it; ``"heavy_connected_device"`` / ``"mscmrseg_aug2_connected_device"`` add connected superpixels (f9b) and
``"heavy_scaled_device"`` / ``"mscmrseg_aug2_scaled_device"`` imgaug's ``max_size = 128`` working size on top (f9c).  Histogram matching against a
fixed reference image (the MM-WHS generator's ``-mh``) lives in ``utils/histmatch.py`` (f10) and is re-exported here:
``augment_batch(.., match_hist=reference)`` and ``AugmentedBatches(.., match_hist_reference=image)`` apply it to the raw images
in front of everything else.  A reference per sample, drawn from a ``HistReferenceBank`` that stays on the device (f10b):
``augment_batch(.., match_hist=bank, match_hist_index=idx)`` and ``AugmentedBatches(.., match_hist_bank=bank)``.
Fourier domain adaptation against a ``FourierBank`` (f10c, ``utils/fourier.py``: the low-frequency amplitudes of a target
image, the source's own phase) is re-exported here too:
``augment_batch(.., fourier=bank, fourier_index=idx, fourier_radius=rad)`` and ``AugmentedBatches(.., fourier_bank=bank)`` apply it
to the raw images behind ``match_hist`` and in front of everything else.  fp32 batches
reach the uint8 stages through ``rescale="minmax_u8"`` (f6b: ``quantize_minmax``, then the plan or program, then the dequantising
assemble), which is the MM-WHS generator's ``-aug heavy`` branch.

This module is the facade: the parameters and matrices of the light pipeline live in ``utils/affine.py``, the heavy recipes
(presets, ``sample_heavy_plan``, ``heavy_aug``, ``sample_geo_program``, ``sample_style_program``) in ``utils/heavy.py``, the frame all
programs share in ``utils/_program.py``; every name is re-exported here."""
from __future__ import annotations

from typing import Iterable, Optional, Union

import numpy as np
import torch

from .. import kernels as K
from .npy2point import masks_to_pointclouds
from ._program import HEAVY_MESSAGE, as_labels, like_masks  # noqa: F401
from .affine import (OP_AFFINE, OP_FLIPLR, OP_FLIPUD, ROTATE, SCALE, SHEAR, TRANSLATE_X, TRANSLATE_Y, _PRESETS, AugmentParams,  # noqa: F401
                     _translate, forward_matrices, inverse_matrices, kernel_params, sample_params, upload_params)
from .photometric import (PHOTOMETRIC_PRESET, PhotoProgram, emboss_weights, gaussian_weights, photometric_aug,  # noqa: F401
                          sample_program, sharpen_weights, upload_program)
from .geometric import GeoProgram, geometric_aug, upload_geo_program  # noqa: F401
from .stylize import (StyleProgram, directed_edge_weights, edge_detect_weights, simplex_grid, stylize_aug, superpixel_grid,  # noqa: F401
                      superpixel_min_size, superpixel_working_size, upload_style_program)
from .histmatch import HistReference, HistReferenceBank, match_histograms, reference_tables  # noqa: F401
from .fourier import FourierBank, fourier_adapt  # noqa: F401
from .croppad import MODE_NAMES, CropPadProgram, crop_pad_aug, upload_crop_pad_program  # noqa: F401
from .heavy import (AUG2_CONNECTED_PRESET, AUG2_DEVICE_PRESET, AUG2_FULL_PRESET, AUG2_REFPAD_PRESET, AUG2_SCALED_PRESET,  # noqa: F401
                    HEAVY_CONNECTED_PRESET, HEAVY_DEVICE_PRESET, HEAVY_FULL_PRESET, HEAVY_REFPAD_PRESET, HEAVY_SCALED_PRESET, HeavyPlan, _check_interp, _check_preset, heavy_aug,
                    sample_geo_program, sample_heavy_plan, sample_style_program)


RESCALES = ("minmax", "minmax_u8", "div255", None)


def _check_rescale(who, rescale):
    if rescale is not None and not (isinstance(rescale, str) and rescale in RESCALES):
        raise ValueError("%s: rescale must be 'minmax', 'minmax_u8', 'div255' or None, got %r" % (who, rescale))


def quantize_minmax(images_f32: torch.Tensor):
    """``data_generator_mmwhs.py:246-249`` on the device: fp32 ``[B,H,W,C]`` images -> ``(q uint8 [B,H,W,C], minmax [2])`` with
    the batch-global ``(min, max)`` pair kept on the device (``kernels.minmax``) and ``q = trunc((x - min) * 255 / (max - min))``
    in fp32 (``kernels.quantize_u8``); ``max == min`` gives 0 everywhere.  ``kernels.augment_assemble_dequant`` takes both back
    to fp32 behind the uint8 stages."""
    if not torch.is_tensor(images_f32) or images_f32.dtype != torch.float32 or images_f32.dim() != 4:
        raise TypeError("quantize_minmax: fp32 [B,H,W,C] images")
    images_f32 = images_f32.contiguous()
    mm = K.minmax(images_f32)
    return K.quantize_u8(images_f32, mm), mm


def augment_batch(images_hwc: torch.Tensor, masks: torch.Tensor, params: Optional[AugmentParams], num_classes: int = 5,
                  crop_size: int = 0, rescale: Optional[str] = "minmax", resample_verts: bool = False,
                  firsts: Optional[torch.Tensor] = None, verts: Optional[torch.Tensor] = None, fused_mask: bool = True,
                  photometric: Optional[PhotoProgram] = None, heavy: Optional[HeavyPlan] = None,
                  match_hist: Optional[Union[HistReference, HistReferenceBank]] = None, match_hist_index=None,
                  fourier: Optional[FourierBank] = None, fourier_index=None, fourier_radius=None):
    """``data_generator_mmwhs.py:245-274`` after the file reads (``rescale="minmax"``, fp32 images), or
    ``data_generator_mscmrseg.py:305-317`` (``rescale="div255"``, uint8 images), on the device: images ``[B,H,W,C]``,
    integer masks ``[B,H,W]`` (or ``[B,H,W,1]``) ->
    ``(images [B,C,h,w] fp32, one-hot uint8 [B,K,h,w], verts fp32 [B,300,3] / 255 or None)``.

    ``"minmax"``: batch-global min and max (kept on the device), ``q = trunc((x - min) * 255 / (max - min))`` as uint8,
    warp, ``min + float(q') * (max - min) / 255``, all fp32.  ``max == min`` is undefined in the reference (a NaN cast to
    uint8); here ``q`` is 0 everywhere, so every output equals ``min``.  ``"div255"``: warp, ``float32(q') / 255``.
    ``None``: no quantisation, the fp32 values themselves are gathered / interpolated; with ``params=None`` or
    all-identity parameters this is ``assemble_batch`` bit for bit.  ``"minmax_u8"`` (fp32 images; the MM-WHS generator's
    ``-aug heavy`` branch, ``data_generator_mmwhs.py:245-263``): the same round trip with the uint8 images written out in
    between, so that a ``heavy`` plan and a ``photometric`` program run on them: ``match_hist`` on fp32, min / max, quantise
    (``quantize_minmax``), plan, program, then the warp with ``min + float(q') * (max - min) / 255``
    (``kernels.augment_assemble_dequant``).  Without a plan or program it is the fused ``"minmax"`` launch, whose bits it
    shares; uint8 images raise ``TypeError``.

    ``resample_verts`` re-samples the point cloud from the FULL-size warped mask (``:255-263``); the mask is written by the
    same launch (``fused_mask``) or by a second launch of the kernel over the full image.  Otherwise ``verts`` (integer
    vertices stored with the data set) are only scaled.  The augmentation adds no host synchronisation; the sampler's one
    ``counts.max()`` is its own.

    ``photometric``: a ``PhotoProgram`` applied to the uint8 images in front of the warp (``photometric_aug``: the
    photometric part of ``augmentation2``, ``data_generator_mscmrseg.py:87-132``); masks and vertices are untouched by it.  fp32
    images (``rescale="minmax"``) with a program raise ``TypeError``; ``rescale="minmax_u8"`` is the way in for them.

    ``heavy``: a ``HeavyPlan`` (``sample_heavy_plan``: the reference's default ``augmentation``, ``data_generator_mscmrseg.py:20-84``)
    run on the uint8 images AND the masks in front of everything else (``heavy_aug``); with ``resample_verts`` the point
    cloud is drawn from the full-size warped mask, as without a plan.  fp32 images with a plan raise ``TypeError`` unless
    ``rescale="minmax_u8"`` quantises them first.

    ``match_hist``: a ``HistReference``; the raw images (fp32 or uint8) are histogram-matched against it before anything else
    (``match_histograms``: ``data_generator_mmwhs.py:236-237``, the generator's ``-mh``), so the batch min / max of
    ``rescale="minmax"`` are those of the matched images and a heavy plan or a photometric program sees the matched uint8
    images; masks and vertices are untouched.  ``params=None, rescale=None`` is then the generator's ``aug=''`` branch.  With a
    ``HistReferenceBank`` sample ``i`` is matched to reference ``match_hist_index[i]`` (``match_histograms``' ``index``: a host
    sequence, an int32 device tensor, or ``None`` for a bank of ``B`` or of one).

    ``fourier``: a ``FourierBank``; the raw images (fp32 or uint8, of the bank's size and dtype) are adapted to the references
    ``fourier_index`` names (``fourier_adapt``: ``index`` and ``radius`` as there; index -1 passes a sample through) after
    ``match_hist`` and before everything else, so the min-max rescale, a heavy plan and a photometric program see the adapted
    images; masks and vertices are untouched.  fp32 results are not clipped."""
    _check_rescale("augment_batch", rescale)
    if match_hist is not None:
        images_hwc = match_histograms(images_hwc, match_hist, index=match_hist_index)
    elif match_hist_index is not None:
        raise TypeError("augment_batch: match_hist_index goes with match_hist (a HistReferenceBank)")
    if fourier is not None:
        images_hwc = fourier_adapt(images_hwc, fourier, index=fourier_index, radius=fourier_radius)
    elif fourier_index is not None or fourier_radius is not None:
        raise TypeError("augment_batch: fourier_index and fourier_radius go with fourier (a FourierBank)")
    mm = None
    if rescale == "minmax_u8":
        if images_hwc.dtype != torch.float32:
            raise TypeError("augment_batch: the min-max rescale takes fp32 images")
        if heavy is not None or photometric is not None:      # (without uint8 stages the fused "minmax" launch: same bits)
            images_hwc, mm = quantize_minmax(images_hwc)
    if heavy is not None:
        if rescale == "minmax" or images_hwc.dtype != torch.uint8:
            raise TypeError("augment_batch: a heavy plan takes uint8 images (rescale='div255' or None)")
        images_hwc, masks = heavy_aug(images_hwc, masks, heavy)
    lab = as_labels(masks)
    b, h, w, _ = images_hwc.shape
    dev = images_hwc.device
    if photometric is not None:
        if rescale == "minmax" or images_hwc.dtype != torch.uint8:
            raise TypeError("augment_batch: a photometric program takes uint8 images (rescale='div255' or None)")
        images_hwc = photometric_aug(images_hwc, photometric)
    inv, order, cval = upload_params(params, b, h, w, dev)
    if mm is not None:
        mode = None      # quantised above: the dequantising assemble
    elif rescale in ("minmax", "minmax_u8"):
        if images_hwc.dtype != torch.float32:
            raise TypeError("augment_batch: the min-max rescale takes fp32 images")
        mode, mm = K.AUG_MINMAX, K.minmax(images_hwc)
    elif rescale == "div255":
        if images_hwc.dtype != torch.uint8:
            raise TypeError("augment_batch: the /255 rescale takes uint8 images")
        mode = K.AUG_DIV255
    else:
        mode = K.AUG_NONE

    def assemble(**want):
        if mode is None:
            return K.augment_assemble_dequant(images_hwc, lab, inv, order, cval, mm, num_classes, crop_size, **want)
        return K.augment_assemble(images_hwc, lab, inv, order, cval, num_classes, crop_size, mode, mm, **want)
    out = assemble(want_full_mask=resample_verts and fused_mask)
    if resample_verts:
        full = out["full_mask"] if fused_mask else assemble(want_images=False, want_onehot=False, want_full_mask=True)["full_mask"]
        if firsts is None:
            firsts = torch.zeros(b, dtype=torch.int32, device=dev)
        verts = masks_to_pointclouds(full, firsts)
    v = None if verts is None else verts.to(torch.float32) / torch.full((), 255.0, dtype=torch.float32, device=verts.device)
    return out["images"], out["onehot"], v


def light_aug(images: torch.Tensor, masks: Optional[torch.Tensor] = None, params: Optional[AugmentParams] = None,
              segmap: bool = False):
    """``data_generator_mmwhs.py:87-122``: uint8 ``[B,H,W,C]`` images (and integer masks ``[B,H,W]`` / ``[B,H,W,1]``) on
    the device -> the warped uint8 images (and masks, same shape and dtype).  ``params`` is required: draw it with
    ``sample_params(B, "mmwhs_light", rng)``.  (``segmap`` only selects imgaug's container type in the reference.)"""
    if params is None:
        raise TypeError("light_aug: params is required (sample_params(batch, preset, rng)); there is no silent identity")
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise TypeError("light_aug: uint8 [B,H,W,C] images")
    b, h, w, _ = images.shape
    inv, order, cval = upload_params(params, b, h, w, images.device)
    lab = as_labels(masks)
    out = K.augment_assemble(images, lab, inv, order, cval, 2, 0, K.AUG_NONE, None, want_images=False, want_onehot=False,
                             want_labels=lab is not None, want_u8=True)
    if masks is None:
        return out["images_u8"]
    return out["images_u8"], like_masks(out["labels"], masks)


def simple_aug(image: torch.Tensor, mask: Optional[torch.Tensor], params: Optional[AugmentParams] = None):
    """``data_generator_mscmrseg.py:135-167``: as ``light_aug`` (preset ``"mscmrseg_simple"``), also for one ``[H,W,C]``
    image with its ``[H,W]`` / ``[H,W,1]`` mask."""
    if params is None:
        raise TypeError("simple_aug: params is required (sample_params(batch, preset, rng)); there is no silent identity")
    if image.dim() == 4:
        return light_aug(image, mask, params)
    if mask is None:
        return light_aug(image[None], None, params)[0]
    im, m = light_aug(image[None], mask[None], params)
    return im[0], m[0]


class AugmentedBatches:
    """Wraps a host iterator of raw ``(images [B,H,W,C], masks [B,H,W] or [B,H,W,1])`` batches (optionally with the stored
    integer vertices as a third item) and yields the ``(x [B,C,h,w] fp32, y [B,K,h,w] uint8 one-hot, z [B,300,3] fp32)``
    device tensors ``train_epoch`` consumes.  Raw batches go to the device one ahead through pinned staging buffers
    (``DeviceBatches``); the parameters of each batch are drawn from ``rng`` on the host and ride along through pinned,
    non-blocking copies.  ``last_params`` holds the parameters of the batch yielded last; with
    ``photometric_preset`` a ``PhotoProgram`` is drawn after them from the same ``rng`` (``last_program``) and applied to the
    uint8 images in front of the warp.  With ``heavy_preset`` (``"heavy_device"``, ``"mscmrseg_aug2_device"``, their ``_full_``,
    ``_refpad_``, ``_connected_`` or ``_scaled_`` twins) ``preset`` must
    be ``None``: a ``HeavyPlan`` is drawn per batch (``last_plan``) and the assembler gets identity parameters;
    ``heavy_interp="cubic"`` (f8b) draws it with ``sample_heavy_plan(.., interp="cubic")`` -- order-3 elastic warps and a share of
    cubic noise upscales, one more ``rng.random(B)`` per batch --, ``"linear"`` (the default) as before.  With
    ``match_hist_reference`` (an ``[H,W,C]`` numpy image) its tables are built and uploaded once (``match_hist``) and every batch
    is histogram-matched against it first.  With ``match_hist_bank`` (a ``HistReferenceBank``) every sample is matched to a
    reference drawn from the bank: ``rng.integers(R, size=B)`` is the FIRST draw of a batch (``last_match_index``), made only
    when a bank is given, so without one the generator is consumed exactly as before.  ``rescale="minmax_u8"`` (fp32 batches)
    goes with every kind of preset and consumes the generator draw for draw as ``"div255"`` does: with
    ``heavy_preset="heavy_refpad_device"`` it is the MM-WHS generator's ``-aug heavy`` branch.  With ``fourier_bank`` (a
    ``FourierBank``) every sample is adapted to a reference drawn from the bank, behind the histogram match: per batch, after the
    histogram-bank index draw where there is one, ``rng.integers(R, size=B)`` (``last_fourier_index``); if ``fourier_p < 1``,
    ``rng.random(B)``, and the index becomes -1 (the sample passes through) where the draw is ``>= fourier_p``; if
    ``fourier_radius_range = (lo, hi)`` is given, ``rng.integers(lo, hi + 1, size=B)`` (``last_fourier_radius``; otherwise the
    bank's radius).  Without a bank none of these draws is made."""

    def __init__(self, iterator: Iterable, device: torch.device, preset: str, rng: np.random.Generator, num_classes: int = 5,
                 crop_size: int = 0, rescale: Optional[str] = "minmax", resample_verts: bool = True, depth: int = 2,
                 photometric_preset: Optional[str] = None, heavy_preset: Optional[str] = None,
                 match_hist_reference: Optional[np.ndarray] = None, match_hist_bank: Optional[HistReferenceBank] = None,
                 heavy_interp: str = "linear", fourier_bank: Optional[FourierBank] = None, fourier_p: float = 1.0,
                 fourier_radius_range=None):
        _check_interp(heavy_interp)
        if fourier_bank is not None and not isinstance(fourier_bank, FourierBank):
            raise TypeError("AugmentedBatches: fourier_bank is a FourierBank")
        if fourier_bank is None and (fourier_p != 1.0 or fourier_radius_range is not None):
            raise ValueError("AugmentedBatches: fourier_p and fourier_radius_range go with fourier_bank")
        if not 0.0 <= float(fourier_p) <= 1.0:
            raise ValueError("AugmentedBatches: fourier_p in [0, 1], got %r" % (fourier_p,))
        if fourier_radius_range is not None:
            lo, hi = (int(v) for v in fourier_radius_range)
            if not 0 <= lo <= hi <= fourier_bank.radius:
                raise ValueError("AugmentedBatches: fourier_radius_range = (lo, hi) with 0 <= lo <= hi <= the bank's radius (%d), "
                                 "got %r" % (fourier_bank.radius, tuple(fourier_radius_range)))
            fourier_radius_range = (lo, hi)
        _check_rescale("AugmentedBatches", rescale)
        if match_hist_reference is not None and match_hist_bank is not None:
            raise ValueError("AugmentedBatches: match_hist_reference (one image for every sample) or match_hist_bank, not both")
        if match_hist_bank is not None and not isinstance(match_hist_bank, HistReferenceBank):
            raise TypeError("AugmentedBatches: match_hist_bank is a HistReferenceBank")
        if preset == "heavy" or photometric_preset == "heavy" or heavy_preset == "heavy":
            raise NotImplementedError(HEAVY_MESSAGE)
        if heavy_preset is not None:
            _check_preset(heavy_preset)
            if preset is not None or photometric_preset is not None:
                raise ValueError("AugmentedBatches: a heavy preset is the whole recipe (preset and photometric_preset must be None)")
            if rescale == "minmax":
                raise TypeError("AugmentedBatches: a heavy preset takes uint8 images (rescale='div255' or None)")
        elif preset not in _PRESETS:
            raise ValueError("unknown augmentation preset %r" % (preset,))
        if photometric_preset is not None and photometric_preset != PHOTOMETRIC_PRESET:
            raise ValueError("unknown photometric preset %r" % (photometric_preset,))
        if photometric_preset is not None and rescale == "minmax":
            raise TypeError("AugmentedBatches: a photometric preset takes uint8 images (rescale='div255' or None)")
        from .._epoch import DeviceBatches      # (imports the trainer: only when batches are actually wrapped)
        self.batches = DeviceBatches(iterator, device, depth)
        self.preset, self.rng = preset, rng
        self.num_classes, self.crop_size, self.rescale, self.resample_verts = num_classes, crop_size, rescale, resample_verts
        self.photometric_preset, self.heavy_preset, self.heavy_interp = photometric_preset, heavy_preset, heavy_interp
        self.match_hist = None if match_hist_reference is None else HistReference(match_hist_reference, device)
        self.match_hist_bank = match_hist_bank
        if match_hist_bank is not None:
            self.match_hist = match_hist_bank
        self.last_match_index: Optional[np.ndarray] = None
        self.fourier_bank, self.fourier_p, self.fourier_radius_range = fourier_bank, float(fourier_p), fourier_radius_range
        self.last_fourier_index: Optional[np.ndarray] = None
        self.last_fourier_radius: Optional[np.ndarray] = None
        self.last_plan: Optional[HeavyPlan] = None
        self.last_params: Optional[AugmentParams] = None
        self.last_program: Optional[PhotoProgram] = None

    def __iter__(self):
        return self

    def __next__(self):
        item = next(self.batches)
        images, masks = item[0], item[1]
        verts = item[2] if len(item) > 2 else None
        index = None
        if self.match_hist_bank is not None:
            index = self.last_match_index = self.rng.integers(self.match_hist_bank.size, size=images.shape[0])
        fda = {}
        if self.fourier_bank is not None:
            fidx = self.rng.integers(self.fourier_bank.size, size=images.shape[0])
            if self.fourier_p < 1.0:
                fidx = np.where(self.rng.random(images.shape[0]) >= self.fourier_p, -1, fidx)
            if self.fourier_radius_range is not None:
                lo, hi = self.fourier_radius_range
                self.last_fourier_radius = self.rng.integers(lo, hi + 1, size=images.shape[0])
            self.last_fourier_index = fidx
            fda = dict(fourier=self.fourier_bank, fourier_index=fidx, fourier_radius=self.last_fourier_radius)
        if self.heavy_preset is not None:
            self.last_params = AugmentParams.identity(images.shape[0])
            self.last_plan = sample_heavy_plan(images.shape[0], self.heavy_preset, self.rng, images.shape[1], images.shape[2],
                                               interp=self.heavy_interp)
            return augment_batch(images, masks, self.last_params, self.num_classes, self.crop_size, self.rescale,
                                 resample_verts=self.resample_verts, verts=verts, heavy=self.last_plan,
                                 match_hist=self.match_hist, match_hist_index=index, **fda)
        self.last_params = sample_params(images.shape[0], self.preset, self.rng)
        if self.photometric_preset is not None:
            self.last_program = sample_program(images.shape[0], self.photometric_preset, self.rng)
        return augment_batch(images, masks, self.last_params, self.num_classes, self.crop_size, self.rescale,
                             resample_verts=self.resample_verts, verts=verts, photometric=self.last_program,
                             match_hist=self.match_hist, match_hist_index=index, **fda)
