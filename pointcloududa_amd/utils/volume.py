"""Test volumes of the evaluate scripts on the device (``csrc/evalprep.hip``).

``src/evaluate_mmwhs.py:19-29`` turns a NIfTI volume ``[H,W,D]`` into the segmenter's input: ``np.moveaxis(img, 2, 0)[:, ::-1, ::-1]``,
the 2.5-D stack ``img[[i - 1, i, (i + 1) % D]]`` (``i - 1`` at ``i = 0`` is numpy's ``-1``, the last slice) as float32, and the mask
through ``to_categorical(.., 5)``, read back with ``argmax``; ``src/evaluate_mscmrseg.py:147`` takes the ground truth as ``nimg.T``.
Here each is one HIP entry point over one strided index map (``include/pcuda_hip.h``, ``pcuda_volume_slices``): the array is
read as it lies -- C order, Fortran order (what a NIfTI reader returns) or any permuted view are strides only -- once, and the
result is written along its own fastest axis.  ``restore_volume`` is the way back from a prediction ``[D,H,W]`` to the volume's
own axis order.  Nothing is computed but casts, so numpy pins every output bit for bit.

Not here: NIfTI and CSV file I/O (the caller brings the array), slice axes other than the one given by strides, windows other
than 1 and 3.  The ``INTER_AREA`` resize and ``reconstuct_volume`` of the MS-CMRSeg script live in ``csrc/area_resize.hip``
(``utils.utils.resize_volume``, ``evaluate_mscmrseg.evaluate_segmentation``)."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from .. import kernels as K

_NUMPY_DTYPES = (np.float32, np.float64, np.int16, np.uint8, np.int32)


def as_device_volume(vol, what: str = "volume", device=None) -> torch.Tensor:
    """A 3-D device tensor of ``vol``'s shape AND memory order.  A device tensor is returned as it is.  A numpy array is
    uploaded as it lies: its axes are sorted by stride, the (then C-contiguous) memory goes to the device in one copy and
    the result is permuted back, so a Fortran-ordered array is never made C-contiguous on the host.  Only an array that is
    contiguous in no axis order (a strided slice, a mirrored view) is copied on the host first, in its own axis order."""
    if torch.is_tensor(vol):
        if vol.dim() != 3:
            raise ValueError("%s: a 3-D volume, got %d dimensions" % (what, vol.dim()))
        if not vol.is_cuda:
            raise RuntimeError("%s: pointcloududa_amd kernels need HIP device tensors or numpy arrays (no CPU fallback)" % what)
        return vol
    if not isinstance(vol, np.ndarray):
        raise TypeError("%s: a device tensor or a numpy array, got %s" % (what, type(vol).__name__))
    if vol.ndim != 3:
        raise ValueError("%s: a 3-D volume, got %d dimensions" % (what, vol.ndim))
    if vol.dtype not in _NUMPY_DTYPES:
        raise TypeError("%s: a float32 / float64 / int16 / uint8 / int32 array, got %s" % (what, vol.dtype))
    if not torch.cuda.is_available():
        raise RuntimeError("%s: pointcloududa_amd kernels run on a HIP device; none is available (no CPU fallback)" % what)
    order = sorted(range(3), key=lambda a: -abs(vol.strides[a]))           # slowest axis first (stable for ties)
    lying = vol.transpose(order)
    if not lying.flags.c_contiguous or not lying.dtype.isnative:
        lying = np.ascontiguousarray(lying, dtype=lying.dtype.newbyteorder("="))
    t = torch.from_numpy(lying).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    inverse = [order.index(a) for a in range(3)]
    return t.permute(inverse)


def _flips(what: str, flip) -> Tuple[bool, bool]:
    try:
        fr, fc = flip
    except (TypeError, ValueError):
        raise TypeError("%s: flip is a pair (rows, columns), got %r" % (what, flip))
    return bool(fr), bool(fc)


def _axis(what: str, slice_axis) -> int:
    if isinstance(slice_axis, bool) or not isinstance(slice_axis, int) or not -3 <= slice_axis <= 2:
        raise ValueError("%s: slice_axis is one of the volume's three axes, got %r" % (what, slice_axis))
    return slice_axis % 3


def _check_dtype(what: str, vol, names: Sequence[str]):
    name = str(vol.dtype).replace("torch.", "")
    if name not in names:
        raise TypeError("%s: a %s volume, got %s" % (what, " / ".join(names), name))


def volume_slices(vol, slice_axis: int = 2, flip=(True, True), window: int = 3, out=None) -> torch.Tensor:
    """``np.moveaxis(vol, slice_axis, 0)`` with rows / columns mirrored where ``flip`` says so, as float32 ``[D,window,H,W]``:
    ``window=3`` is the reference's 2.5-D stack (channel ``k`` of sample ``i`` is slice ``(i + k - 1) mod D``, wrapping at both
    ends), ``window=1`` the reoriented slices.  ``vol``: a float32, float64, int16 or uint8 device tensor of any stride, or a numpy
    array (uploaded in its own memory order).  The defaults are ``read_img`` (``evaluate_mmwhs.py:22-27``)."""
    axis, (fr, fc) = _axis("volume_slices", slice_axis), _flips("volume_slices", flip)
    if window not in (1, 3):
        raise ValueError("volume_slices: window is 1 or 3, got %r" % (window,))
    if not isinstance(vol, (np.ndarray, torch.Tensor)):
        raise TypeError("volume_slices: a device tensor or a numpy array, got %s" % type(vol).__name__)
    _check_dtype("volume_slices", vol, ("float32", "float64", "int16", "uint8"))
    t = as_device_volume(vol, "volume_slices")
    return K.volume_slices(t.movedim(axis, 0), fr, fc, window, out=out)


def volume_labels(vol, slice_axis: int = 2, flip=(True, True), num_classes: int = 5, remap=(), onehot: bool = False,
                  check: bool = True, raw: bool = False):
    """The label volume in the slices' orientation: uint8 ``[D,H,W]`` -- what ``np.argmax(to_categorical(mask, num_classes), 1)``
    gives (``evaluate_mmwhs.py:24,28,132``) -- after the ``(from, to)`` pairs of ``remap`` in order; with ``onehot`` also the uint8
    one-hot ``[D,K,H,W]`` from the same pass: ``(labels, onehot)``.  ``vol``: uint8, int16, int32, float32 or float64 (label files
    come back as floating point), device tensor of any stride or numpy array.  A value that is no integer in ``[0, num_classes)``
    after the remap is written as background and counted on the device: with ``check`` the count is read (one synchronisation)
    and a ``ValueError`` names it, where the reference's ``to_categorical`` asserts; ``check=False`` never synchronises.
    ``raw``: int32 ``[D,H,W]`` holding the values themselves, no remap and no range check (MS-CMRSeg's 200 / 500 / 600)."""
    axis, (fr, fc) = _axis("volume_labels", slice_axis), _flips("volume_labels", flip)
    if not isinstance(vol, (np.ndarray, torch.Tensor)):
        raise TypeError("volume_labels: a device tensor or a numpy array, got %s" % type(vol).__name__)
    _check_dtype("volume_labels", vol, ("uint8", "int16", "int32", "float32", "float64"))
    if raw and (onehot or len(tuple(remap))):
        raise ValueError("volume_labels: raw output takes no remap and has no one-hot form")
    if not raw:
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 255:
            raise ValueError("volume_labels: 2..255 classes, got %r" % (num_classes,))
        try:
            remap = tuple((int(a), int(b)) for a, b in remap)
        except (TypeError, ValueError):
            raise TypeError("volume_labels: remap is a sequence of (from, to) pairs, got %r" % (remap,))
        if len(remap) > 8:
            raise ValueError("volume_labels: a remap table of at most 8 (from, to) pairs, got %d" % len(remap))
    t = as_device_volume(vol, "volume_labels")
    lab, hot, counter = K.volume_labels(t.movedim(axis, 0), fr, fc, num_classes, remap, onehot, raw)
    if raw:
        return lab
    if check:
        stray = int(counter.item())
        if stray:
            raise ValueError("volume_labels: %d values of the volume are no integer in 0..%d after the remap %r (the reference's "
                             "to_categorical asserts)" % (stray, num_classes - 1, remap))
    return (lab, hot) if onehot else lab


def restore_volume(pred: torch.Tensor, like_shape, slice_axis: int = 2, flip=(True, True), transpose: bool = False, lut=None,
                   dtype=torch.uint8, fortran: bool = True) -> torch.Tensor:
    """The way back: a uint8 prediction ``[D,H,W]`` in the slices' orientation -> a tensor of shape ``like_shape`` in the volume's
    own axis order, so that ``volume_labels(restore_volume(p, shape, axis, flip), axis, flip) == p``.  ``transpose``: the
    orientation was ``vol.T`` (``evaluate_mscmrseg.py:147``) instead of ``moveaxis(vol, slice_axis, 0)``.  ``lut``: an int16 ``[256]``
    table (tensor or sequence) looked up first; ``dtype``: ``torch.uint8`` or ``torch.int16``.  ``fortran``: the result lies in memory
    with its FIRST axis fastest, as the volume a NIfTI reader returned does (``.cpu().numpy()`` keeps that order)."""
    axis, (fr, fc) = _axis("restore_volume", slice_axis), _flips("restore_volume", flip)
    if dtype not in (torch.uint8, torch.int16):
        raise TypeError("restore_volume: dtype is torch.uint8 or torch.int16, got %r" % (dtype,))
    try:
        shape = tuple(int(n) for n in like_shape)
    except (TypeError, ValueError):
        raise TypeError("restore_volume: like_shape is the volume's shape, got %r" % (like_shape,))
    if len(shape) != 3 or min(shape) < 0:
        raise ValueError("restore_volume: like_shape is a 3-D shape, got %r" % (like_shape,))
    if not torch.is_tensor(pred) or pred.dtype != torch.uint8 or pred.dim() != 3:
        raise TypeError("restore_volume: pred is a uint8 [D,H,W] device tensor, got %s" % (getattr(pred, "dtype", type(pred)),))
    want = shape[::-1] if transpose else (shape[axis],) + tuple(n for a, n in enumerate(shape) if a != axis)
    if tuple(pred.shape) != want:
        raise ValueError("restore_volume: pred %r does not fit a %r volume (expected %r)" % (tuple(pred.shape), shape, want))
    if lut is not None and not torch.is_tensor(lut):
        table = np.asarray(lut)
        if table.shape != (256,) or not np.issubdtype(table.dtype, np.integer) or table.min() < -32768 or table.max() > 32767:
            raise ValueError("restore_volume: lut is 256 int16 values")
        lut = torch.from_numpy(table.astype(np.int16))
    if not pred.is_cuda:
        raise RuntimeError("restore_volume: pointcloududa_amd kernels need HIP device tensors (no CPU fallback)")
    if lut is not None:
        lut = lut.to(pred.device)
    out = torch.empty(shape[::-1], dtype=dtype, device=pred.device).permute(2, 1, 0) if fortran else \
        torch.empty(shape, dtype=dtype, device=pred.device)
    K.volume_restore(pred, out.permute(2, 1, 0) if transpose else out.movedim(axis, 0), fr, fc, lut)
    return out
