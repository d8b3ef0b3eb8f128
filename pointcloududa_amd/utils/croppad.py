"""Device-side CropAndPad with every defined mode of ``numpy.pad``: the reference's
``iaa.CropAndPad(percent=(-0.05, 0.1), pad_mode=ia.ALL, pad_cval=(0, 255))`` of both heavy recipes
(``src/data_generator_mscmrseg.py:28-32, 91-95``; the MM-WHS generator's copy of ``augmentation``) as a per-sample PROGRAM that
one HIP entry point (``csrc/croppad.hip``) runs over uint8 ``[B,H,W,C]`` images and integer masks.  ``ia.ALL`` is ``constant``,
``edge``, ``linear_ramp``, ``maximum``, ``mean``, ``median``, ``minimum``, ``reflect``, ``symmetric``, ``wrap``; ``GeoProgram``'s
``set_crop_and_pad`` (f8) knows five of them and keeps what it does.

A program holds ``opcode`` int32 ``[B]`` (``OP_COPY``, ``OP_CROP_AND_PAD``) and ``iarg`` int32 ``[B,6]`` = (top, right, bottom, left,
mode, cval): signed pixels per side in ``set_crop_and_pad``'s order, positive pads, negative crops; ``mode`` indexes
``MODE_NAMES``; ``cval`` 0..255.  For a live sample with image ``x``:

1. the negative sides crop: ``xc = x[ct:H-cb, cl:W-cr]``
2. ``I = numpy.pad(xc, ((pt, pb), (pl, pr), (0, 0)), mode)`` with ``constant_values=cval`` (``constant``) or ``end_values=cval``
   (``linear_ramp``; imgaug's rule, ``pad_cval`` serves both), the statistics over the whole axis -- numpy's own output bit for
   bit (``tests/golden/croppad.npz``, ``scripts/make_croppad_golden.py``), including the axis order (axis 0 first, axis 1 on the
   padded array: corners are statistics of statistics and ramps of ramps), ``numpy.round`` of mean and median, and both forms
   of ``linspace`` behind ``linear_ramp``
3. ``I`` (``Hi x Wi``) is resized back to ``H x W`` by this build's order-1 rule in ``I``'s frame: ``sx = (x + 0.5) (Wi / W) - 0.5`` in
   float64, neighbours ``floor(sx)`` and ``floor(sx) + 1`` clamped into ``I``, summed in f6's order, ``floor(v + 0.5)`` clipped;
   ``Hi == H`` and ``Wi == W`` return ``I`` itself
4. masks take the same crop, constant 0 and the texel at ``floor(s + 0.5)``, whatever the image's mode is (f6's rule)

``I`` is never materialised.  imgaug's parameter stream is not reproduced (parity unpinned); the pad is numpy's."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import kernels as K
from ._program import as_labels, like_masks, upload

OP_COPY, OP_CROP_AND_PAD = 0, 1
(MODE_CONSTANT, MODE_EDGE, MODE_LINEAR_RAMP, MODE_MAXIMUM, MODE_MEAN, MODE_MEDIAN, MODE_MINIMUM, MODE_REFLECT, MODE_SYMMETRIC,
 MODE_WRAP) = range(10)
MODE_NAMES = ("CONSTANT", "EDGE", "LINEAR_RAMP", "MAXIMUM", "MEAN", "MEDIAN", "MINIMUM", "REFLECT", "SYMMETRIC", "WRAP")
IARGS = 6
MAX_PAD = 64


@dataclass
class CropPadProgram:
    """``opcode`` int32 ``[B]``, ``iarg`` int32 ``[B,6]`` (numpy, on the host; the module docstring says what they mean)."""
    opcode: np.ndarray
    iarg: np.ndarray

    @property
    def batch(self) -> int:
        return self.opcode.shape[0]

    @staticmethod
    def identity(batch: int) -> "CropPadProgram":
        return CropPadProgram(np.zeros(batch, dtype=np.int32), np.zeros((batch, IARGS), dtype=np.int32))

    def is_identity(self) -> bool:
        return not np.any(self.opcode != OP_COPY)

    def set_crop_and_pad(self, i, top, right, bottom, left, mode=MODE_CONSTANT, cval=0):
        """signed pixels per side, positive pads, negative crops; the output keeps its size"""
        self.opcode[i] = OP_CROP_AND_PAD
        self.iarg[i] = (int(top), int(right), int(bottom), int(left), int(mode), int(cval))

    def validate(self, h: int, w: int) -> None:
        """Raises ``ValueError`` for a program the kernel is not defined on: shapes and dtypes, an opcode outside {0, 1}, a mode
        outside 0..9, a cval outside 0..255, a cropped side below 2 pixels, a pad above ``min(64, cropped size - 1)`` on its
        axis; ``h`` or ``w`` below 2."""
        op, ia = self.opcode, self.iarg
        if getattr(op, "ndim", 0) != 1 or op.dtype != np.int32:
            raise ValueError("CropPadProgram.opcode must be int32 [B]")
        if getattr(ia, "shape", None) != (op.shape[0], IARGS) or ia.dtype != np.int32:
            raise ValueError("CropPadProgram.iarg must be int32 [B,%d]" % IARGS)
        if np.any((op != OP_COPY) & (op != OP_CROP_AND_PAD)):
            raise ValueError("CropPadProgram.opcode: unknown opcode")
        if h < 2 or w < 2:
            raise ValueError("CropPadProgram: H and W must be at least 2")
        a = ia[op == OP_CROP_AND_PAD].astype(np.int64)
        if np.any((a[:, 4] < 0) | (a[:, 4] > MODE_WRAP)):
            raise ValueError("CropPadProgram: mode must be in 0..9")
        if np.any((a[:, 5] < 0) | (a[:, 5] > 255)):
            raise ValueError("CropPadProgram: cval must be in 0..255")
        crop, pad = np.maximum(-a[:, :4], 0), np.maximum(a[:, :4], 0)
        hc, wc = h - crop[:, 0] - crop[:, 2], w - crop[:, 1] - crop[:, 3]
        if np.any(hc < 2) or np.any(wc < 2):
            raise ValueError("CropPadProgram: the crop must leave at least 2 pixels on each axis")
        if np.any(np.maximum(pad[:, 0], pad[:, 2]) > np.minimum(MAX_PAD, hc - 1)) or \
                np.any(np.maximum(pad[:, 1], pad[:, 3]) > np.minimum(MAX_PAD, wc - 1)):
            raise ValueError("CropPadProgram: a pad must be at most min(%d, cropped size - 1) on its axis" % MAX_PAD)

    def kernel_arrays(self, h: int, w: int):
        """(opcode, iarg) as the kernel takes them, validated for an ``h x w`` image"""
        self.validate(h, w)
        return self.opcode, self.iarg

    def apply(self, images, masks):
        return crop_pad_aug(images, masks, self)


def upload_crop_pad_program(program: CropPadProgram, batch: int, h: int, w: int, device: torch.device):
    """Validate on the host, then move the kernel's arrays through pinned, non-blocking copies (no synchronisation)."""
    return upload(program, batch, h, w, device=device)


def crop_pad_aug(images: torch.Tensor, masks: Optional[torch.Tensor], program: Optional[CropPadProgram] = None, out=None):
    """uint8 ``[B,H,W,C]`` images and integer masks ``[B,H,W]`` / ``[B,H,W,1]`` (or ``None``) on the device -> ``(images, masks of
    the same shape and dtype)``, new tensors (``out``: a uint8 tensor for the images).  ``program`` is required: build it with
    ``CropPadProgram.set_crop_and_pad`` or draw it inside ``sample_heavy_plan(B, "heavy_refpad_device", rng, H, W)``."""
    if program is None:
        raise TypeError("crop_pad_aug: program is required (CropPadProgram.identity(batch) and set_crop_and_pad); there is no "
                        "silent identity")
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise TypeError("crop_pad_aug: uint8 [B,H,W,C] images")
    b, h, w, _ = images.shape
    up = upload_crop_pad_program(program, b, h, w, images.device)
    res, lab_out = K.crop_pad(images, as_labels(masks), *up, out=out)
    return res, like_masks(lab_out, masks)
