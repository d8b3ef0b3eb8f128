"""The light augmentation's parameters and matrices: what ``sample_params`` draws for the reference's
``light_aug`` / ``simple_aug`` pipelines, and the one inverse 2x3 matrix per sample that ``csrc/augment.hip`` consumes.
``utils/augment.py`` states the sub-pixel convention and runs the kernel; ``GeoProgram.set_affine`` (``utils/geometric.py``) encodes
the heavy ``Affine`` through ``inverse_matrices``."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

from ._program import HEAVY_MESSAGE, upload

OP_FLIPLR, OP_FLIPUD, OP_AFFINE = 0, 1, 2

# (p_fliplr, p_flipud, p_affine): data_generator_mmwhs.py:89-94, data_generator_mscmrseg.py:136-142
_PRESETS = {"mmwhs_light": (0.2, 0.2, 0.3), "mscmrseg_simple": (0.3, 0.3, 0.45)}
# shared by both pipelines (data_generator_mmwhs.py:95-100, data_generator_mscmrseg.py:143-150)
SCALE = (0.8, 1.2)
TRANSLATE_X = (-0.1, 0.05)
TRANSLATE_Y = (-0.1, 0.1)
ROTATE = (-10.0, 10.0)
SHEAR = (-12.0, 12.0)


@dataclass
class AugmentParams:
    """Per-sample parameters (numpy arrays of length B) and the one application order of the batch: ``op_order`` lists
    ``OP_FLIPLR``, ``OP_FLIPUD``, ``OP_AFFINE`` in the order they are applied (``random_order=True`` draws one order per
    batch).  ``translate_*`` are fractions of the width / height, ``rotate`` and ``shear`` degrees."""
    flip_lr: np.ndarray
    flip_ud: np.ndarray
    affine_on: np.ndarray
    scale_x: np.ndarray
    scale_y: np.ndarray
    translate_x: np.ndarray
    translate_y: np.ndarray
    rotate: np.ndarray
    shear: np.ndarray
    order: np.ndarray
    cval: np.ndarray
    op_order: Tuple[int, int, int] = field(default=(OP_FLIPLR, OP_FLIPUD, OP_AFFINE))

    @property
    def batch(self) -> int:
        return len(self.flip_lr)

    @staticmethod
    def identity(batch: int) -> "AugmentParams":
        z, o = np.zeros(batch, dtype=np.float64), np.ones(batch, dtype=np.float64)
        f = np.zeros(batch, dtype=bool)
        i = np.zeros(batch, dtype=np.int64)
        return AugmentParams(f.copy(), f.copy(), f.copy(), o.copy(), o.copy(), z.copy(), z.copy(), z.copy(), z.copy(), i.copy(),
                             i.copy())

    def is_identity(self) -> bool:
        return not (np.any(self.flip_lr) or np.any(self.flip_ud) or np.any(self.affine_on))

    def validate(self) -> None:
        b = self.batch
        for name in ("flip_ud", "affine_on", "scale_x", "scale_y", "translate_x", "translate_y", "rotate", "shear", "order",
                     "cval"):
            if len(getattr(self, name)) != b:
                raise ValueError("AugmentParams.%s has %d entries, flip_lr has %d" % (name, len(getattr(self, name)), b))
        if sorted(int(o) for o in self.op_order) != [OP_FLIPLR, OP_FLIPUD, OP_AFFINE]:
            raise ValueError("AugmentParams.op_order must be a permutation of (0, 1, 2), got %r" % (tuple(self.op_order),))
        order, cval = np.asarray(self.order), np.asarray(self.cval)
        if np.any((order != 0) & (order != 1)):
            raise ValueError("AugmentParams.order must be 0 or 1")
        if np.any((cval < 0) | (cval > 255)) or np.any(cval != np.floor(cval)):
            raise ValueError("AugmentParams.cval must be an integer in [0, 255]")

    def kernel_arrays(self, h: int, w: int):
        return kernel_params(self, h, w)


def sample_params(batch: int, preset: str, rng: np.random.Generator) -> AugmentParams:
    """Draw the parameters of one batch.  ``preset``: ``"mmwhs_light"`` (flips 0.2 / 0.2, affine with p = 0.3) or
    ``"mscmrseg_simple"`` (0.3 / 0.3, p = 0.45); both: scale 0.8-1.2 per axis, translate x in (-0.1, 0.05) and y in
    (-0.1, 0.1), rotate +/-10, shear +/-12 degrees, order from {0, 1}, cval from 0..255, one operation order per batch.
    (imgaug's own parameter stream is not reproduced: parity unpinned.)"""
    if preset == "heavy":
        raise NotImplementedError(HEAVY_MESSAGE)
    if preset not in _PRESETS:
        raise ValueError("unknown augmentation preset %r (have: %s)" % (preset, ", ".join(sorted(_PRESETS))))
    p_lr, p_ud, p_aff = _PRESETS[preset]
    op_order = tuple(int(i) for i in rng.permutation(3))
    u = lambda lo_hi: rng.uniform(lo_hi[0], lo_hi[1], batch)
    return AugmentParams(flip_lr=rng.random(batch) < p_lr, flip_ud=rng.random(batch) < p_ud, affine_on=rng.random(batch) < p_aff,
                         scale_x=u(SCALE), scale_y=u(SCALE), translate_x=u(TRANSLATE_X), translate_y=u(TRANSLATE_Y),
                         rotate=u(ROTATE), shear=u(SHEAR), order=rng.integers(0, 2, batch), cval=rng.integers(0, 256, batch),
                         op_order=op_order)


def _translate(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]], dtype=np.float64)


def forward_matrices(params: AugmentParams, h: int, w: int) -> np.ndarray:
    """float64 ``[B,3,3]``: source pixel (x, y, 1) -> output pixel, the operations multiplied in application order."""
    params.validate()
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    out = np.empty((params.batch, 3, 3), dtype=np.float64)
    for i in range(params.batch):
        m = np.eye(3, dtype=np.float64)
        for op in params.op_order:
            if op == OP_FLIPLR and params.flip_lr[i]:
                m = np.array([[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ m
            elif op == OP_FLIPUD and params.flip_ud[i]:
                m = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]]) @ m
            elif op == OP_AFFINE and params.affine_on[i]:
                r, s = math.radians(float(params.rotate[i])), math.radians(float(params.shear[i]))
                rot = np.array([[math.cos(r), -math.sin(r), 0.0], [math.sin(r), math.cos(r), 0.0], [0.0, 0.0, 1.0]])
                sh = np.array([[1.0, math.tan(s), 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
                sc = np.diag([float(params.scale_x[i]), float(params.scale_y[i]), 1.0])
                a = _translate(cx + float(params.translate_x[i]) * w, cy + float(params.translate_y[i]) * h) @ rot @ sh @ sc \
                    @ _translate(-cx, -cy)
                m = a @ m
        out[i] = m
    return out


def inverse_matrices(params: AugmentParams, h: int, w: int) -> np.ndarray:
    """float64 ``[B,2,3]``: output pixel (x, y) -> source coordinate, what the kernel consumes.  A singular map (a zero
    scale, a 90 degree shear) raises ``ValueError``."""
    fwd = forward_matrices(params, h, w)
    out = np.empty((params.batch, 2, 3), dtype=np.float64)
    for i, m in enumerate(fwd):
        det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
        if not np.all(np.isfinite(m)) or not abs(det) > 1e-12:
            raise ValueError("augmentation matrix of sample %d is singular (determinant %r)" % (i, det))
        out[i] = np.linalg.inv(m)[:2]
    return out


def kernel_params(params: AugmentParams, h: int, w: int):
    """(inverse matrices float64 [B,2,3], order int32 [B], cval int32 [B]) as the kernel takes them: ``order`` and ``cval``
    only matter where an affine is applied (a flip maps integer pixels to integer pixels), so they are 0 elsewhere."""
    inv = inverse_matrices(params, h, w)
    on = np.asarray(params.affine_on, dtype=bool)
    order = np.where(on, np.asarray(params.order), 0).astype(np.int32)
    cval = np.where(on, np.asarray(params.cval), 0).astype(np.int32)
    return inv, order, cval


def upload_params(params: Optional[AugmentParams], batch: int, h: int, w: int, device: torch.device):
    """Validate on the host, then move the kernel's parameter arrays through pinned, non-blocking copies (no
    synchronisation)."""
    return upload(AugmentParams.identity(batch) if params is None else params, batch, h, w, device=device)
