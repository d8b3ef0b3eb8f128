"""The frame the device-side augmentation programs share: the slot-program base class of
``PhotoProgram``, ``GeoProgram`` and ``StyleProgram``, the pinned non-blocking upload, and the int32 view of a mask batch and its
inverse.  Imports numpy and torch only: every operator module (``photometric``, ``geometric``, ``stylize``, ``croppad``,
``histmatch``, ``affine``) is a leaf above it."""
from __future__ import annotations

import numpy as np
import torch

HEAVY_MESSAGE = ("The heavy pipeline (`augmentation`: Superpixels, median blur, elastic, piecewise affine, hue/saturation ...) "
                 "is out of scope.")
OP_NOP = 0


class SlotProgram:
    """``opcode`` int32 ``[B,S]``, the subclass's ``COLUMNS`` (``(name, dtype, width)``: ``[B,S,width]`` each) and ``seed`` uint64
    ``[B,S]``, numpy arrays on the host.  A subclass is a ``@dataclass`` whose fields are ``opcode``, its columns in ``COLUMNS``'
    order, ``seed``; opcode 0 is its NOP."""
    COLUMNS = ()
    MAX_SLOTS = 8
    SLOTS = 1                  # identity()'s default

    @property
    def batch(self) -> int:
        return self.opcode.shape[0]

    @property
    def slots(self) -> int:
        return self.opcode.shape[1]

    @classmethod
    def identity(cls, batch: int, slots: int = None):
        slots = cls.SLOTS if slots is None else slots
        return cls(np.zeros((batch, slots), dtype=np.int32), *(np.zeros((batch, slots, n), dtype=dt) for _, dt, n in cls.COLUMNS),
                   np.zeros((batch, slots), dtype=np.uint64))

    def is_identity(self) -> bool:
        return not np.any(self.opcode != OP_NOP)

    def _clear(self, i, s, op):
        self.opcode[i, s] = op
        for name, _, _ in self.COLUMNS:
            getattr(self, name)[i, s] = 0
        self.seed[i, s] = 0

    def set_nop(self, i, s):
        self._clear(i, s, OP_NOP)

    def _check_arrays(self, max_op: int) -> None:
        """the head of every ``validate``: shapes and dtypes, the slot count, the opcode range, finite ``farg`` / ``table``"""
        cls, op = type(self).__name__, self.opcode
        if getattr(op, "ndim", 0) != 2 or op.dtype != np.int32:
            raise ValueError("%s.opcode must be int32 [B,S]" % cls)
        b, s = op.shape
        if s > self.MAX_SLOTS:
            raise ValueError("%s: %d slots, at most %d" % (cls, s, self.MAX_SLOTS))
        for name, dt, n in self.COLUMNS + (("seed", np.uint64, None),):
            a, shape = getattr(self, name), (b, s) if n is None else (b, s, n)
            if getattr(a, "shape", None) != shape or a.dtype != dt:
                raise ValueError("%s.%s must be %s %r" % (cls, name, np.dtype(dt).name, list(shape)))
        if np.any((op < 0) | (op > max_op)):
            raise ValueError("%s.opcode: unknown opcode" % cls)
        for name, dt, _ in self.COLUMNS:
            if dt is np.float64 and not np.all(np.isfinite(getattr(self, name))):
                raise ValueError("%s.%s must be finite" % (cls, name))


def to_device(arrays, device) -> tuple:
    """host numpy arrays -> device tensors through pinned, non-blocking copies (no synchronisation)"""
    pin = torch.device(device).type == "cuda"
    out = []
    for a in arrays:
        t = torch.from_numpy(np.ascontiguousarray(a))
        out.append((t.pin_memory() if pin else t).to(device, non_blocking=True))
    return tuple(out)


def upload(program, batch: int, *dims, device) -> tuple:
    """Validate on the host (``program.kernel_arrays(*dims)``), then move the kernel's arrays with ``to_device``."""
    if program.batch != batch:
        raise ValueError("%s for %d samples, batch of %d" % (type(program).__name__, program.batch, batch))
    return to_device(program.kernel_arrays(*dims), device)


def as_labels(masks):
    """integer masks ``[B,H,W]`` / ``[B,H,W,1]`` -> int32 ``[B,H,W]`` as the kernels take them (``None`` stays ``None``)"""
    if masks is None:
        return None
    if masks.dim() == 4 and masks.shape[-1] == 1:
        masks = masks[..., 0]
    return masks.to(torch.int32)


def like_masks(labels, masks):
    """the inverse of ``as_labels``: a kernel's int32 labels in the shape and dtype of ``masks`` (``None`` without masks)"""
    return None if masks is None else labels.to(masks.dtype).reshape(masks.shape)
