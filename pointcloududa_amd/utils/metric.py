"""Metrics of ``src/utils/metric.py`` on the device.

Per-step training metrics (``metric.py:5-36`` + ``src/utils/utils.py:32-40``), and the evaluation metrics the reference
takes from ``medpy.metric.binary``: ``dc``, ``hd`` and ``asd`` with medpy's signatures and definitions (and medpy's
``hd95`` and ``assd``, which the reference does not print but the field's tables do), and the reference's ``evaluate`` / ``metrics2`` (``metric.py:39-113``).  All of them run on the HIP kernels
(``kernels.surface_metrics``: border extraction, exact Euclidean distance transform, deterministic reductions); numpy
inputs are copied to the current device and the results come back as Python floats.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from .. import kernels as K

# medpy's messages (medpy.metric.binary.__surface_distances), raised for an empty first / second argument
EMPTY_FIRST = "The first supplied array does not contain any binary object."
EMPTY_SECOND = "The second supplied array does not contain any binary object."


def dice_coef_multilabel(y_true_onehot_u8: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """mean over labels 1..C-1 of (2|A.B|+1)/(|A|+|B|+1), with B = soft_to_hard_pred(logits)
    computed on the fly; returns a 0-dim device tensor (no host sync)."""
    return K.dice_metric(logits, y_true_onehot_u8)


def argmax_labels(x: torch.Tensor) -> torch.Tensor:
    """``np.argmax(soft_to_hard_pred(x, 1), axis=1)`` (``train_mscmrseg.py:85-87``) on the device: uint8 label map,
    first channel holding the per-pixel maximum.  Accepts fp32 logits or the uint8 one-hot ground truth."""
    return K.argmax_labels(x)


def label_dice(pred_labels: torch.Tensor, gt_labels: torch.Tensor, num_classes: int) -> torch.Tensor:
    """per-class Dice ``2|A.B|/(|A|+|B|)`` (0 when both are empty) of two label maps -- what ``evaluate``
    (``metric.py:39-82``) gets from ``medpy.metric.binary.dc`` for classes 1..3.  fp32 ``[num_classes]``."""
    return K.label_dice(pred_labels, gt_labels, num_classes)


# ------------------------------------------------------------------------------------------------ evaluation
def to_device(x, device=None) -> torch.Tensor:
    """a label volume (numpy array or tensor) as a device tensor; numpy goes to ``device`` or the current HIP device"""
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise RuntimeError("evaluation metrics need HIP device tensors or numpy arrays (no CPU fallback)")
        return x
    if not torch.cuda.is_available():
        raise RuntimeError("evaluation metrics run on a HIP device; none is available (no CPU fallback)")
    a = np.asarray(x)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    elif a.dtype not in (np.uint8, np.int32):
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError("integer label volumes only (got %s)" % a.dtype)
        a = np.clip(a, -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device or torch.device("cuda", torch.cuda.current_device()))


def _binary(x) -> torch.Tensor:
    """medpy's ``np.atleast_1d(x.astype(bool))`` as a uint8 device volume (class value 1)"""
    t = to_device(x)
    return (t != 0).to(torch.uint8)


def raise_if_empty(flags: float) -> None:
    """medpy's error for a class whose first (flag 1) or second (flag 2) array is empty"""
    f = int(flags)
    if f & 1:
        raise RuntimeError(EMPTY_FIRST)
    if f & 2:
        raise RuntimeError(EMPTY_SECOND)


def _pair(result, reference, voxelspacing, connectivity):
    r = K.surface_metrics(_binary(result), _binary(reference), [1], voxelspacing, connectivity)
    return r[0].tolist()                                  # one synchronisation


def dc(result, reference) -> float:
    """medpy.metric.binary.dc: 2|A.B| / (|A| + |B|), 0.0 when both are empty (A = result != 0, B = reference != 0)"""
    return _pair(result, reference, None, 1)[0]


def hd(result, reference, voxelspacing=None, connectivity=1) -> float:
    """medpy.metric.binary.hd: the symmetric Hausdorff distance between the borders of ``result`` and ``reference``
    (border = object minus its erosion with the ``connectivity`` footprint); RuntimeError if either is empty"""
    r = _pair(result, reference, voxelspacing, connectivity)
    raise_if_empty(r[7])
    return r[1]


def asd(result, reference, voxelspacing=None, connectivity=1) -> float:
    """medpy.metric.binary.asd: mean distance from each border voxel of ``result`` to the nearest border voxel of
    ``reference`` (directed); RuntimeError if either is empty"""
    r = _pair(result, reference, voxelspacing, connectivity)
    raise_if_empty(r[7])
    return r[2]


def _pair_ext(result, reference, voxelspacing, connectivity, percentile=95.0):
    r = K.surface_metrics_ext(_binary(result), _binary(reference), [1], voxelspacing, connectivity, percentile)
    return r[0].tolist()                                  # one synchronisation


def hd95(result, reference, voxelspacing=None, connectivity=1) -> float:
    """medpy.metric.binary.hd95: ``numpy.percentile`` (95, linear) of the surface distances of both directions pooled,
    result -> reference and reference -> result; RuntimeError if either is empty"""
    r = _pair_ext(result, reference, voxelspacing, connectivity)
    raise_if_empty(r[7])
    return r[8]


def assd(result, reference, voxelspacing=None, connectivity=1) -> float:
    """medpy.metric.binary.assd: the mean of ``asd(result, reference)`` and ``asd(reference, result)``; RuntimeError if
    either is empty"""
    r = _pair_ext(result, reference, voxelspacing, connectivity)
    raise_if_empty(r[7])
    return r[9]


def _gt_pred(img_gt, img_pred):
    gt, pred = to_device(img_gt), to_device(img_pred)
    if gt.dim() != pred.dim():
        raise ValueError("The arrays 'img_gt' and 'img_pred' should have the "
                         "same dimension, {} against {}".format(gt.dim(), pred.dim()))
    if pred.device != gt.device:
        pred = pred.to(gt.device)
    return gt, pred


def class_metrics(img_gt, img_pred, classes) -> torch.Tensor:
    """``surface_metrics(gt, pred, classes)`` on the device (no synchronisation): per class (dice, hd, asd(gt -> pred) =
    what medpy's ``asd(gt_c, pred_c)`` returns, ...), the argument order of the reference's ``dc(gt_c_i, pred_c_i)`` /
    ``hd(gt_c_i, pred_c_i)`` / ``asd(gt_c_i, pred_c_i)`` calls: flag 1 means an empty gt class (medpy's 'first')."""
    gt, pred = _gt_pred(img_gt, img_pred)
    return K.surface_metrics(gt, pred, classes)


def class_metrics_ext(img_gt, img_pred, classes, percentile=95.0) -> torch.Tensor:
    """``surface_metrics_ext(gt, pred, classes)`` on the device (no synchronisation), with ``class_metrics``' argument
    order: its eight columns, then the percentile distance (hd95), assd and the border counts of gt and pred"""
    gt, pred = _gt_pred(img_gt, img_pred)
    return K.surface_metrics_ext(gt, pred, classes, percentile=percentile)


def _named(img_gt, img_pred, classes, names, apply_hd, apply_asd):
    rows = class_metrics(img_gt, img_pred, classes).tolist()
    res = {}
    for row, name in zip(rows, names):
        h_d, a_sd = 0, 0
        if apply_hd or apply_asd:
            raise_if_empty(row[7])                         # (the reference's hd / asd call raises for this class)
        if apply_hd:
            h_d = row[1]
        if apply_asd:
            a_sd = row[2]
        res[name] = [row[0], h_d, a_sd]
    return res


def evaluate(img_gt, img_pred, apply_hd=False, apply_asd=False):
    """``metric.py:39-82``: {"myo": [dice, hd, asd], "lv": ..., "rv": ...} for the labels 1, 2, 3; hd / asd are 0 unless
    asked for, asd = medpy ``asd(gt, pred)``.  RuntimeError (medpy's) for an empty class when hd or asd is asked for."""
    return _named(img_gt, img_pred, [1, 2, 3], ["myo", "lv", "rv"], apply_hd, apply_asd)


def metrics2(img_gt, img_pred, apply_hd=False, apply_asd=False):
    """``metric.py:85-113``: the MM-WHS classes 1..4 as {"myo", "la", "lv", "aa"}, otherwise as ``evaluate``"""
    return _named(img_gt, img_pred, [1, 2, 3, 4], ["myo", "la", "lv", "aa"], apply_hd, apply_asd)
