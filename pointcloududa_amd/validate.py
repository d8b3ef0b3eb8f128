"""Validation / inference forward of the segmenter on the HIP kernels.

Mirrors ``valid_model_with_one_dataset`` (``src/train_mscmrseg.py:53-99``): eval-mode forward (BatchNorm folded
from its running statistics), BCE + Jaccard (+ point NN) loss, hard labels, per-class Dice -- with every
per-batch quantity kept on the device (one synchronisation per data set instead of three per batch).  ``hd=True`` adds
the reference's Hausdorff distance (medpy ``hd`` through ``evaluate`` / ``metrics2``) from the HIP surface-metric kernels;
``evaluate_volume`` is the device-side core of the evaluate scripts (forward, argmax, largest components, dice / hd /
asd)."""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import evaluate_mmwhs as EW
from . import evaluate_mscmrseg as EM
from . import kernels as K
from .utils import loss as L
from .utils import metric as M
from .utils import utils as U

# the classes of ``evaluate`` (MS-CMRSeg) / ``metrics2`` (MM-WHS), and the order in which the validation loops add their
# hd values: (lv + myo + rv) / 3 (train_mscmrseg.py:91), (lv + myo + la + aa) / 4 (train_mmwhs.py:90)
_HD_CLASSES = {"mscmrseg": [1, 2, 3], "mmwhs": [1, 2, 3, 4]}
_HD_ORDER = {"mscmrseg": [1, 0, 2], "mmwhs": [2, 0, 1, 3]}


@torch.no_grad()
def predict_labels(seg_model, x: torch.Tensor) -> torch.Tensor:
    """``evaluate_segmentation``'s core (``evaluate_mscmrseg.py:132-145``): eval forward -> uint8 label map."""
    was_training = seg_model.training
    seg_model.eval()
    try:
        out = seg_model(x)
        logits = out[0] if isinstance(out, tuple) else out
        return M.argmax_labels(logits)
    finally:
        seg_model.train(was_training)


@torch.no_grad()
def valid_batch(seg_model, x: torch.Tensor, y_onehot_u8: torch.Tensor, z: Optional[torch.Tensor] = None,
                d4: bool = True, variant: str = "mscmrseg", softmax: bool = True, hd: bool = False,
                dice: str = "") -> Dict[str, torch.Tensor]:
    """One iteration of the reference's validation loop; ``seg_model`` must be in eval mode.  Returns device scalars.
    ``variant="mscmrseg"`` (``train_mscmrseg.py:67-92``): loss = BCE + Jaccard + point NN loss (l1 + l2 + l3), vert_loss
    (l3 or -1), dice = mean of classes 1..3.  ``variant="mmwhs"`` (``train_mmwhs.py:65-90``): l1 = double-softmax CE
    (``softmax``) or BCE, loss = l1 + l2 WITHOUT the point term (:82), dice = mean of classes 1..4 (``metrics2``).
    ``hd``: also "hd_rows", the fp64 ``surface_metrics(gt, pred)`` rows of those classes with the batch's label maps
    taken as one [B,H,W] volume (column 1: hd, column 7: empty flags).  ``dice``: "" (l2 = Jaccard), "class" or "sample":
    the Dice term of ``TrainCfg.dice`` in its place."""
    prediction, _, vert_s = seg_model(x)
    ms = variant == "mscmrseg"
    l1, l2 = L.seg_loss(prediction, y_onehot_u8, "sigmoid" if (ms or not softmax) else "softmax", L.overlap_for(dice))
    loss = l1 + l2
    if d4 and vert_s is not None and z is not None:
        vert = L.batch_NN_loss(vert_s, z)
        if ms:
            loss = loss + vert
    else:
        vert = torch.full((), -1.0, dtype=torch.float32, device=x.device)
    c = prediction.shape[1]
    pred_lab, gt_lab = M.argmax_labels(prediction), M.argmax_labels(y_onehot_u8)
    dc = M.label_dice(pred_lab, gt_lab, c)
    r = {"loss": loss, "vert_loss": vert, "dice": dc[1:(4 if ms else 5)].mean(), "dice_per_class": dc}
    if hd:
        r["hd_rows"] = K.surface_metrics(gt_lab, pred_lab, _HD_CLASSES[variant])
    return r


def valid_model_with_one_dataset(seg_model, batches: Iterable, d4: bool = True, variant: str = "mscmrseg",
                                 softmax: bool = True, hd: bool = False, dice: str = "") -> Dict[str, float]:
    """``train_mscmrseg.py:53-99``: means over the batches of dice / loss / valid_vert_loss.  ``batches`` yields
    ``(x, y_onehot_u8, z)`` device tensors.  ``hd=True`` adds "hd": the mean over the batches of the mean over the
    classes of medpy ``hd(gt, pred)``; a class empty on either side of any batch raises medpy's RuntimeError at the
    data set's one synchronisation (the reference raises at that batch)."""
    was_training = seg_model.training
    seg_model.eval()
    acc = {"dice": [], "loss": [], "vert_loss": []}
    rows = []
    try:
        for x, y, z in batches:
            r = valid_batch(seg_model, x, y, z, d4, variant, softmax, hd, dice)
            for k in acc:
                acc[k].append(r[k])
            if hd:
                rows.append(r["hd_rows"])
    finally:
        seg_model.train(was_training)
    if not acc["dice"]:
        out = {"dice": float("nan"), "loss": float("nan"), "valid_vert_loss": float("nan")}
        if hd:
            out["hd"] = float("nan")
        return out
    means = torch.stack([torch.stack(acc[k]).mean() for k in ("dice", "loss", "vert_loss")])
    if not hd:
        means = means.tolist()   # one sync
        return {"dice": means[0], "loss": means[1], "valid_vert_loss": means[2]}
    host = torch.cat([means.double(), torch.stack(rows).flatten()]).tolist()       # one sync
    ncls = len(_HD_CLASSES[variant])
    hd_list = []
    for b in range(len(rows)):
        cls_rows = [host[3 + (b * ncls + k) * 8:3 + (b * ncls + k + 1) * 8] for k in range(ncls)]
        for row in cls_rows:
            M.raise_if_empty(row[7])
        hd_list.append(sum(cls_rows[k][1] for k in _HD_ORDER[variant]) / float(ncls))
    return {"dice": host[0], "loss": host[1], "valid_vert_loss": host[2], "hd": float(np.mean(np.array(hd_list)))}


def _native_size(name, native_shape, variant):
    """``native_shape = (X, Y)``, the first two axes of the label file -> the (rows, columns) = (Y, X) of a predicted slice"""
    if native_shape is None:
        return None
    if variant != "mscmrseg":
        raise ValueError("%s: native_shape is the resize of evaluate_mscmrseg.py (variant='mscmrseg')" % name)
    if len(native_shape) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in native_shape):
        raise ValueError("%s: native_shape = (X, Y), two positive integers, got %r" % (name, native_shape))
    return int(native_shape[1]), int(native_shape[0])


def _predict_volume(seg_model, x, bs, dev, native, crop_size, origin_size):
    """eval forward in batches of ``bs`` -> uint8 labels: ``argmax`` at the network's size, or with ``native = (rows, columns)``
    the fused ``reconstuct_volume`` / ``resize_volume`` / ``argmax`` of ``evaluate_mscmrseg.py:139-145``"""
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    x = x.to(dev)
    was_training = seg_model.training
    seg_model.eval()
    try:
        preds = []
        for i in range(0, x.shape[0], bs):
            out = seg_model(x[i:i + bs])
            logits = out[0] if isinstance(out, tuple) else out
            if native is None:
                preds.append(M.argmax_labels(logits))
            else:
                preds.append(K.reconstruct_resize_argmax(logits, native[0], native[1], crop_size, origin_size))
    finally:
        seg_model.train(was_training)
    return torch.cat(preds)


@torch.no_grad()
def evaluate_volume(seg_model, x, gt_labels, bs: int = 8, klc: bool = True, ifhd: bool = True, ifasd: bool = True,
                    variant: str = "mmwhs", extended: bool = False, native_shape=None, crop_size: int = 112,
                    origin_size: int = 256):
    """The device-side core of ``evaluate_segmentation`` (``evaluate_mmwhs.py:118-132``; ``evaluate_mscmrseg.py:132-169``;
    its resize with ``native_shape``): eval forward in batches of ``bs`` -> argmax -> ``keep_largest_connected_components``
    (``klc``) -> the variant's ``metrics`` list ([dice, hd, asd] per class), with one synchronisation per volume.
    ``x``: the volume's slices [Z,C,H,W] (fp32, device tensor or numpy); ``gt_labels``: its label volume [Z,H,W] (MM-WHS
    1..4; MS-CMRSeg codes 200 / 500 / 600, which the predicted labels 1 / 2 / 3 are mapped to after ``klc``).
    ``extended``: [dice, hd, asd, hd95, assd] per class (``metrics_from_rows_ext``) from the one call per volume to the
    extended kernel; the first three are the bits the default call returns.
    ``native_shape=(X, Y)`` (``variant="mscmrseg"``): the tail of ``evaluate_mscmrseg.py:139-153`` at the label file's own size:
    the logits pasted at ``origin_size // 2 +- crop_size`` of a zero ``origin_size`` canvas, every class plane resized to ``X``
    columns by ``Y`` rows (``resize_volume``, the build's INTER_AREA rule: DESIGN.md f15) and ``argmax``, in one kernel that
    writes the labels ``[Z,Y,X]`` only; then ``klc``, the codes and the metrics against ``gt_labels [Z,Y,X]``
    (``evaluate_mscmrseg.read_labels``).  With the default ``None`` nothing is resized."""
    if variant not in ("mmwhs", "mscmrseg"):
        raise ValueError("evaluate_volume: variant 'mmwhs' or 'mscmrseg'")
    dev = next(seg_model.parameters()).device
    pred = _predict_volume(seg_model, x, bs, dev, _native_size("evaluate_volume", native_shape, variant), crop_size, origin_size)
    if klc:
        pred = U.keep_largest_connected_components(pred)
    mod = EW if variant == "mmwhs" else EM
    if variant == "mscmrseg":
        pred = EM.codes_table(dev)[pred.long()]      # (uploaded once per device: an upload makes the host wait)
    if extended:
        rows = M.class_metrics_ext(M.to_device(gt_labels, dev), pred, mod.CLASSES).tolist()    # one sync
        return mod.metrics_from_rows_ext(rows, ifhd, ifasd)
    rows = M.class_metrics(M.to_device(gt_labels, dev), pred, mod.CLASSES).tolist()        # one sync
    return mod.metrics_from_rows(rows, ifhd, ifasd)


@torch.no_grad()
def evaluate_volume_rows(seg_model, x, gt_labels, bs: int = 8, klc: bool = True, variant: str = "mmwhs", extended: bool = False,
                         native_shape=None, crop_size: int = 112, origin_size: int = 256):
    """``evaluate_volume`` up to its synchronisation: the same stages on the same kernels, returning the DEVICE rows
    (``M.class_metrics`` / ``M.class_metrics_ext`` of the variant's classes, float64) that ``metrics_from_rows`` /
    ``metrics_from_rows_ext`` turn into ``evaluate_volume``'s list.  Nothing synchronises, so a loop over patients can keep its
    rows on the device and read them all at once (``evaluate_mmwhs.evaluate_segmentation``,
    ``evaluate_mscmrseg.evaluate_segmentation``).  ``native_shape``, ``crop_size``, ``origin_size``: as in ``evaluate_volume``."""
    if variant not in ("mmwhs", "mscmrseg"):
        raise ValueError("evaluate_volume_rows: variant 'mmwhs' or 'mscmrseg'")
    dev = next(seg_model.parameters()).device
    pred = _predict_volume(seg_model, x, bs, dev, _native_size("evaluate_volume_rows", native_shape, variant), crop_size, origin_size)
    if klc:
        pred = U.keep_largest_connected_components(pred)
    mod = EW if variant == "mmwhs" else EM
    if variant == "mscmrseg":
        pred = EM.codes_table(dev)[pred.long()]      # (uploaded once per device: an upload makes the host wait)
    if extended:
        return M.class_metrics_ext(M.to_device(gt_labels, dev), pred, mod.CLASSES)
    return M.class_metrics(M.to_device(gt_labels, dev), pred, mod.CLASSES)
