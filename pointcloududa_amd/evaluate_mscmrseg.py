"""The metric functions of ``src/evaluate_mscmrseg.py`` on the device: ``compute_metrics_on_files`` (``metric.py:116-175``,
called at ``evaluate_mscmrseg.py:169``) on MS-CMRSeg label volumes (codes 500 = endo / LV, 600 = RV, 200 = myo).  The
file I/O of ``evaluate_segmentation`` (NIfTI, cv2 resize, pandas) is not part of this package; ``validate.evaluate_volume``
is its device-side core."""
from __future__ import annotations

import torch

from .utils import metric as M

CLASSES = [500, 600, 200]
FORMAT = "Endo {:>8} , {:>8} , {:>8} , RV {:>8} , {:>8} , {:>8} , Myo {:>8} , {:>8} , {:>8}"


def metrics_from_rows(rows, ifhd=True, ifasd=True):
    """the result list from ``M.class_metrics(gt, pred, CLASSES)`` rows (host lists): [dice, hd, asd] per class, with
    a -1 triplet for a class empty on either side when hd or asd is asked for; hd / asd are -1 when not asked for"""
    res = []
    for row in rows:
        dice, h_d, a_sd = row[0], -1, -1
        if ifhd or ifasd:
            if row[7]:
                dice, h_d, a_sd = -1, -1, -1
            else:
                h_d = row[1] if ifhd else h_d
                a_sd = row[2] if ifasd else a_sd
        res += [dice, h_d, a_sd]
    return res


def metrics_from_rows_ext(rows, ifhd=True, ifasd=True):
    """[dice, hd, asd, hd95, assd] per class from ``M.class_metrics_ext(gt, pred, CLASSES)`` rows, with the conventions of
    ``metrics_from_rows``: hd and hd95 go with ``ifhd``, asd and assd with ``ifasd``; -1 where not asked for, and five
    times -1 for a class empty on either side when any of them is asked for"""
    res = []
    for row in rows:
        vals = [row[0], -1, -1, -1, -1]
        if ifhd or ifasd:
            if row[7]:
                vals = [-1, -1, -1, -1, -1]
            else:
                if ifhd:
                    vals[1], vals[3] = row[1], row[8]
                if ifasd:
                    vals[2], vals[4] = row[2], row[9]
        res += vals
    return res


def metrics(img_gt, img_pred, ifhd=True, ifasd=True):
    """[Dice endo, HD endo, ASD endo, Dice RV, HD RV, ASD RV, Dice Myo, HD Myo, ASD Myo] (``metric.py:126-169``)"""
    return metrics_from_rows(M.class_metrics(img_gt, img_pred, CLASSES).tolist(), ifhd, ifasd)


def compute_metrics_on_files(gt, pred, ifhd=True, ifasd=True):
    """``metric.py:116-175``: ``metrics`` and the reference's printed line"""
    res = metrics(gt, pred, ifhd=ifhd, ifasd=ifasd)
    print(FORMAT.format(*["{:.3f}".format(r) for r in res]))
    return res


_CODES = [0, 200, 500, 600] + list(range(4, 256))
_codes_lut = {}      # device -> the int16 [256] table 1 / 2 / 3 -> 200 / 500 / 600 (uploaded once: an upload makes the host wait)


def read_labels(nimg):
    """The ground truth of ``evaluate_mscmrseg.py:147``: ``nimg.T`` -- a NIfTI label volume ``[X,Y,Z]`` (device tensor of any
    stride or numpy array, uploaded in its own memory order; uint8, int16, int32, float32 or float64) -> int32 ``[Z,Y,X]`` on the
    device with the codes 200 / 500 / 600 kept, what ``validate.evaluate_volume(.., variant="mscmrseg")`` takes.  No resize."""
    from . import kernels as K
    from .utils import volume as VOL
    t = VOL.as_device_volume(nimg, "read_labels")
    if t.dtype not in (torch.uint8, torch.int16, torch.int32, torch.float32, torch.float64):
        raise TypeError("read_labels: a uint8 / int16 / int32 / float32 / float64 volume, got %s" % (t.dtype,))
    return K.volume_labels(t.permute(2, 1, 0), raw=True)[0]


def restore_prediction(pred, nimg_shape):
    """A uint8 prediction ``[Z,Y,X]`` with labels 1 / 2 / 3 (at the network's resolution) -> int16 of shape ``nimg_shape`` =
    ``[X,Y,Z]``, in the file's axis order and memory order (first axis fastest), with the codes 200 / 500 / 600: the inverse of
    ``read_labels``' orientation.  No resize."""
    from .utils import volume as VOL
    if torch.is_tensor(pred) and pred.is_cuda and pred.device not in _codes_lut:
        _codes_lut[pred.device] = torch.tensor(_CODES, dtype=torch.int16).to(pred.device)
    lut = _codes_lut.get(getattr(pred, "device", None), _CODES)
    return VOL.restore_volume(pred, nimg_shape, flip=(False, False), transpose=True, lut=lut, dtype=torch.int16)
