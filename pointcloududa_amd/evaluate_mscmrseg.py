"""The metric functions of ``src/evaluate_mscmrseg.py`` on the device: ``compute_metrics_on_files`` (``metric.py:116-175``,
called at ``evaluate_mscmrseg.py:169``) on MS-CMRSeg label volumes (codes 500 = endo / LV, 600 = RV, 200 = myo).  The
file I/O of ``evaluate_segmentation`` (NIfTI, cv2 resize, pandas) is not part of this package; ``validate.evaluate_volume``
is its device-side core."""
from __future__ import annotations

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
