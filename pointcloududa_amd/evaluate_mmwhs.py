"""The metric functions of ``src/evaluate_mmwhs.py`` on the device: ``metrics`` / ``compute_metrics_on_files``
(``evaluate_mmwhs.py:32-80``) on MM-WHS label volumes (1 = Myo, 2 = LA-blood, 3 = LV-blood, 4 = AA).  The file I/O of
``evaluate_segmentation`` is not part of this package; ``validate.evaluate_volume`` is its device-side core
(``evaluate_mmwhs.py:118-132``)."""
from __future__ import annotations

from .utils import metric as M

CLASSES = [1, 2, 3, 4]
FORMAT = ("Myo {:>8} , {:>8} , {:>8} , LA-blood {:>8} , {:>8} , {:>8} , LV-blood {:>8} , {:>8} , {:>8} , "
          "AA {:>8} , {:>8} , {:>8}")


def metrics_from_rows(rows, ifhd=True, ifasd=True):
    """[dice, hd, asd] per class from ``M.class_metrics(gt, pred, CLASSES)`` rows: hd / asd are -1 when not asked for
    and when medpy would raise (a class empty on either side: the reference's ``try / except``)"""
    res = []
    for row in rows:
        h_d = row[1] if ifhd and not row[7] else -1
        a_sd = row[2] if ifasd and not row[7] else -1
        res += [row[0], h_d, a_sd]
    return res


def metrics_from_rows_ext(rows, ifhd=True, ifasd=True):
    """[dice, hd, asd, hd95, assd] per class from ``M.class_metrics_ext(gt, pred, CLASSES)`` rows, with the conventions of
    ``metrics_from_rows``: hd and hd95 go with ``ifhd``, asd and assd with ``ifasd``; -1 where not asked for and where
    medpy would raise (a class empty on either side)"""
    res = []
    for row in rows:
        ok_hd, ok_asd = ifhd and not row[7], ifasd and not row[7]
        res += [row[0], row[1] if ok_hd else -1, row[2] if ok_asd else -1, row[8] if ok_hd else -1,
                row[9] if ok_asd else -1]
    return res


def metrics(img_gt, img_pred, ifhd=True, ifasd=True):
    """``evaluate_mmwhs.py:32-62``"""
    return metrics_from_rows(M.class_metrics(img_gt, img_pred, CLASSES).tolist(), ifhd, ifasd)


def compute_metrics_on_files(gt, pred, ifhd=True, ifasd=True):
    """``evaluate_mmwhs.py:65-80``: ``metrics`` and the reference's printed line"""
    res = metrics(gt, pred, ifhd=ifhd, ifasd=ifasd)
    print(FORMAT.format(*["{:.3f}".format(r) for r in res]))
    return res
