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


# ------------------------------------------------------------------------------------------------ the evaluate script's plumbing
# the columns of the reference's table, in the order it prints them, with the class (position in CLASSES) each one reads
TABLE_CLASSES = (("AA", 3), ("LAblood", 1), ("LVblood", 2), ("LVmyo", 0))
TABLE_METRICS = ("DC", "HD", "ASD")


def _read_volume(img, mask):
    """-> (x, gt, counter): ``read_volume`` without its check; counter: the device-side count of mask values that are no class"""
    from . import kernels as K
    from .utils import volume as VOL
    x = VOL.volume_slices(img, slice_axis=2, flip=(True, True), window=3)
    t = VOL.as_device_volume(mask, "read_volume")
    gt, _, counter = K.volume_labels(t.movedim(2, 0), True, True, 5)
    return x, gt, counter


def read_volume(img, mask, check=True):
    """``read_img`` (``evaluate_mmwhs.py:11-29``) without its file reads: ``img``, ``mask``: the NIfTI arrays ``[H,W,D]`` (numpy, uploaded
    in their own memory order, or device tensors of any stride) -> ``(x [D,3,H,W] fp32, gt [D,H,W] uint8)`` on the device:
    ``np.moveaxis(.., 2, 0)[:, ::-1, ::-1]``, the 2.5-D stack ``img[[i - 1, i, (i + 1) % D]]``, and the mask as
    ``np.argmax(to_categorical(mask, 5), axis=1)`` reads it back.  ``check`` (one synchronisation): a mask value outside 0..4
    raises ``ValueError`` where ``to_categorical`` asserts; ``check=False`` writes such values as background and never synchronises."""
    x, gt, counter = _read_volume(img, mask)
    if check:
        stray = int(counter.item())
        if stray:
            raise ValueError("read_volume: %d values of the mask are no integer in 0..4 (the reference's to_categorical asserts)" % stray)
    return x, gt


def save_row(res, model_name, pat_id, extended=False):
    """the row the reference appends with ``-save`` (``evaluate_mmwhs.py:134-138``): the means of DC, HD and ASD over the four
    classes (the -1 entries included, as there), the model's name and the patient"""
    import numpy as np
    step = 5 if extended else 3
    return [float(np.mean([res[k * step + n] for k in range(4)])) for n in range(3)] + [model_name, pat_id]


def summary_table(results, ifhd=True, ifasd=True, extended=False):
    """The table of ``evaluate_mmwhs.py:141-195`` from the per-patient result lists (12 values each, 20 with ``extended``), on the
    host with numpy as there: ``table[metric][name] = (np.around(np.mean(v), 3), np.around(np.std(v), 3))`` for metric in DC /
    HD / ASD and name in AA / LAblood / LVblood / LVmyo, the -1 entries of HD and ASD left out of that class's list only (a
    class that is -1 for every patient gives nan, as ``np.mean([])`` does), and ``table["Ave"][metric]`` = the reference's
    averages over the four classes of the rounded means and stds."""
    import warnings

    import numpy as np
    step = 5 if extended else 3
    table = {"Ave": {}}
    for n, metric in enumerate(TABLE_METRICS):
        if (metric == "HD" and not ifhd) or (metric == "ASD" and not ifasd):
            continue
        table[metric] = {}
        for name, k in TABLE_CLASSES:
            vals = [res[k * step + n] for res in results]
            if n > 0:
                vals = [v for v in vals if v != -1]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)       # np.mean([]): nan, as the reference prints it
                table[metric][name] = (np.around(np.mean(np.array(vals)), 3), np.around(np.std(np.array(vals)), 3))
        cols = [table[metric][name] for name, _ in TABLE_CLASSES]
        table["Ave"][metric] = (sum(c[0] for c in cols) / 4., sum(c[1] for c in cols) / 4.)
    return table


def print_table(table):
    """the reference's closing lines (``evaluate_mmwhs.py:172-201``)"""
    long_names = {"DC": "Dice"}
    for metric in TABLE_METRICS:
        if metric in table:
            print(", ".join("Ave {} {}: {}, {}".format(name, metric, *table[metric][name]) for name, _ in TABLE_CLASSES))
            print("Ave {}: {:.3f}, {:.3f}".format(long_names.get(metric, metric), *table["Ave"][metric]))
    for metric in TABLE_METRICS:
        if metric in table:
            print(", ".join("{}, {}".format(*table[metric][name]) for name, _ in TABLE_CLASSES))


def evaluate_segmentation(unet_model, volumes, bs=8, ifhd=True, ifasd=True, klc=True, model_name="", extended=False, toprint=True):
    """The loop over patients of ``evaluate_segmentation`` (``evaluate_mmwhs.py:113-201``) without its file reads: ``volumes`` is an
    iterable of ``(pat_id, img, mask)`` with the NIfTI arrays ``[H,W,D]``.  Every volume goes through ``read_volume`` and the stages
    of ``validate.evaluate_volume`` (forward in batches of ``bs``, argmax, largest components with ``klc``, the class metrics) with no
    synchronisation in between; the metric rows of all patients stay on the device and are read at once: ONE synchronisation
    for the whole set.  A mask value outside 0..4 raises ``ValueError`` there (the reference asserts in ``read_img``).
    -> ``{"per_patient": {pat_id: res}, "rows": [...], "table": {...}}``: ``res`` is the reference's list of 12 values per patient
    ([dice, hd, asd] per class; 20 with ``extended``: + hd95, assd), ``rows`` its ``-save`` rows (``save_row``), ``table`` is
    ``summary_table``.  ``toprint``: the reference's lines."""
    import torch

    from . import validate as V
    ids, rows, counters = [], [], []
    for pat_id, img, mask in volumes:
        x, gt, counter = _read_volume(img, mask)
        rows.append(V.evaluate_volume_rows(unet_model, x, gt, bs=bs, klc=klc, variant="mmwhs", extended=extended).flatten())
        counters.append(counter.double())
        ids.append(pat_id)
    per_patient, save_rows = {}, []
    if ids:
        width = rows[0].numel() // len(CLASSES)
        host = torch.cat(rows + counters).tolist()                     # the one synchronisation
        stray = host[len(ids) * len(CLASSES) * width:]
        for pat_id, n in zip(ids, stray):
            if n:
                raise ValueError("evaluate_segmentation: patient %s: %d values of the mask are no integer in 0..4 (the reference's "
                                 "to_categorical asserts)" % (pat_id, int(n)))
        for p, pat_id in enumerate(ids):
            mine = [host[(p * len(CLASSES) + k) * width:(p * len(CLASSES) + k + 1) * width] for k in range(len(CLASSES))]
            res = metrics_from_rows_ext(mine, ifhd, ifasd) if extended else metrics_from_rows(mine, ifhd, ifasd)
            if toprint:
                print("patient {}".format(pat_id))
                if not extended:
                    print(FORMAT.format(*["{:.3f}".format(r) for r in res]))
            per_patient[pat_id] = res
            save_rows.append(save_row(res, model_name, pat_id, extended))
    table = summary_table(list(per_patient.values()), ifhd, ifasd, extended)
    if toprint:
        print_table(table)
    return {"per_patient": per_patient, "rows": save_rows, "table": table}
