"""The metric functions of ``src/evaluate_mscmrseg.py`` on the device: ``compute_metrics_on_files`` (``metric.py:116-175``,
called at ``evaluate_mscmrseg.py:169``) on MS-CMRSeg label volumes (codes 500 = endo / LV, 600 = RV, 200 = myo), and the loop
over patients of ``evaluate_segmentation`` (``:122-229``) from ``read_img``'s result onward: ``read_volume``, the forward,
``reconstuct_volume`` / ``resize_volume`` / ``argmax`` at the label file's own size (one fused kernel, ``csrc/area_resize.hip``;
the resize rule is the build's own, written after OpenCV's ``resize.cpp``, parity with OpenCV not pinned: DESIGN.md f15), the
largest components, the codes, the metrics and the printed table.  File I/O (NIfTI, PNG, CSV), ``clahe=True`` and ``toplot`` are
not part of this package: the caller brings the arrays."""
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
_codes_lut = {}      # (device, dtype) -> the [256] table 1 / 2 / 3 -> 200 / 500 / 600 (uploaded once: an upload makes the host wait)


def codes_table(device, dtype=torch.int32):
    """the ``[256]`` device table 1 / 2 / 3 -> 200 / 500 / 600 (``evaluate_mscmrseg.py:151-153``), uploaded once per device and dtype"""
    key = (device, dtype)
    if key not in _codes_lut:
        _codes_lut[key] = torch.tensor(_CODES, dtype=dtype).to(device)
    return _codes_lut[key]


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
    lut = codes_table(pred.device, torch.int16) if torch.is_tensor(pred) and pred.is_cuda else _CODES
    return VOL.restore_volume(pred, nimg_shape, flip=(False, False), transpose=True, lut=lut, dtype=torch.int16)


# ------------------------------------------------------------------------------------------------ the evaluate script's plumbing
# the columns of the reference's table in the order it prints them, with the class (position in CLASSES) each one reads, the
# order of its three closing lines, and the 'cat' of the -save rows in the order of CLASSES
TABLE_CLASSES = (("endo", 0), ("rv", 1), ("myo", 2))
TABLE_METRICS = ("DC", "HD", "ASD")
CLOSING_ORDER = ("myo", "endo", "rv")
SAVE_CATS = ("lv", "rv", "myo")
SAVE_COLUMNS = ["DSC", "HD", "ASD", "cat", "model", "pad_id"]


def reconstuct_volume(vol, crop_size=112, origin_size=256):
    """``evaluate_mscmrseg.py:30-44`` (sic) for callers that want the intermediate: channels-last fp32 ``vol [N,2 crop,2 crop,C]``
    on the device pasted at ``int(origin_size / 2) +- crop_size`` of a zero ``[N,origin_size,origin_size,C]`` canvas (the
    reference fixes C = 4; here it is ``vol``'s).  ``evaluate_segmentation`` never builds this tensor (``K.reconstruct_resize_argmax``)."""
    if not torch.is_tensor(vol) or vol.dtype != torch.float32 or vol.dim() != 4:
        raise TypeError("reconstuct_volume: a float32 [N,H,W,C] device tensor")
    if not vol.is_cuda:
        raise RuntimeError("reconstuct_volume: HIP device tensors only (no CPU fallback)")
    o = int(origin_size / 2)
    if crop_size < 1 or o - crop_size < 0 or o + crop_size > origin_size or tuple(vol.shape[1:3]) != (2 * crop_size, 2 * crop_size):
        raise ValueError("reconstuct_volume: slices of %dx%d do not fill the window %d +- %d of a canvas of %d"
                         % (vol.shape[1], vol.shape[2], o, crop_size, origin_size))
    recon = torch.zeros((vol.shape[0], origin_size, origin_size, vol.shape[3]), dtype=torch.float32, device=vol.device)
    recon[:, o - crop_size:o + crop_size, o - crop_size:o + crop_size, :] = vol
    return recon


def read_volume(images, crop_size=224):
    """``evaluate_mscmrseg.py:128-130`` from ``read_img``'s result onward: the uint8 stack ``[Z,256,256,3]`` of a patient's PNG
    slices (device tensor or numpy) -> fp32 ``[Z,3,crop_size,crop_size]`` on the device: ``crop_volume(.., crop_size // 2)``,
    ``np.array(.., np.float32) / 255.`` (a float32 division) and ``np.moveaxis(.., -1, 1)``."""
    from .utils import preprocess as PRE
    if not torch.is_tensor(images):
        import numpy as np
        if not isinstance(images, np.ndarray) or images.dtype != np.uint8:
            raise TypeError("read_volume: a uint8 [Z,H,W,C] device tensor or numpy array")
        if not torch.cuda.is_available():
            raise RuntimeError("read_volume: pointcloududa_amd kernels run on a HIP device; none is available (no CPU fallback)")
        images = torch.from_numpy(np.ascontiguousarray(images)).cuda()
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise TypeError("read_volume: a uint8 [Z,H,W,C] device tensor or numpy array")
    if not images.is_cuda:
        raise RuntimeError("read_volume: HIP device tensors only (no CPU fallback)")
    z, h, w, c = images.shape
    planes = images.permute(0, 3, 1, 2).reshape(z * c, h, w)
    crop = PRE.crop_volume(planes, crop_size=int(crop_size) // 2)
    # a 0-dim device divisor: a Python scalar would be turned into a multiplication by its reciprocal
    x = crop.to(torch.float32) / torch.full((), 255.0, dtype=torch.float32, device=crop.device)
    return x.view(z, c, crop.shape[1], crop.shape[2])


def save_rows(res, model_name, pat_id, extended=False):
    """the three rows the reference appends with ``-save`` (``evaluate_mscmrseg.py:171-174``), columns ``SAVE_COLUMNS``: ``res[0:3]``
    as 'lv', ``res[3:6]`` as 'rv', ``res[6:9]`` as 'myo' (with ``extended`` the first three of each class's five)"""
    step = 5 if extended else 3
    return [[res[k * step], res[k * step + 1], res[k * step + 2], cat, model_name, pat_id] for k, cat in enumerate(SAVE_CATS)]


def summary_table(results, ifhd=True, ifasd=True, extended=False):
    """The table of ``evaluate_mscmrseg.py:176-223`` from the per-patient result lists (9 values each, 15 with ``extended``), on the
    host with numpy as there: ``table[metric][name] = (np.around(np.mean(v), 3), np.around(np.std(v), 3))`` for metric in DC / HD
    / ASD and name in endo / rv / myo.  Every Dice value is kept, a -1 included (``:178-180``); the -1 entries of HD and ASD are
    left out of that class's list (``:181-192``; a class that is -1 for every patient gives nan, as ``np.mean([])`` does).
    ``table["Ave"][metric]`` = the sums of the three rounded means and of the three rounded stds over 3."""
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
        table["Ave"][metric] = ((cols[0][0] + cols[1][0] + cols[2][0]) / 3., (cols[0][1] + cols[1][1] + cols[2][1]) / 3.)
    return table


def print_table(table):
    """the reference's closing lines (``evaluate_mscmrseg.py:204-229``), the last three in its order myo, endo, rv"""
    long_names = {"DC": "Dice"}
    for metric in TABLE_METRICS:
        if metric in table:
            print(", ".join("Ave {} {}: {}, {}".format(name, metric, *table[metric][name]) for name, _ in TABLE_CLASSES))
            print("Ave {}: {:.3f}, {:.3f}".format(long_names.get(metric, metric), *table["Ave"][metric]))
    for metric in TABLE_METRICS:
        if metric in table:
            print(", ".join("{}, {}".format(*table[metric][name]) for name in CLOSING_ORDER))


def evaluate_segmentation(unet_model, volumes, bs=8, klc=True, ifhd=True, ifasd=True, crop_size=224, model_name="", extended=False,
                          toprint=True):
    """The loop over patients of ``evaluate_segmentation`` (``evaluate_mscmrseg.py:122-229``) without its file reads: ``volumes``
    is an iterable of ``(pat_id, images, nimg)``: ``read_img``'s uint8 stack ``[Z,256,256,3]`` and the NIfTI label array
    ``[X,Y,Z]`` with the codes 200 / 500 / 600.  Every patient goes through ``read_volume``, the forward in batches of ``bs``,
    the fused ``reconstuct_volume(.., crop_size // 2)`` (into a canvas of the stack's side, the reference's 256) /
    ``resize_volume(.., w=X, h=Y)`` / ``argmax`` to ``[Z,Y,X]``, the
    largest components with ``klc``, the codes and the class metrics against ``nimg.T`` (``read_labels``) with no
    synchronisation in between; the metric rows of all patients stay on the device and are read at once: ONE synchronisation
    for the whole set.
    -> ``{"per_patient": {pat_id: res}, "rows": [...], "table": {...}}``: ``res`` is the reference's list of 9 values per patient
    ([dice, hd, asd] for endo, rv, myo; 15 with ``extended``: + hd95, assd), ``rows`` its ``-save`` rows (``save_rows``, three per
    patient, columns ``SAVE_COLUMNS``), ``table`` is ``summary_table``.  ``toprint``: the reference's lines."""
    from . import validate as V
    ids, rows = [], []
    for pat_id, images, nimg in volumes:
        x = read_volume(images, crop_size)
        gt = read_labels(nimg)
        rows.append(V.evaluate_volume_rows(unet_model, x, gt, bs=bs, klc=klc, variant="mscmrseg", extended=extended,
                                           native_shape=(int(nimg.shape[0]), int(nimg.shape[1])), crop_size=int(crop_size) // 2,
                                           origin_size=int(images.shape[1])).flatten())
        ids.append(pat_id)
    per_patient, out_rows = {}, []
    if ids:
        width = rows[0].numel() // len(CLASSES)
        host = torch.cat(rows).tolist()                                # the one synchronisation
        for p, pat_id in enumerate(ids):
            mine = [host[(p * len(CLASSES) + k) * width:(p * len(CLASSES) + k + 1) * width] for k in range(len(CLASSES))]
            res = metrics_from_rows_ext(mine, ifhd, ifasd) if extended else metrics_from_rows(mine, ifhd, ifasd)
            if toprint:
                print("patient {}".format(pat_id))
                if not extended:
                    print(FORMAT.format(*["{:.3f}".format(r) for r in res]))
            per_patient[pat_id] = res
            out_rows += save_rows(res, model_name, pat_id, extended)
    table = summary_table(list(per_patient.values()), ifhd, ifasd, extended)
    if toprint:
        print_table(table)
    return {"per_patient": per_patient, "rows": out_rows, "table": table}
