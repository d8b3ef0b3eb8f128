"""Writes tests/golden/eval_metrics.npz: the evaluation metrics (medpy.metric.binary dc / hd / asd, utils.py's
keep_largest_connected_components, the evaluate scripts' result lists) restated with scipy.ndimage on small cases.

    python scripts/make_eval_golden.py            # (re)writes the fixture; tests/test_eval_metrics.py checks it regenerates

Definitions (A = pred == c, B = gt == c):
  dc        = 2|A.B| / (|A| + |B|), 0 when both are empty
  border(X) = X & ~binary_erosion(X, generate_binary_structure(ndim, connectivity), border_value=0)
  sd(X, Y)  = distance_transform_edt(~border(Y), sampling=spacing)[border(X)]
  hd        = max(max sd(A, B), max sd(B, A));  asd(X, Y) = mean sd(X, Y)
The numpy-only half of this file (blobs, the brute-force restatement) is imported by the GPU tests, which must not need
scipy; the scipy half is imported lazily."""
from __future__ import annotations

import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "eval_metrics.npz")
COLS = 8   # dice, hd, asd(pred->gt), asd(gt->pred), |A|, |B|, |A.B|, flags (1: A empty, 2: B empty)


# ------------------------------------------------------------------------------------------------ numpy only
def blobs(shape, seed, labels, n=12, shift=0):
    """a label volume of random ellipsoids (later ones paint over earlier ones); ``shift`` moves every centre by up to
    that many voxels per axis (a second, seeded draw), so that blobs(.., shift=2) is a plausible prediction of blobs(..)"""
    rng = np.random.default_rng(seed)
    jit = np.random.default_rng(seed + 1000)
    vol = np.zeros(shape, dtype=np.int32)
    grids = np.ogrid[tuple(slice(0, s) for s in shape)]
    for i in range(n):
        c = [rng.uniform(0, s) for s in shape]
        r = [rng.uniform(1.5, max(2.0, s / 4)) for s in shape]
        if shift:
            c = [ci + jit.integers(-shift, shift + 1) for ci in c]
        d = sum(((g - ci) / ri) ** 2 for g, ci, ri in zip(grids, c, r))
        vol[d <= 1.0] = labels[i % len(labels)]
    return vol


def footprint_offsets(ndim, connectivity):
    """the neighbours of generate_binary_structure(ndim, connectivity), centre excluded"""
    offs = np.stack(np.meshgrid(*[[-1, 0, 1]] * ndim, indexing="ij"), -1).reshape(-1, ndim)
    k = np.abs(offs).sum(1)
    return offs[(k > 0) & (k <= connectivity)]


def border_np(x, connectivity=1):
    x = np.asarray(x, dtype=bool)
    pad = np.pad(x, 1, constant_values=False)
    er = x.copy()
    for o in footprint_offsets(x.ndim, connectivity):
        sl = tuple(slice(1 + d, 1 + d + s) for d, s in zip(o, x.shape))
        er &= pad[sl]
    return x & ~er


def surface_brute(pred, gt, classes, spacing=None, connectivity=1):
    """the definitions above by all-pairs distances (small volumes only)"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    sp = np.ones(pred.ndim) if spacing is None else np.asarray(spacing, dtype=np.float64)
    out = np.zeros((len(classes), COLS))
    for k, c in enumerate(classes):
        a, b = pred == c, gt == c
        na, nb, nab = int(a.sum()), int(b.sum()), int((a & b).sum())
        flags = (1 if na == 0 else 0) | (2 if nb == 0 else 0)
        out[k, [0, 4, 5, 6, 7]] = [2.0 * nab / (na + nb) if na + nb else 0.0, na, nb, nab, flags]
        if flags:
            out[k, 1:4] = np.nan
            continue
        pa = np.argwhere(border_np(a, connectivity)) * sp
        pb = np.argwhere(border_np(b, connectivity)) * sp
        dist = np.sqrt(((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1))
        ab, ba = dist.min(1), dist.min(0)
        out[k, 1:4] = [max(ab.max(), ba.max()), ab.mean(), ba.mean()]
    return out


def largest_components_brute(mask):
    """utils.py:43-65 by flood fill (face connectivity), ties to the raster-first component"""
    mask = np.asarray(mask)
    out = np.zeros(mask.shape, dtype=np.uint8)
    offs = footprint_offsets(mask.ndim, 1)
    for sid in range(1, mask.shape[1] + 1):
        m = mask == sid
        seen = np.zeros(mask.shape, dtype=bool)
        best = None
        for start in map(tuple, np.argwhere(m)):                # raster order
            if seen[start]:
                continue
            comp, stack = [], [start]
            seen[start] = True
            while stack:
                p = stack.pop()
                comp.append(p)
                for o in offs:
                    q = tuple(int(pi + oi) for pi, oi in zip(p, o))
                    if all(0 <= qi < s for qi, s in zip(q, mask.shape)) and m[q] and not seen[q]:
                        seen[q] = True
                        stack.append(q)
            if best is None or len(comp) > len(best):
                best = comp
        if best is not None:
            out[tuple(np.array(best).T)] = sid
    return out


# ------------------------------------------------------------------------------------------------ scipy
def border(x, connectivity=1):
    from scipy.ndimage import binary_erosion, generate_binary_structure
    x = np.asarray(x, dtype=bool)
    return x & ~binary_erosion(x, structure=generate_binary_structure(x.ndim, connectivity), iterations=1, border_value=0)


def sd(x, y, spacing=None, connectivity=1):
    from scipy.ndimage import distance_transform_edt
    return distance_transform_edt(~border(y, connectivity), sampling=spacing)[border(x, connectivity)]


def surface(pred, gt, classes, spacing=None, connectivity=1):
    pred, gt = np.asarray(pred), np.asarray(gt)
    out = np.zeros((len(classes), COLS))
    for k, c in enumerate(classes):
        a, b = pred == c, gt == c
        na, nb, nab = int(a.sum()), int(b.sum()), int((a & b).sum())
        flags = (1 if na == 0 else 0) | (2 if nb == 0 else 0)
        out[k, [0, 4, 5, 6, 7]] = [2.0 * nab / (na + nb) if na + nb else 0.0, na, nb, nab, flags]
        if flags:
            out[k, 1:4] = np.nan
            continue
        ab, ba = sd(a, b, spacing, connectivity), sd(b, a, spacing, connectivity)
        out[k, 1:4] = [max(ab.max(), ba.max()), ab.mean(), ba.mean()]
    return out


def largest_components(mask):
    """utils.py:43-65 with scipy.ndimage.label; the tie goes to the component with the smallest first linear index"""
    from scipy.ndimage import generate_binary_structure, label
    mask = np.asarray(mask)
    out = np.zeros(mask.shape, dtype=np.uint8)
    for sid in range(1, mask.shape[1] + 1):
        lab, n = label(mask == sid, structure=generate_binary_structure(mask.ndim, 1))
        if n == 0:
            continue
        flat = lab.ravel()
        sizes = np.bincount(flat, minlength=n + 1)[1:]
        first = np.full(n, flat.size)
        idx = np.flatnonzero(flat)
        np.minimum.at(first, flat[idx] - 1, idx)
        cand = np.flatnonzero(sizes == sizes.max())
        win = cand[np.argmin(first[cand])] + 1
        out[lab == win] = sid
    return out


def mscmrseg_list(rows, ifhd, ifasd):
    res = []
    for r in rows:
        dice, h, a = r[0], -1, -1
        if ifhd or ifasd:
            if r[7]:
                dice, h, a = -1, -1, -1
            else:
                h = r[1] if ifhd else h
                a = r[2] if ifasd else a       # rows of surface(gt, pred): medpy asd(gt, pred), over gt's border
        res += [dice, h, a]
    return res


def mmwhs_list(rows, ifhd, ifasd):
    res = []
    for r in rows:
        res += [r[0], r[1] if ifhd and not r[7] else -1, r[2] if ifasd and not r[7] else -1]
    return res


# ------------------------------------------------------------------------------------------------ cases
def surface_cases():
    """(name, pred, gt, classes, spacing, connectivity); pred None = regenerate from the seed (big cases)"""
    cs = []
    a = np.zeros((12, 16, 16), np.uint8); a[2:8, 3:9, 4:10] = 1
    b = np.zeros_like(a); b[4:10, 5:11, 4:10] = 1                       # offset cubes: hd = |(2, 2, 0)| = sqrt 8
    cs.append(("offset_cubes", a, b, [1], None, 1))
    full = np.ones((5, 6, 7), np.uint8); part = full.copy(); part[0] = 0  # every face touches the volume's edge
    cs.append(("touch_faces", full, part, [1], None, 1))
    s1 = np.zeros((7, 9, 8), np.uint8); s1[3, 4, 2] = 1
    s2 = np.zeros_like(s1); s2[1, 0, 7] = 1                              # single voxels: their own border
    cs.append(("single_voxels", s1, s2, [1], None, 1))
    sh = np.zeros((14, 14, 14), np.uint8); sh[2:12, 2:12, 2:12] = 1; sh[4:10, 4:10, 4:10] = 0   # hollow shell
    so = np.zeros_like(sh); so[3:11, 3:11, 3:11] = 1
    cs.append(("hollow_shell", sh, so, [1], None, 1))
    wall = np.zeros((9, 12, 12), np.uint8); wall[:, 6, :] = 1            # one-voxel wall: erosion empties it
    w2 = np.zeros_like(wall); w2[4, :, 3] = 1
    cs.append(("thin_walls", wall, w2, [1], None, 1))
    p2, g2 = blobs((40, 48), 11, [1, 2, 3], n=8), blobs((40, 48), 11, [1, 2, 3], n=8, shift=3)
    cs.append(("blobs_2d", p2, g2, [1, 2, 3], None, 1))
    cs.append(("blobs_2d_conn2", p2, g2, [1, 2, 3], None, 2))
    cs.append(("blobs_2d_spacing", p2, g2, [1, 2, 3], (1.25, 0.8), 1))
    p3, g3 = blobs((12, 64, 64), 21, [1, 2, 3, 4]), blobs((12, 64, 64), 21, [1, 2, 3, 4], shift=2)
    for conn in (1, 2, 3):
        cs.append(("blobs_12x64x64_conn%d" % conn, p3, g3, [1, 2, 3, 4], None, conn))
    cs.append(("blobs_12x64x64_aniso", p3, g3, [1, 2, 3, 4], (10.0, 1.25, 1.25), 1))
    cs.append(("blobs_12x64x64_aniso_conn3", p3, g3, [4, 3, 2, 1], (2.5, 1.0, 0.7), 3))
    cs.append(("blobs_12x64x64_empty", p3, g3, [1, 5, 0, 2], None, 1))  # class 5 empty on both sides
    pe = p3.copy(); pe[pe == 2] = 0
    cs.append(("pred_class_empty", pe, g3, [1, 2, 3], None, 1))
    cs.append(("gt_class_empty", g3, pe, [1, 2, 3], None, 1))
    cm = blobs((10, 48, 48), 31, [200, 500, 600])
    cm2 = blobs((10, 48, 48), 31, [200, 500, 600], shift=2)
    cs.append(("mscmrseg_codes", cm.astype(np.int16), cm2.astype(np.int16), [500, 600, 200], None, 1))
    cs.append(("mmwhs_1to4_8cls", p3, g3, [1, 2, 3, 4, 5, 6, 7, 0], None, 1))
    cs.append(("big_20x256x256", None, None, [1, 2, 3], None, 1))      # regenerated: big_volume()
    return cs


def big_volume():
    return blobs((20, 256, 256), 41, [1, 2, 3], n=24), blobs((20, 256, 256), 41, [1, 2, 3], n=24, shift=3)


def ccl_cases():
    cs = []
    t = np.zeros((6, 8), np.uint8)                                        # 2-D: two equal components of label 1
    t[1, 1:3] = 1; t[4, 5:7] = 1; t[0, 7] = 2; t[5, 0] = 2; t[3, 3] = 3
    cs.append(("tie_2d", t))
    t3 = np.zeros((4, 6, 6), np.uint8)                                    # 3-D ties, diagonal-only contacts
    t3[0, 0, 0] = t3[1, 1, 1] = 1; t3[3, 5, 5] = t3[2, 4, 4] = 1; t3[0, 2:4, 2] = 4; t3[3, 2, 2:4] = 4
    cs.append(("tie_3d_diagonal", t3))
    cs.append(("blobs_3d", blobs((12, 64, 64), 51, [1, 2, 3, 4], n=30).astype(np.uint8)))
    big = blobs((6, 5, 40), 52, [1, 2, 3, 4, 5, 6, 7, 9], n=20).astype(np.uint8)    # labels above shape[1] = 5 stay 0
    cs.append(("labels_above_shape1", big))
    sp = (np.random.default_rng(53).random((10, 12, 14)) < 0.45).astype(np.int32) * \
        np.random.default_rng(54).integers(1, 4, (10, 12, 14)).astype(np.int32)     # speckle: many small components
    cs.append(("speckle_int32", sp))
    cs.append(("empty", np.zeros((3, 4, 5), np.uint8)))
    return cs


def file_cases():
    """(variant, gt, pred, ifhd, ifasd) for the evaluate scripts' compute_metrics_on_files"""
    cm = blobs((10, 48, 48), 61, [200, 500, 600]).astype(np.int16)
    cp = blobs((10, 48, 48), 61, [200, 500, 600], shift=2).astype(np.int16)
    cpe = cp.copy(); cpe[cpe == 600] = 0
    wg = blobs((12, 64, 64), 62, [1, 2, 3, 4]).astype(np.uint8)
    wp = blobs((12, 64, 64), 62, [1, 2, 3, 4], shift=2).astype(np.uint8)
    wpe = wp.copy(); wpe[wpe == 3] = 0
    return [("mscmrseg", cm, cp, True, True), ("mscmrseg", cm, cpe, True, True), ("mscmrseg", cm, cpe, False, False),
            ("mscmrseg", cm, cp, True, False), ("mmwhs", wg, wp, True, True), ("mmwhs", wg, wpe, True, True),
            ("mmwhs", wg, wpe, False, True)]


CLASSES = {"mscmrseg": [500, 600, 200], "mmwhs": [1, 2, 3, 4]}


def build():
    g = {}
    for i, (name, p, t, cls, sp, conn) in enumerate(surface_cases()):
        if p is None:
            p, t = big_volume()
            g["s%d_regen" % i] = np.int8(1)
        else:
            g["s%d_pred" % i], g["s%d_gt" % i] = p, t
        g["s%d_name" % i] = np.array(name)
        g["s%d_classes" % i] = np.array(cls, np.int32)
        g["s%d_spacing" % i] = np.array(sp if sp is not None else [], np.float64)
        g["s%d_conn" % i] = np.int32(conn)
        g["s%d_out" % i] = surface(p, t, cls, sp, conn)
    for i, (name, m) in enumerate(ccl_cases()):
        g["c%d_name" % i], g["c%d_mask" % i], g["c%d_out" % i] = np.array(name), m, largest_components(m)
    for i, (var, gt, pr, ifhd, ifasd) in enumerate(file_cases()):
        rows = surface(gt, pr, CLASSES[var])          # (gt, pred): the scripts call dc / hd / asd(gt_c, pred_c)
        res = (mscmrseg_list if var == "mscmrseg" else mmwhs_list)(rows, ifhd, ifasd)
        g["f%d_variant" % i], g["f%d_gt" % i], g["f%d_pred" % i] = np.array(var), gt, pr
        g["f%d_flags" % i] = np.array([ifhd, ifasd])
        g["f%d_res" % i] = np.array(res, np.float64)
    return g


if __name__ == "__main__":
    g = build()
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays")
