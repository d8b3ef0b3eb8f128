"""Generator of tests/golden/spx_connect.npz and tests/golden/spx_connect_digests.json: the expected values of the connected
superpixels (pointcloududa_amd/utils/stylize.py ``min_size``, csrc/spx_connect.hip).

The rule (integers only, this build's own; skimage is not installed, parity with its ``_enforce_label_connectivity_cython`` is
unpinned).  Input: the label plane ``lab[H,W]`` of the grid SLIC's last assignment (``slic_numpy`` / ``slic_python`` of
make_stylize_golden.py), the slot's input image and ``min_size >= 1``:

1. 4-connected components of equal labels (label 0 is an ordinary label); a component's id is its raster-first pixel's index
   ``r = y W + x``, its size its own pixel count
2. a component is small iff ``size < min_size`` and ``r != 0``; its target is the component of pixel ``r - 1`` if ``x > 0``, else of
   pixel ``r - W``; targets are followed until a component that is not small (merged pixels count towards nobody's size)
3. a final segment -- the pixels of one final id -- takes ``rdiv(sum_ch, n)`` over its pixels iff the first Philox word for
   counter = final id is below ``floor(p_replace 2^32)``, else its pixels are copied

restated twice, independently:

* ``connect_numpy``: ``scipy.ndimage.label`` per label value, the minimum index per component, the targets of the small
  roots and pointer jumping until nothing moves
* ``connect_python``: plain Python integers, sequential: a raster-order flood fill that gives a small component the ALREADY FINAL
  id of its left / upper pixel; Philox in Python integers

``run_program`` interprets a whole program: a SUPERPIXELS slot with ``iarg[5] > 0`` goes through the rule above, every other
slot through make_stylize_golden.py's interpreter.  ``main`` refuses to write unless the two restatements agree bit for bit on
every case, every final segment of every case is 4-connected (``scipy.sparse.csgraph.connected_components`` on the grid graph:
a third route) and no final id other than 0 belongs to a component below ``min_size``.

    python scripts/make_spx_connect_golden.py        # writes the two files"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import make_stylize_golden as F9  # noqa: E402
from make_stylize_golden import SUPERPIXELS, Prog, dilate, philox4x32_10, planar, rdiv, threshold  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spx_connect.npz")
OUT_DIGESTS = os.path.join(ROOT, "tests", "golden", "spx_connect_digests.json")


def superpixel_min_size(gy, gx, h, w):
    """half the mean segment size (skimage's min_size_factor = 0.5), at least 1"""
    return max(1, (h * w) // (2 * gy * gx))


# ------------------------------------------------------------------------------------------------ vectorised
def components_numpy(lab):
    """-> int64 [H,W]: the raster-first index of every pixel's 4-connected component of equal labels"""
    from scipy import ndimage
    h, w = lab.shape
    index = np.arange(h * w, dtype=np.int64).reshape(h, w)
    ids = np.full((h, w), -1, dtype=np.int64)
    for k in np.unique(lab):
        mask = lab == k
        comp, n = ndimage.label(mask)                 # (the default structure is the 4-neighbourhood)
        roots = np.asarray(ndimage.minimum(index, comp, index=np.arange(1, n + 1)), dtype=np.int64)
        ids[mask] = roots[comp[mask] - 1]
    return ids


def final_ids_numpy(lab, min_size, info=None):
    """-> int64 [H,W] final ids; ``info`` (a dict) receives the component count, the pointer-jumping rounds and the longest
    chain of targets"""
    h, w = lab.shape
    ids = components_numpy(lab)
    flat = ids.ravel()
    size = np.bincount(flat, minlength=h * w)
    roots = np.unique(flat)
    small = roots[(size[roots] < min_size) & (roots != 0)]
    parent = np.arange(h * w, dtype=np.int64)
    parent[small] = flat[np.where(small % w > 0, small - 1, small - w)]
    assert np.all(parent[small] < small)
    rounds = 0
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            break
        parent, rounds = nxt, rounds + 1
    if info is not None:
        depth = np.zeros(h * w, dtype=np.int64)
        first = np.arange(h * w, dtype=np.int64)
        first[small] = flat[np.where(small % w > 0, small - 1, small - w)]
        for r in small:                               # (ascending: a target is below its source)
            depth[r] = depth[first[r]] + 1
        info.update(components=int(len(roots)), rounds=rounds, longest_chain=int(depth.max()) if len(small) else 0)
    return parent[ids], ids


def connect_numpy(img, lab, min_size, thr, seed, info=None):
    """-> (int64 [H,W,C], final ids int64 [H,W], component ids int64 [H,W])"""
    h, w, c = img.shape
    v = img.astype(np.int64)
    fin, ids = final_ids_numpy(np.asarray(lab, dtype=np.int64).reshape(h, w), int(min_size), info)
    flat = fin.ravel()
    n = np.bincount(flat, minlength=h * w).astype(np.int64)
    sums = np.zeros((h * w, c), dtype=np.int64)
    np.add.at(sums, flat, v.reshape(-1, c))
    seg = np.unique(flat)
    rep = np.zeros(h * w, dtype=bool)
    if thr:
        rep[seg] = philox4x32_10(seed, seg.astype(np.uint32))[0] < np.uint32(thr)
    mean = np.zeros((h * w, c), dtype=np.int64)
    mean[seg] = rdiv(sums[seg], n[seg, None])
    return np.where(rep[fin][..., None], mean[fin], v), fin, ids


# ------------------------------------------------------------------------------------------------ sequential
def connect_python(img, lab, min_size, thr, seed):
    """plain Python integers; ``lab``: a list of H W labels -> (int64 [H,W,C], final ids int64 [H,W])"""
    h, w, c = img.shape
    px = img.reshape(h * w, c).tolist()
    lab = [int(v) for v in lab]
    final = [-1] * (h * w)
    for r in range(h * w):
        if final[r] >= 0:
            continue
        k = lab[r]
        final[r] = r                       # (marks the pixel as seen; r is the raster-first pixel of its component)
        comp, stack = [r], [r]
        while stack:
            p = stack.pop()
            y, x = divmod(p, w)
            for q, ok in ((p - 1, x > 0), (p + 1, x + 1 < w), (p - w, y > 0), (p + w, y + 1 < h)):
                if ok and final[q] < 0 and lab[q] == k:
                    final[q] = r
                    comp.append(q)
                    stack.append(q)
        if len(comp) < min_size and r != 0:
            fid = final[r - 1] if r % w > 0 else final[r - w]      # already final: that pixel comes before r
            for p in comp:
                final[p] = fid
    n, sums = {}, {}
    for p in range(h * w):
        f = final[p]
        if f not in n:
            n[f], sums[f] = 0, [0] * c
        n[f] += 1
        acc = sums[f]
        for ch in range(c):
            acc[ch] += px[p][ch]
    paint = {f: [(2 * sums[f][ch] + n[f]) // (2 * n[f]) for ch in range(c)]
             for f in n if F9._philox_word0_python(int(seed), f) < thr}
    out = [paint.get(final[p], px[p]) for p in range(h * w)]
    return np.array(out, dtype=np.int64).reshape(h, w, c), np.array(final, dtype=np.int64).reshape(h, w)


# ------------------------------------------------------------------------------------------------ properties
def segments_are_connected(fin):
    """every set of pixels with one final id is 4-connected: the grid graph with an edge between equal neighbours has as many
    connected components as there are ids"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    h, w = fin.shape
    idx = np.arange(h * w).reshape(h, w)
    eh, ev = fin[:, :-1] == fin[:, 1:], fin[:-1] == fin[1:]
    a = np.concatenate([idx[:, :-1][eh], idx[:-1][ev]])
    b = np.concatenate([idx[:, 1:][eh], idx[1:][ev]])
    g = coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(h * w, h * w))
    return connected_components(g, directed=False)[0] == len(np.unique(fin))


def check_properties(fin, ids, min_size, name=""):
    assert segments_are_connected(fin), "a final segment is in pieces: %s" % name
    size = np.bincount(ids.ravel(), minlength=ids.size)
    seg = np.unique(fin)
    assert np.all(ids.ravel()[seg] == seg), "a final id is not a component's own id: %s" % name
    assert np.all(size[seg[seg != 0]] >= min_size), "a segment other than id 0's is below min_size: %s" % name


# ------------------------------------------------------------------------------------------------ interpreter
_SLIC = {}


def _labels(cur, ia, backend):
    key = (backend, cur.shape, cur.tobytes(), tuple(int(v) for v in ia[:4]))
    if key not in _SLIC:
        if len(_SLIC) > 64:
            _SLIC.clear()
        args = (cur, int(ia[0]), int(ia[1]), int(ia[2]), int(ia[3]))
        _SLIC[key] = F9.slic_numpy(*args)[0] if backend == "numpy" else F9.slic_python(*args)[0]
    return _SLIC[key]


def run_program(images, opcode, iarg, farg, table, seed, backend="numpy", info=None, check=False):
    """uint8 [B,H,W,C] + a program -> (uint8 [B,H,W,C], excusable bool [B,H,W,C]) as make_stylize_golden.run_program, with
    ``iarg[5]`` of SUPERPIXELS slots honoured.  ``info`` (a list) receives a dict per connected slot; ``check`` asserts the
    connectedness and min-size properties of every connected slot (numpy backend)."""
    out = np.empty_like(images)
    exc = np.zeros(images.shape, dtype=bool)
    h, w = images.shape[1:3]
    for i in range(images.shape[0]):
        cur, e = images[i], np.zeros(images.shape[1:], dtype=bool)
        for s in range(opcode.shape[1]):
            op, ia = int(opcode[i, s]), iarg[i, s]
            if op == SUPERPIXELS and int(ia[5]) > 0:
                lab, m, thr = _labels(cur, ia, backend), min(int(ia[5]), h * w), threshold(farg[i, s, 0])
                if backend == "numpy":
                    d = dict(sample=i, slot=s)
                    v, fin, ids = connect_numpy(cur, lab, m, thr, int(seed[i, s]), d)
                    if check:
                        check_properties(fin, ids, m, "sample %d slot %d" % (i, s))
                    d.update(segments=int(len(np.unique(fin))))
                    if info is not None:
                        info.append(d)
                else:
                    v, fin = connect_python(cur, np.asarray(lab).reshape(-1).tolist(), m, thr, int(seed[i, s]))
                e = np.full_like(e, bool(e.any()))      # (every pixel depends on every pixel)
                cur = v.astype(np.uint8)
            else:
                one = tuple(np.ascontiguousarray(a[i:i + 1, s:s + 1]) for a in (opcode, iarg, farg, table, seed))
                o, ee = F9.run_program(cur[None], *one, backend=backend)
                radius, mixes = {F9.HUE_SATURATION: (0, True), F9.NOISE_ALPHA: (1, False)}.get(op, (0, False))
                e = (np.full_like(e, bool(e.any())) if op == SUPERPIXELS else dilate(e, radius, mixes)) | ee[0]
                cur = o[0]
        out[i], exc[i] = cur, e
    return out, exc


# ------------------------------------------------------------------------------------------------ cases
SMALL = (      # name, (h, w, c), kind, (gy, gx), updates, compactness
    ("one_pixel", (1, 1, 1), "random", (1, 1), 5, 10),
    ("row", (1, 40, 1), "random", (1, 5), 5, 10),
    ("column", (40, 1, 1), "random", (5, 1), 5, 10),
    ("tiny", (5, 7, 1), "random", (2, 3), 5, 10),
    ("odd", (50, 70, 1), "random", (10, 20), 5, 10),
    ("fragments", (64, 48, 3), "random", (16, 16), 0, 0),
    ("smooth", (48, 64, 3), "smooth", (6, 8), 5, 10),
    ("tiles_c4", (130, 90, 4), "smooth", (9, 6), 5, 10),
)
PRODUCTION = (("production_n20", 20), ("production_n200", 200))
P_BETWEEN = 0.55


def _noisy(kind, h, w, c, seed):
    """the image of a case: f7's kinds; a smooth image gets +-12 grey levels of noise so that colour breaks the segments"""
    x = F9.make_images(kind, 1, h, w, c, seed)[0]
    if kind == "smooth":
        n = np.random.default_rng(seed + 1).integers(-12, 13, x.shape)
        x = np.clip(x.astype(np.int64) + n, 0, 255).astype(np.uint8)
    return x


def small_cases():
    """one image per case, nine samples: min_size in {1, superpixel_min_size, H W} x p_replace in {0, between, 1}"""
    cs = []
    rng = np.random.default_rng(20270)
    for n, (name, (h, w, c), kind, (gy, gx), iters, compactness) in enumerate(SMALL):
        prog = Prog(9, 1)
        for i in range(9):
            m = (1, superpixel_min_size(gy, gx, h, w), h * w)[i // 3]
            prog.put(i, 0, SUPERPIXELS, gy=gy, gx=gx, iters=iters, compactness=compactness, p=(0.0, P_BETWEEN, 1.0)[i % 3],
                     seed=int(rng.integers(0, 2 ** 63)))
            prog.iarg[i, 0, 5] = m
        cs.append(dict(name="%s_%dx%dx%d" % (name, h, w, c), b=9, h=h, w=w, c=c, seed=700 + n, kind=kind, prog=prog))
    return cs


def production_cases():
    """256 x 256 x 3, B = 2 (a smooth image with noise, uniform noise), n_segments 20 and 200 through the package's grid rule
    restated here, 5 updates, compactness 10, min_size = superpixel_min_size"""
    cs = []
    rng = np.random.default_rng(20271)
    for n, (name, segments) in enumerate(PRODUCTION):
        h = w = 256
        gy = min(h, max(1, int(np.floor(np.sqrt(segments * h / w) + 0.5))))
        gx = min(w, max(1, int(np.floor(segments / gy + 0.5))))
        prog = Prog(2, 1)
        for i in range(2):
            prog.put(i, 0, SUPERPIXELS, gy=gy, gx=gx, iters=5, p=(1.0, P_BETWEEN)[i], seed=int(rng.integers(0, 2 ** 63)))
            prog.iarg[i, 0, 5] = superpixel_min_size(gy, gx, h, w)
        cs.append(dict(name=name, b=2, h=h, w=w, c=3, seed=800 + n, kind="mixed", prog=prog))
    return cs


def case_inputs(case):
    b, h, w, c, seed = (int(case[k]) for k in ("b", "h", "w", "c", "seed"))
    if case["kind"] == "mixed":
        return np.stack([_noisy("smooth", h, w, c, seed), _noisy("random", h, w, c, seed + 7)])
    return np.ascontiguousarray(np.repeat(_noisy(case["kind"], h, w, c, seed)[None], b, axis=0))


def _arrays(case):
    p = case["prog"]
    return p.opcode, p.iarg, p.farg, p.table, p.seed


def expected(case, backend="numpy", info=None, check=False):
    out, exc = run_program(case_inputs(case), *_arrays(case), backend=backend, info=info, check=check)
    assert not exc.any()
    return out


def check_restatement(case_list):
    """the sequential restatement against the vectorised one, bit for bit, with the properties asserted -> pixels compared"""
    tot = 0
    for case in case_list:
        a = expected(case, "independent")
        n = expected(case, "numpy", check=True)
        assert np.array_equal(a, n), (case["name"], int((a != n).sum()))
        tot += a.size
    return tot


def build():
    g = {}
    for n, case in enumerate(small_cases()):
        info = []
        out = expected(case, "numpy", info=info, check=True)
        h, w = case["h"], case["w"]
        x = case_inputs(case)
        for i in range(6, 9):      # min_size = H W: everything drains into pixel 0's segment
            assert info[i]["segments"] == 1, case["name"]
        want = rdiv(x[8].astype(np.int64).reshape(h * w, -1).sum(0), h * w)
        assert np.array_equal(out[8].reshape(h * w, -1), np.broadcast_to(want, (h * w, len(want)))), case["name"]
        assert np.array_equal(out[0], x[0]) and np.array_equal(out[3], x[3]) and np.array_equal(out[6], x[6])      # p = 0 copies
        k = "c%02d_" % n
        g[k + "name"] = np.array(case["name"])
        g[k + "kind"] = np.array(case["kind"])
        g[k + "dims"] = np.array([case[s] for s in ("b", "h", "w", "c", "seed")], dtype=np.int64)
        g[k + "opcode"], g[k + "iarg"], g[k + "farg"], g[k + "table"], g[k + "seed"] = _arrays(case)
        g[k + "u8"] = planar(out)
        g[k + "components"] = np.array([d["components"] for d in info], dtype=np.int64)
        g[k + "segments"] = np.array([d["segments"] for d in info], dtype=np.int64)
        g[k + "longest_chain"] = np.array([d["longest_chain"] for d in info], dtype=np.int64)
        if case["name"].startswith("fragments"):
            assert info[3]["longest_chain"] >= 64 and info[3]["rounds"] >= 7, "the fragmented case is meant to have long chains"
    return g


def build_digests():
    d = {}
    for case in production_cases():
        info = []
        out = expected(case, "numpy", info=info, check=True)
        d[case["name"]] = dict(sha256=hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest(),
                               dims=[int(case[s]) for s in ("b", "h", "w", "c", "seed")],
                               grid=[int(v) for v in case["prog"].iarg[0, 0, :2]], min_size=int(case["prog"].iarg[0, 0, 5]),
                               components=[q["components"] for q in info], segments=[q["segments"] for q in info],
                               rounds=[q["rounds"] for q in info], longest_chain=[q["longest_chain"] for q in info])
    return d


def load_cases(g):
    """the cases of a loaded fixture: dicts with the program arrays and the expected images ([B,H,W,C] again)"""
    out = []
    for k in sorted(f[:-4] for f in g.files if f.endswith("_name")):
        b, h, w, c, seed = (int(v) for v in g[k + "dims"])
        out.append(dict(name=str(g[k + "name"]), kind=str(g[k + "kind"]), b=b, h=h, w=w, c=c, seed=seed, opcode=g[k + "opcode"],
                        iarg=g[k + "iarg"], farg=g[k + "farg"], table=g[k + "table"], seed_arr=g[k + "seed"],
                        segments=g[k + "segments"], components=g[k + "components"], longest_chain=g[k + "longest_chain"],
                        u8=np.ascontiguousarray(np.moveaxis(g[k + "u8"], 1, -1))))
    return out


if __name__ == "__main__":
    print("restatements agree on %d values" % check_restatement(small_cases() + production_cases()))
    g, d = build(), build_digests()
    np.savez_compressed(OUT, **g)
    with open(OUT_DIGESTS, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays;", OUT_DIGESTS)
