"""CPU checks of the photometric edge table (tests/photometric_edge_cases.py): every shape reaches the
kernel path it names (the arithmetic of csrc/photometric.hip's dispatch, restated here), the table is band-free (no excusable
pixel in any case, which is what lets tests/test_photometric_edges_gpu.py demand equality), the scipy and the numpy backend of
scripts/make_photometric_golden.py agree on it, a third twin in plain Python loops with the closed-form reflect index agrees
on the small shapes, the cases tell a wrong border, a wrong channel and a wrong random counter from the right one (the
REFERENCE is what gets mutated here, never a kernel), and the digests are the recorded ones
(tests/golden/photometric_edges.json, ``scripts/make_photometric_golden.py --edges``).  No GPU and no library load.

scipy runs in a child process (see tests/test_eval_metrics.py)."""
import importlib.util
import json
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import photometric_edge_cases as T

G = T.G
RECORDED = json.load(open(T.JSON_PATH))
IDS = [cs.name for cs in T.CASES]
needs_scipy = pytest.mark.skipif(importlib.util.find_spec("scipy") is None, reason="the restatement needs scipy")

# csrc/photometric.hip, restated
K_ROWS, MAX_R, MAX_STAGE_ROW, MAX_TILE_ROW = 16, 12, 352, 256


def twpx(c):
    return 64 if c == 3 else MAX_TILE_ROW // c


def cdiv(a, b):
    return -(-a // b)


def paths(cs):
    """what the host and the kernels derive from a shape"""
    h, w, c = cs.h, cs.w, cs.c
    return dict(tiles_x=cdiv(w, twpx(c)), tiles_y=cdiv(h, K_ROWS), last_tile_px=w - (cdiv(w, twpx(c)) - 1) * twpx(c), rows_left=h % K_ROWS,
                vec_n=(w * c) % 16 == 0, vec_p=(h * w * c) % 16 == 0, blocks_p=cdiv(cdiv(h * w * c, 16), 256), tail_p=(h * w * c) % 16)


# ---------------------------------------------------------------------------------------------- the table
def test_the_table_reaches_what_it_names():
    by = {cs.name: cs for cs in T.OPS_CASES}
    assert [(cs.name, cs.h, cs.w, cs.c) for cs in T.OPS_CASES] == [
        ("c1_two_tiles_tail", 17, 257, 1), ("c1_two_tiles_vec", 16, 272, 1), ("c2_tail", 18, 129, 2), ("c2_vec", 16, 136, 2),
        ("c3_tail", 17, 65, 3), ("c3_three_y_tiles", 33, 70, 3), ("c4_tail", 19, 65, 4), ("c4_vec", 16, 68, 4),
        ("flags_disagree", 2, 40, 3), ("tiny_c1", 5, 7, 1), ("tiny_c2", 5, 7, 2), ("tiny_c3", 5, 7, 3), ("tiny_c4", 5, 7, 4),
        ("one_row", 1, 9, 1), ("one_col", 9, 1, 3), ("three_by_three_c4", 3, 3, 4), ("one_pixel", 1, 1, 1),
        ("production_grey", 224, 224, 1)]
    assert [twpx(c) for c in (1, 2, 3, 4)] == [256, 128, 64, 64]
    assert [(twpx(c) + 2 * MAX_R) * c for c in (1, 2, 3, 4)] == [280, 304, 264, MAX_STAGE_ROW]      # the staged rows
    p = {name: paths(cs) for name, cs in by.items()}

    q = p["c1_two_tiles_tail"]      # a one-pixel second x tile, a one-row second y tile, byte stores, a second pointwise block
    assert (q["tiles_x"], q["last_tile_px"], q["tiles_y"], q["rows_left"]) == (2, 1, 2, 1) and not q["vec_n"] and not q["vec_p"]
    assert q["blocks_p"] == 2 and q["tail_p"] == 1
    q = p["c1_two_tiles_vec"]       # a partial second x tile of exactly one 16-byte chunk, everything vectorised
    assert (q["tiles_x"], q["last_tile_px"], q["tiles_y"], q["rows_left"]) == (2, 16, 1, 0) and q["vec_n"] and q["vec_p"]
    q = p["c2_tail"]
    assert (q["tiles_x"], q["last_tile_px"], q["tiles_y"], q["rows_left"]) == (2, 1, 2, 2) and not q["vec_n"] and not q["vec_p"]
    q = p["c2_vec"]
    assert (q["tiles_x"], q["last_tile_px"], q["rows_left"]) == (2, 8, 0) and q["vec_n"] and q["vec_p"]
    q = p["c3_tail"]                # 195-byte rows; the pointwise tail ends inside the last pixel's lane: pix runs past H W
    assert (q["tiles_x"], q["last_tile_px"], q["tiles_y"], q["rows_left"]) == (2, 1, 2, 1) and not q["vec_n"] and not q["vec_p"]
    assert by["c3_tail"].w * 3 == 195 and q["tail_p"] == 3 and (17 * 65 * 3 // 16 * 16 + 15) // 3 >= 17 * 65
    q = p["c3_three_y_tiles"]       # the middle tile's rows 16..31: a halo of 1 stays inside 0..32; a one-row last tile
    assert (q["tiles_x"], q["tiles_y"], q["rows_left"]) == (2, 3, 1) and not q["vec_n"]
    first, last, h = K_ROWS, 2 * K_ROWS - 1, by["c3_three_y_tiles"].h
    assert first - 1 >= 0 and last + 1 == h - 1, "r = 1 reads rows 15..32, all inside; r = 2 already reflects off the bottom"
    q = p["c4_tail"]
    assert (q["tiles_x"], q["last_tile_px"], q["tiles_y"], q["rows_left"]) == (2, 1, 2, 3) and not q["vec_n"] and not q["vec_p"]
    assert by["c4_tail"].w * 4 == 260
    q = p["c4_vec"]
    assert (q["tiles_x"], q["last_tile_px"], q["rows_left"]) == (2, 4, 0) and q["vec_n"] and q["vec_p"]
    q = p["flags_disagree"]         # the two kernels disagree on vectorisation
    assert q["vec_p"] and not q["vec_n"] and (40 * 3) % 16 == 8
    q = p["production_grey"]
    assert (q["tiles_x"], q["tiles_y"], q["rows_left"]) == (1, 14, 0) and q["vec_n"] and q["vec_p"]
    # every *_tail shape puts the samples behind the first on misaligned bases
    assert all(p[n]["tail_p"] for n in T.TAILS)

    # below the halo: the Gaussian's r = 12 and the median's r = 5 wrap / clamp more than once around 5 x 7; n == 1 on
    # either axis; a window larger than the image on both
    for name in ("tiny_c1", "tiny_c2", "tiny_c3", "tiny_c4"):
        cs = by[name]
        assert MAX_R > 2 * (cs.h - 1) and MAX_R > 2 * (cs.w - 1) - 1 and 11 // 2 >= cs.h and cs.c == int(name[-1])
    assert (by["one_row"].h, by["one_col"].w) == (1, 1) and by["one_row"].w > 1 and by["one_col"].h > 1
    cs = by["three_by_three_c4"]      # every window above 3 wide (k >= 4, the Gaussian above r = 1) is larger than the image
    assert (cs.h, cs.w, cs.c) == (3, 3, 4) and by["one_pixel"].h * by["one_pixel"].w == 1
    assert {cs.name for cs in T.OPS_CASES if cs.h * cs.w <= T.LOOPS_AT_MOST} == set(T.SMALL)


def test_every_operator_case_holds_every_opcode_and_corner():
    for cs in T.OPS_CASES:
        ops = [r[0] for r in cs.rows]
        want = set(range(1, 12)) - (set() if cs.c in (1, 3) else {G.GRAYSCALE})
        assert set(ops) == want and ops == sorted(ops) and len(ops) == (33 if cs.c in (1, 3) else 30), cs.name
        assert cs.prog.opcode.shape == (len(ops), 1) and [int(v) for v in cs.prog.opcode[:, 0]] == ops
        ia, fa = cs.prog.iarg[:, 0], cs.prog.farg[:, 0]
        sel = lambda op: np.array(ops) == op
        assert {1, 12} <= set(ia[sel(G.GAUSSIAN_BLUR), 0]) and set(ia[sel(G.AVERAGE_BLUR), 0]) == {2, 4, 7}
        assert set(ia[sel(G.MEDIAN_BLUR), 0]) == {3, 7, 11}
        for op in (G.GAUSSIAN_NOISE, G.DROPOUT, G.COARSE_DROPOUT):
            assert set(ia[sel(op), 0]) == {0, 1}, (cs.name, op)
        assert len(set(ia[sel(G.ADD)][0, :4])) > 2 and len(set(fa[sel(G.MULTIPLY)][0, :4])) == 4 and 5 in set(ia[sel(G.INVERT), 0])
        # every blur opcode sees random content and a smooth field; no two channels hold the same bytes
        assert len(cs.smooth) == 4 and sorted(ops[i] for i in cs.smooth) == list(T.BLURS)
        x = T.images_of(cs)
        if cs.h * cs.w >= 9:
            assert all(not np.array_equal(x[..., a], x[..., b]) for a in range(cs.c) for b in range(a))
            assert all(not np.array_equal(x[i], x[j]) for i in range(3) for j in range(i))


def test_the_chains_put_two_neighbourhood_operators_next_to_each_other():
    assert [cs.name for cs in T.CHAIN_CASES[:4]] == ["chain_c1", "chain_c2", "chain_c3", "chain_c4"]
    for cs, shape in zip(T.CHAIN_CASES, (s for _, s in T.CHAIN_SHAPES)):
        src = T.BY_NAME[shape]
        assert (cs.h, cs.w, cs.c) == (src.h, src.w, src.c) and cs.prog.opcode.shape == (4, 5) and np.all(cs.prog.opcode != 0)
        assert len(set(cs.rows)) == 4, "every sample its own order"
        for i, ops in enumerate(cs.rows):
            assert len(set(ops)) == 5 and ops[i] in T.BLURS and ops[i + 1] in T.BLURS, (cs.name, i, ops)
            assert G.GRAYSCALE not in ops or cs.c in (1, 3)
    for (name, shape), c in zip(T.CHAIN_SHAPES[:4], (1, 2, 3, 4)):
        assert shape in T.TAILS and T.BY_NAME[name].c == c
    assert {op for cs in T.CHAIN_CASES for ops in cs.rows for op in ops} == set(range(1, 12))


def test_the_host_rejects_grayscale_at_two_and_four_channels():
    import torch
    from pointcloududa_amd.utils.photometric import PhotoProgram, upload_program
    src = T.BY_NAME["tiny_c3"]
    rows = [i for i, r in enumerate(src.rows) if r[0] == G.GRAYSCALE]
    assert len(rows) == 3
    prog = PhotoProgram(*(np.ascontiguousarray(a[rows]) for a in T.arrays_of(src)))
    for c in (1, 3):
        prog.validate(c)
        upload_program(prog, 3, 5, 7, c, torch.device("cpu"))
    for c in (2, 4):
        with pytest.raises(ValueError, match="GRAYSCALE takes 3 channels"):
            prog.validate(c)
        with pytest.raises(ValueError, match="GRAYSCALE takes 3 channels"):
            upload_program(prog, 3, 5, 7, c, torch.device("cpu"))
    # and what the table does hold passes the host's validation at its own channel count
    for cs in T.CASES:
        PhotoProgram(*T.arrays_of(cs)).validate(cs.c)


# ---------------------------------------------------------------------------------------------- band-free, two backends, digests
@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_no_excused_pixel_and_the_recorded_digest(case):
    """a condition, not a tolerance: no pre-rounding value of the restatement within G.EPS of a rounding boundary"""
    out, exc = T.expected(case)
    assert out.dtype == np.uint8 and out.shape == T.images_of(case).shape
    assert not exc.any(), (case.name, int(exc.sum()), "change the case's seed")
    assert T.digests_of(case) == RECORDED["cases"][case.name]


def test_the_recorded_file_holds_digests_only():
    assert sorted(RECORDED) == ["cases", "numpy_version"] and RECORDED["numpy_version"]
    assert sorted(RECORDED["cases"]) == sorted(IDS)
    for cs in T.CASES:
        rec = RECORDED["cases"][cs.name]
        assert sorted(rec) == ["batch", "expected", "shape"] and rec["shape"] == [cs.h, cs.w, cs.c] and rec["batch"] == len(cs.rows)
        assert isinstance(rec["expected"], str) and len(rec["expected"]) == 64
    assert os.path.getsize(T.JSON_PATH) < 8192


@needs_scipy
def test_the_scipy_backend_equals_the_numpy_backend_on_every_case():
    code = "import sys, numpy as np\nsys.path.insert(0, %r)\nimport photometric_edge_cases as T\n" % os.path.dirname(os.path.abspath(__file__))
    body = """
        n = 0
        for cs in T.CASES:
            (a, ea), (b, eb) = T.expected(cs, "scipy"), T.expected(cs, "numpy")
            assert np.array_equal(a, b), (cs.name, int((a != b).sum()))
            assert not ea.any() and not eb.any(), cs.name
            n += a.size
        assert n > 2800000, n
    """
    r = subprocess.run([sys.executable, "-c", code + textwrap.dedent(body)], capture_output=True, text=True,
                       env=dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1"), timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------- a third twin: plain loops
def reflect_closed_form(i, n):
    """the rule csrc/photometric.hip implements: i mod 2 (n - 1), folded; n == 1 -> 0"""
    if n == 1:
        return 0
    period = 2 * (n - 1)
    i %= period                     # (Python's % is non-negative)
    return i if i < n else period - i


def replicate(i, n):
    return min(max(i, 0), n - 1)


def round_u8(v):
    return int(min(max(math.floor(v + 0.5), 0), 255))


def loops(img, op, ia, fa):
    """one neighbourhood slot on uint8 [H,W,C] in Python integer loops, no np.pad -> uint8 [H,W,C]"""
    h, w, c = img.shape
    px = [[[int(img[y, x, ch]) for ch in range(c)] for x in range(w)] for y in range(h)]
    out = np.zeros((h, w, c), dtype=np.uint8)
    k = int(ia[0])
    wts = [float(v) for v in fa]
    at = replicate if op == G.MEDIAN_BLUR else reflect_closed_form
    if op == G.GAUSSIAN_BLUR:                   # rows first, then along x on the unrounded values
        r = k
        mid = [[[0.0] * c for _ in range(w)] for _ in range(h)]
        for y in range(h):
            for x in range(w):
                for ch in range(c):
                    t = px[y][x][ch] * wts[0]
                    for d in range(r, 0, -1):
                        t += (px[at(y - d, h)][x][ch] + px[at(y + d, h)][x][ch]) * wts[d]
                    mid[y][x][ch] = t
    for y in range(h):
        for x in range(w):
            for ch in range(c):
                if op == G.GAUSSIAN_BLUR:
                    t = mid[y][x][ch] * wts[0]
                    for d in range(k, 0, -1):
                        t += (mid[y][at(x - d, w)][ch] + mid[y][at(x + d, w)][ch]) * wts[d]
                    out[y, x, ch] = round_u8(t)
                elif op == G.AVERAGE_BLUR:
                    lo, hi = -(k // 2), k - k // 2 - 1
                    s = sum(px[at(y + dy, h)][at(x + dx, w)][ch] for dy in range(lo, hi + 1) for dx in range(lo, hi + 1))
                    out[y, x, ch] = (2 * s + k * k) // (2 * k * k)
                elif op == G.MEDIAN_BLUR:
                    r = k // 2
                    win = sorted(px[at(y + dy, h)][at(x + dx, w)][ch] for dy in range(-r, r + 1) for dx in range(-r, r + 1))
                    out[y, x, ch] = win[(k * k - 1) // 2]
                else:
                    t = 0.0
                    for i in range(9):
                        t += px[at(y + i // 3 - 1, h)][at(x + i % 3 - 1, w)][ch] * wts[i]
                    out[y, x, ch] = round_u8(t)
    return out


def test_reflect_closed_form_is_numpy_pad_iterated():
    for n in (1, 2, 3, 5, 7, 9):
        pad = np.pad(np.arange(n), (12, 12), mode="reflect")
        assert [reflect_closed_form(i, n) for i in range(-12, n + 12)] == pad.tolist(), n


@pytest.mark.parametrize("name", T.SMALL)
def test_plain_loops_equal_the_restatement_on_the_small_shapes(name):
    """the four neighbourhood operators at every corner where H W <= 64: this pins np.pad's iterated reflection (and scipy's
    "mirror") against the closed-form index, n == 1 included"""
    cs = T.BY_NAME[name]
    assert cs.h * cs.w <= T.LOOPS_AT_MOST
    x, (want, _) = T.images_of(cs), T.expected(cs)
    n = 0
    for i, (op,) in enumerate(cs.rows):
        if op in T.BLURS:
            got = loops(x[i], op, cs.prog.iarg[i, 0], cs.prog.farg[i, 0])
            assert np.array_equal(got, want[i]), (name, G.NAMES[op], i, np.argwhere(got != want[i])[:5].tolist())
            n += 1
    assert n == 13


# ---------------------------------------------------------------------------------------------- the cases discriminate
class _SwappedBorders:
    """numpy, with np.pad's "reflect" and "edge" exchanged: the restatement with the wrong border on every operator"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def pad(a, width, mode):
        return np.pad(a, width, mode={"reflect": "edge", "edge": "reflect"}[mode])


def _slot(cs, i, img=None, s=0):
    """the pre-rounding values of slot s of sample i, rounded"""
    v = G.op_values(T.images_of(cs)[i] if img is None else img, int(cs.prog.opcode[i, s]), cs.prog.iarg[i, s], cs.prog.farg[i, s],
                    int(cs.prog.seed[i, s]), "numpy")[0]
    return G.to_u8(v) if v.dtype == np.float64 else v.astype(np.uint8)


@pytest.mark.parametrize("name", [n for n in T.SMALL if n != "one_pixel"] + list(T.TAILS))
def test_a_wrong_border_changes_the_expected_output(name, monkeypatch):
    """edge-replicate in place of reflect-101 for the Gaussian, the average and the 3x3, reflect in place of replicate for the
    median: every small and *_tail case tells them apart for every one of the four operators (a one-pixel image has one
    border), and the *_tail cases in every row but the one whose operator is the identity after rounding whatever the
    border (the Gaussian at sigma just above 0.125, whose w[1] is below exp(-15)).  On the few texels of a small shape a
    saturating sharpen may round both borders to the same 0 / 255: there one row per operator is what is asked"""
    cs = T.BY_NAME[name]
    rows = [i for i, r in enumerate(cs.rows) if r[0] in T.BLURS]
    right = [_slot(cs, i) for i in rows]
    for i, a in zip(rows, right):
        assert np.array_equal(a, T.expected(cs)[0][i])
    monkeypatch.setattr(G, "np", _SwappedBorders())
    wrong = [_slot(cs, i) for i in rows]
    monkeypatch.undo()
    told = {op: 0 for op in T.BLURS}
    for i, a, b in zip(rows, right, wrong):
        if np.array_equal(a, T.images_of(cs)[i]) and np.array_equal(b, a):
            assert cs.rows[i][0] == G.GAUSSIAN_BLUR and cs.prog.iarg[i, 0, 0] == 1 and cs.prog.farg[i, 0, 1] < math.exp(-15.0), (name, i)
            continue
        told[cs.rows[i][0]] += not np.array_equal(a, b)
    assert all(told.values()), (name, told)
    if name in T.TAILS:
        assert sum(told.values()) == 12, (name, told)


@pytest.mark.parametrize("name", [cs.name for cs in T.OPS_CASES if cs.c > 1 and cs.h * cs.w > 1])
def test_rolled_channels_change_the_expected_output(name):
    """a kernel that reads channel ch + 1 where it means ch: every blur row changes, because no two channels hold the same
    content; and ADD, MULTIPLY and INVERT with per-channel arguments change when the ARGUMENT of the next channel is taken"""
    cs = T.BY_NAME[name]
    x, want = T.images_of(cs), T.expected(cs)[0]
    per_channel = 0
    for i, (op,) in enumerate(cs.rows):
        rolled = np.roll(x[i], 1, axis=-1)
        if op in T.BLURS:
            assert not np.array_equal(_slot(cs, i, rolled), want[i]), (name, G.NAMES[op], i)
        elif op in (G.ADD, G.MULTIPLY, G.INVERT):
            ia, fa = cs.prog.iarg[i, 0], cs.prog.farg[i, 0]
            args = [(ia[0] >> ch) & 1 for ch in range(cs.c)] if op == G.INVERT else list((ia if op == G.ADD else fa)[:cs.c])
            if len(set(args)) > 1:
                assert not np.array_equal(np.roll(_slot(cs, i, rolled), -1, axis=-1), want[i]), (name, G.NAMES[op], i)
                per_channel += 1
    assert per_channel == 3, "one row with per-channel arguments for each of ADD, MULTIPLY and INVERT"


@pytest.mark.parametrize("name", [cs.name for cs in T.OPS_CASES if cs.c > 1])
def test_the_random_draw_is_shared_by_a_pixels_channels_exactly_when_not_per_channel(name):
    cs = T.BY_NAME[name]
    x = T.images_of(cs)
    big = cs.h * cs.w >= 1000                   # enough draws that independent channels cannot coincide
    seen = set()
    for i, (op,) in enumerate(cs.rows):
        if op not in (G.GAUSSIAN_NOISE, G.DROPOUT, G.COARSE_DROPOUT):
            continue
        ia, fa, seed = cs.prog.iarg[i, 0], cs.prog.farg[i, 0], int(cs.prog.seed[i, 0])
        pc = bool(ia[0])
        seen.add((op, pc))
        v = G.op_values(x[i], op, ia, fa, seed, "numpy")[0]
        if op == G.GAUSSIAN_NOISE:
            draw = G.op_values(np.zeros_like(x[i]), op, ia, fa, seed, "numpy")[0]      # 0 + scale z, unrounded
            assert np.abs(draw).max() > 0 and np.abs(v - (x[i] + draw)).max() < 1e-9
        else:
            draw = G.op_values(np.full_like(x[i], 9), op, ia, fa, seed, "numpy")[0] == 0      # the dropped elements
            assert np.array_equal(v == 0, draw | (x[i] == 0))
        shared = all(np.array_equal(draw[..., 0], draw[..., ch]) for ch in range(1, cs.c))
        if not pc:
            assert shared, (name, G.NAMES[op], i)
        elif big and op != G.COARSE_DROPOUT:    # (a coarse grid of a small image has a handful of cells)
            assert not shared, (name, G.NAMES[op], i)
    assert seen >= {(G.GAUSSIAN_NOISE, False), (G.GAUSSIAN_NOISE, True), (G.DROPOUT, False), (G.DROPOUT, True),
                    (G.COARSE_DROPOUT, False), (G.COARSE_DROPOUT, True)}


def test_the_pointwise_tail_counts_pixels_where_it_is_not_per_channel():
    """the ragged last chunk of c3_tail and c2_tail: a kernel that fed the per-ELEMENT counter to a per-pixel row (or the
    reverse) gives other bytes in the last sixteen elements of a sample"""
    for name in ("c3_tail", "c2_tail", "c4_tail"):
        cs = T.BY_NAME[name]
        x, want = T.images_of(cs), T.expected(cs)[0]
        n = 0
        for i, (op,) in enumerate(cs.rows):
            if op == G.DROPOUT or (op == G.GAUSSIAN_NOISE and cs.prog.farg[i, 0, 0] > 1.0):      # (the third noise corner's scale is near 0)
                ia = cs.prog.iarg[i, 0].copy()
                ia[0] ^= 1
                other = G.op_values(x[i], op, ia, cs.prog.farg[i, 0], int(cs.prog.seed[i, 0]), "numpy")[0]
                other = G.to_u8(other) if other.dtype == np.float64 else other.astype(np.uint8)
                assert not np.array_equal(other, want[i])
                if op == G.GAUSSIAN_NOISE:
                    assert not np.array_equal(other.ravel()[-16:], want[i].ravel()[-16:]), (name, i)
                n += 1
        assert n == 4
