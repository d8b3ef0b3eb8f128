"""CPU checks of the CropAndPad edge table (tests/croppad_edge_cases.py): every row is valid and every
mode meets every side set of its shape, the restatement equals numpy.pad live on every row, its digests are the recorded ones
(tests/golden/croppad_edges.json, ``scripts/make_croppad_golden.py --edges``), the planted ramp texels flip exactly their side,
and the workspace holds the statistics table of every shape."""
import json

import numpy as np
import pytest

import croppad_edge_cases as T

G = T.G
RECORDED = json.load(open(T.JSON_PATH))
IDS = [cs.name for cs in T.CASES]


def test_the_table_reaches_what_it_names():
    by = T.BY_NAME
    assert {(cs.h, cs.w, cs.c) for cs in T.CASES if cs.kind == "modes"} == {
        (18, 65, 1), (18, 65, 3), (17, 128, 1), (20, 66, 2), (19, 65, 4), (16, 64, 4), (80, 70, 3), (130, 90, 3), (256, 256, 3),
        (224, 224, 1)}
    for cs in T.CASES:
        assert all(G.sides_valid(cs.h, cs.w, *r[:4]) for r in cs.rows), cs.name
        if cs.kind != "modes":
            continue
        # pads only, crops only, mixed, the largest valid pad; every mode meets every set, ten modes per batch
        assert len(cs.sets) >= 4 and len(cs.rows) == 10 * len(cs.sets), cs.name
        assert all(min(s) >= 0 for s in cs.sets[:1]) and all(max(s) <= 0 for s in cs.sets[1:2]), cs.name
        assert min(cs.sets[2]) < 0 < max(cs.sets[2]), cs.name
        assert cs.sets[3] == (min(64, cs.h - 1), min(64, cs.w - 1)) * 2, cs.name
        assert {(r[4], r[:4]) for r in cs.rows} == {(m, tuple(s)) for m in range(10) for s in cs.sets}, cs.name
        for r in range(len(cs.sets)):
            assert [row[4] for row in cs.rows[10 * r:10 * r + 10]] == list(range(10)), cs.name
    # the word stores with a partial last group; C = 4; lines above a wave; pads of exactly 64 with both flag loops above 256
    w, c = by["c2_vec_tail"].w, by["c2_vec_tail"].c
    assert (w * c) % 4 == 0 and w % 4 == 2
    assert by["two_tiles_full"].w % 4 == 0 and by["c4_tail"].w % 4 and by["c4_full"].w % 4 == 0
    hc_wc = [(cs.h - G.split_sides(cs.h, cs.w, *s)[0] - G.split_sides(cs.h, cs.w, *s)[1],
              cs.w - G.split_sides(cs.h, cs.w, *s)[2] - G.split_sides(cs.h, cs.w, *s)[3])
             for cs in T.CASES if cs.name.startswith("long_lines") for s in cs.sets]
    assert min(min(p) for p in hc_wc) > 64
    mp = by["max_pad"]
    assert (64, 64, 64, 64) in mp.sets and mp.w * mp.c == 270 and mp.h * mp.c == 390
    assert by["production_256"].sets[4:] == [(-12, 25, 25, -12), (-13, 26, 26, -13)]
    assert by["production_224"].sets[4:] == [(-10, 22, 22, -10), (-11, 22, 22, -11)]
    for cs in T.CASES:
        if cs.kind == "stats":
            assert {r[4] for r in cs.rows} == {3, 4, 5, 6} and (9, 0, 7, 0) in cs.sets and (0, 6, 0, 11) in cs.sets
    assert sorted(np.unique(T.labels_for(16, 64)).tolist()) == sorted(T.LABEL_VALUES)


def test_the_built_images_hold_what_they_promise():
    few = T.image_of(T.BY_NAME["long_lines_few"])
    assert sorted(np.unique(few).tolist()) == [0, 131, 255]
    const = T.image_of(T.BY_NAME["long_lines_const"])
    assert all(len(np.unique(const[..., k])) == 1 for k in range(3))
    for name, axis in (("long_lines_half_cols", 0), ("long_lines_half_rows", 1)):
        img = np.moveaxis(T.image_of(T.BY_NAME[name]).astype(np.int64), axis, 0)[:66]      # [66, lines, C]
        lo = img.min(0)
        assert np.all((img == lo).sum(0) == 33) and np.all((img == lo + 1).sum(0) == 33)
        assert np.any(lo % 2 == 0) and np.any(lo % 2 == 1)
        # mean and median of such a line are k + 0.5: numpy.pad rounds them to the even neighbour
        cs = T.BY_NAME[name]
        sides = (9, 0, -14, 0) if axis == 0 else (0, -4, 0, 11)
        for mode in (4, 5):
            big = T.expected_rows(cs)[cs.rows.index(sides + (mode, 0))][0]
            got = big[0, :, :] if axis == 0 else big[:, 0, :]
            even = lo + (lo % 2)
            assert np.array_equal(got, even if axis == 0 else even[:, :]), (name, mode)


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_restatement_equals_numpy_pad_and_the_recorded_digests(case):
    x = T.image_of(case)
    for row, (big, _) in zip(case.rows, T.expected_rows(case)):
        pt, pb, pl, pr = G.split_sides(case.h, case.w, *row[:4])[4:]
        want = G.numpy_pad(G.crop(x, *row[:4]), pt, pb, pl, pr, row[4], row[5])
        assert big.dtype == want.dtype and big.shape == want.shape and np.array_equal(big, want), (case.name, row)
    assert T.digests_of(case) == RECORDED["cases"][case.name]


def test_the_recorded_file_holds_digests_only():
    assert sorted(RECORDED) == ["cases", "numpy_version"] and RECORDED["numpy_version"]
    assert sorted(RECORDED["cases"]) == sorted(IDS)
    for cs in T.CASES:
        rec = RECORDED["cases"][cs.name]
        assert sorted(rec) == ["labels", "rows", "shape"] and rec["shape"] == [cs.h, cs.w, cs.c]
        assert len(rec["rows"]) == len(cs.rows) and len(rec["labels"]) == len(cs.sets)
        assert all(isinstance(d, str) and len(d) == 64 for d in rec["rows"] + rec["labels"])


@pytest.mark.parametrize("side", ("top", "right", "bottom", "left"))
def test_a_planted_ramp_texel_flips_exactly_its_side(side):
    """numpy.pad of the planted image against numpy.pad of the same image with the planted texel one higher: the other form of
    linspace on that side's pad region (corners included), and outside it nothing but the texel itself"""
    (y, x, k), sides = T.RAMP_PLANTS[side]
    a = T.ramp_image(side)
    b = a.copy()
    assert a[y, x, k] == T.RAMP_CVAL
    b[y, x, k] += 1
    edge = {"top": a[0], "bottom": a[-1], "left": a[:, 0], "right": a[:, -1]}
    assert {s: int((e == T.RAMP_CVAL).sum()) for s, e in edge.items()} == {s: int(s == side) for s in edge}
    assert (x if side in ("top", "bottom") else y) * 3 + k >= 256
    pt, pb, pl, pr = G.split_sides(130, 90, *sides)[4:]
    pa, pb_ = G.numpy_pad(a, pt, pb, pl, pr, 2, T.RAMP_CVAL), G.numpy_pad(b, pt, pb, pl, pr, 2, T.RAMP_CVAL)
    diff = (pa != pb_).any(-1)
    band = T.side_band(side, diff.shape, sides)
    own = np.zeros_like(diff)
    own[pt + y, pl + x] = True
    assert not np.any(diff & ~band & ~own)
    line = np.zeros_like(diff)
    if side in ("top", "bottom"):
        line[:, pl + x] = True
    else:
        line[pt + y] = True
    assert np.any(diff & band & ~line), "the two forms differ away from the planted texel's own line"
    # and the planted image against the unplanted one, as the GPU test compares them
    base = G.numpy_pad(T.ramp_base_image(), pt, pb, pl, pr, 2, T.RAMP_CVAL)
    d2 = (pa != base).any(-1)
    assert np.any(d2 & band & ~line) and not np.any(d2 & ~band & ~own)
    # the same in the resized outputs, in the regions that the GPU test looks at
    plain = T.BY_NAME["max_pad_ramp_none_" + ("all" if sides == T.RAMP_ALL else "lr")]
    d3 = (T.expected_rows(T.BY_NAME["max_pad_ramp_" + side])[0][1] != T.expected_rows(plain)[0][1]).any(-1)
    inside, outside = T.ramp_output_regions(side)
    assert d3[inside].any() and not d3[outside].any()


def test_the_workspace_holds_the_table_of_every_shape():
    from pointcloududa_amd import _lib
    size = _lib.lib().pcuda_crop_pad_workspace_size
    for h, w, c in sorted({(cs.h, cs.w, cs.c) for cs in T.CASES}):
        for b in (1, 10):
            need = size(b, h, w, c)
            assert need % 16 == 0 and need >= b * c * (w + h + 128) + 4 * b, (b, h, w, c)
