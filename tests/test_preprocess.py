"""CPU checks of the device-side slice preparation (pointcloududa_amd/utils/preprocess.py, csrc/preprocess.hip; DESIGN.md
section 6, f11): the two restatements of the convention (vectorised numpy / plain Python loops, scripts/make_preprocess_golden.py)
against the committed fixture and against each other, the branches the fixture's cases reach, properties of the convention,
the host-side validation, and the C declaration against the binding.  No GPU and no library load."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import GOLD, ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
GEN = os.path.join(ROOT, "scripts", "make_preprocess_golden.py")


def _helper():
    spec = importlib.util.spec_from_file_location("make_preprocess_golden", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _helper()
CLAHE_CASES, RESCALE_CASES = G.load_cases(np.load(os.path.join(GOLD, "preprocess.npz")))
F = np.float32


def _case(name):
    return next(c for c in CLAHE_CASES if c["name"] == name)


def _report(c):
    rep = []
    G.clahe_loops(c["images"], c["clip_limit"], c["grid"], rep)
    return rep                       # per tile: (clip, clipped, batch, residual, step)


# ---------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("case", CLAHE_CASES, ids=[c["name"] for c in CLAHE_CASES])
def test_both_clahe_restatements_reproduce_the_golden(case):
    a = G.clahe_numpy(case["images"], case["clip_limit"], case["grid"])
    b = G.clahe_loops(case["images"], case["clip_limit"], case["grid"])
    assert G.bit_equal(a, case["expected"]) and G.bit_equal(b, case["expected"])
    assert case["expected"].dtype == np.uint8 and case["expected"].shape == case["images"].shape


@pytest.mark.parametrize("case", RESCALE_CASES, ids=[c["name"] for c in RESCALE_CASES])
def test_both_rescale_restatements_reproduce_the_golden(case):
    a = G.rescale_numpy(case["volume"], case["resize_h"], case["resize_w"], case["crop"])
    b = G.rescale_loops(case["volume"], case["resize_h"], case["resize_w"], case["crop"])
    assert G.bit_equal(a, case["expected"]) and G.bit_equal(b, case["expected"])
    side = 2 * (case["crop"] // 2)
    want = (side, side) if case["crop"] else (case["resize_h"], case["resize_w"])
    assert case["expected"].dtype == np.uint8 and case["expected"].shape == (case["volume"].shape[0],) + want


def test_the_fixture_regenerates_exactly_and_is_small():
    assert G.check_file() == 4 * (len(CLAHE_CASES) + len(RESCALE_CASES))
    assert os.path.getsize(os.path.join(GOLD, "preprocess.npz")) < 1000 * 1000


def test_the_luts_of_the_two_restatements_agree():
    for c in CLAHE_CASES:
        for img in c["images"]:
            a = G.clahe_luts_numpy(img, c["clip_limit"], *c["grid"])
            b = np.array(G.clahe_luts_loops(img.tolist(), c["clip_limit"], *c["grid"]), dtype=np.uint8)
            assert G.bit_equal(a, b), c["name"]


def test_fixture_case_set_reaches_the_branches_it_is_there_for():
    names = [c["name"] for c in CLAHE_CASES]
    assert len(set(names)) == len(names) == 16
    P = lambda c: G.clahe_params(c["images"].shape[1], c["images"].shape[2], c["clip_limit"], *c["grid"])
    # divisible; 2.0 * 64 / 256 < 1: the clip is clamped to 1; the residual's steps lie in 13..23
    c = _case("16x16_g2x2_clip2")
    p, rep = P(c), _report(c)
    assert (p["eh"], p["ew"], p["T"], p["clip"]) == (16, 16, 64, 1) and int(2.0 * 64 / 256) == 0
    assert all(13 <= r[4] <= 23 for r in rep) and len(rep) == 4
    # both axes reflected; small residuals, steps up to 256 // 2
    c = _case("17x13_g4x4_clip2")
    p, rep = P(c), _report(c)
    assert (p["eh"], p["ew"], p["th"], p["tw"]) == (20, 16, 5, 4)
    assert {r[3] for r in rep} >= {0, 2, 5} and max(r[4] for r in rep) == 128 and min(r[4] for r in rep if r[3]) >= 36
    # the quirk: 16 % 4 == 0, yet the height grows by a whole tiles_y because the width is indivisible
    c = _case("16x13_g4x4_clip2")
    p, rep = P(c), _report(c)
    assert (p["eh"], p["ew"]) == (20, 16) and c["images"].shape[1] % 4 == 0
    assert {r[4] for r in rep} >= {256, 128}, "residual 1 and 2"
    # 3x5-pixel tiles; the clamps of tx2 / ty2 (and of tx1 / ty1 at the other end) on the outer half tiles
    c = _case("24x40_g8x8_clip4")
    p = P(c)
    assert (p["th"], p["tw"], p["clip"]) == (3, 5, 1)
    xs, ys = G._axis_loops(40, p["inv_tw"], 8), G._axis_loops(24, p["inv_th"], 8)
    assert sum(t1 == t2 for t1, t2, _, _ in xs) >= 5 and sum(t1 == t2 for t1, t2, _, _ in ys) >= 3
    # no clipping; one tile: all four LUTs are the same
    c = _case("32x32_g1x1_clip0")
    assert P(c)["clip"] == 0 and all(r[:4] == (0, 0, 0, 0) for r in _report(c))
    # clip 8 with real clipping (a batch and a residual), clip 160 with none
    c = _case("64x64_g2x2_clip2")
    rep = _report(c)
    assert P(c)["clip"] == 8 and all(r[1] > 0 for r in rep) and any(r[2] > 0 for r in rep)
    c = _case("64x64_g2x2_clip40")
    assert P(c)["clip"] == 160 and all(r[1] == 0 for r in _report(c))
    # residual above 128: step 1
    c = _case("64x64_g4x4_clip0.01")
    rep = _report(c)
    assert P(c)["clip"] == 1 and all(r[3] > 128 and r[4] == 1 for r in rep) and len(rep) == 16
    # the reference's own parameters
    c = _case("224x224_g4x4_clip2_n3")
    rep = _report(c)
    assert c["images"].shape == (3, 224, 224) and (c["clip_limit"], c["grid"]) == (2.0, (4, 4)) and P(c)["clip"] == 24
    assert len(rep) == 48 and {r[4] for r in rep} >= {1, 2, 25} and all(r[2] >= 1 for r in rep)
    # a constant slice: one full bin; 84 everywhere
    c = _case("constant77_16x16_g2x2_clip2")
    assert all(r == (1, 63, 0, 63, 4) for r in _report(c)) and np.all(c["expected"] == 84)
    c = _case("constant9_64x64_g1x1_clip2")
    assert _report(c) == [(32, 4064, 15, 224, 1)] and len(np.unique(c["expected"])) == 1, "batch > 0"
    # edges of the LUT, batch indexing, odd grids, the largest grid, the smallest slice
    c = _case("all0_all255_16x16_g4x4_clip2")
    assert np.all(c["images"][0] == 0) and np.all(c["images"][1] == 255) and np.all(c["expected"][1] == 255)
    assert len(np.unique(c["expected"][0])) == 1
    c = _case("n5_20x28_g2x2_clip3")
    assert c["images"].shape[0] == 5 and len({im.tobytes() for im in c["images"]}) == 5
    assert _case("30x18_g3x5_clip2.5")["grid"] == (3, 5) and _case("64x64_g16x16_clip2")["grid"] == (16, 16)
    assert _case("2x2_g1x1_clip2")["images"].shape == (1, 2, 2)
    # rescale / resize / crop
    by = {c["name"]: c for c in RESCALE_CASES}
    assert len(by) == len(RESCALE_CASES) == 15
    for tag, dt in (("f32", np.float32), ("i16", np.int16), ("u8", np.uint8)):
        a, b = by["%s_3x20x28_to16_crop12" % tag], by["%s_3x20x28_to16_crop0" % tag]
        assert a["volume"].dtype == dt and a["volume"].shape == (3, 20, 28) and a["expected"].shape == (3, 12, 12)
        assert b["expected"].shape == (3, 16, 16) and np.array_equal(a["expected"], b["expected"][:, 2:14, 2:14])
    assert by["i16_3x20x28_to16_crop12"]["volume"].min() < 0
    assert np.all(by["f32_constant_7.5"]["expected"] == 0) and np.all(by["i16_constant_-3"]["expected"] == 0), "hi == lo != 0"
    assert np.all(by["f32_zeros"]["expected"] == 0) and np.all(by["u8_zeros"]["expected"] == 0), "hi == lo == 0"
    c = by["i16_at_target_size_2x16x16_crop12"]
    assert c["volume"].shape[1:] == (c["resize_h"], c["resize_w"])
    assert by["i16_negative_only"]["volume"].max() < 0 and by["i16_negative_only"]["expected"].shape == (2, 12, 12)
    c = by["u8_full_range_identity"]
    assert (c["volume"].min(), c["volume"].max()) == (0, 255) and np.array_equal(c["expected"], c["volume"]), "scale 1, shift -0"


# ---------------------------------------------------------------------------------------------- properties of the convention
def test_clip_limit_zero_equals_a_clip_limit_that_clips_nothing():
    for shape, grid, seed in (((2, 32, 32), (2, 2), 1), ((1, 17, 13), (4, 4), 2), ((1, 64, 64), (1, 1), 3)):
        img = G.slices_u8(shape, seed)
        none = G.clahe_numpy(img, 0.0, grid)
        assert G.bit_equal(none, G.clahe_numpy(img, -1.0, grid))
        for big in (256.0, 1e6, 1e300):
            rep = []
            G.clahe_loops(img, big, grid, rep)
            assert all(r[0] > 0 and r[1] == 0 for r in rep), "a clip limit of 256 puts the clip at T: nothing is clipped"
            assert G.bit_equal(none, G.clahe_numpy(img, big, grid))


def test_one_tile_without_clipping_is_the_global_equalisation_lut():
    img = G.slices_u8((1, 24, 40), 7)[0]
    n = img.size
    cdf = np.cumsum(np.bincount(img.ravel(), minlength=256))
    lut = np.clip(np.rint(cdf.astype(F) * (F(255) / F(n))), 0, 255).astype(np.uint8)
    assert np.array_equal(G.clahe_luts_numpy(img, 0.0, 1, 1)[0, 0], lut)
    assert np.array_equal(G.clahe_numpy(img, 0.0, (1, 1)), lut[img]), "all four LUTs are this one: the blend returns its value"
    assert np.array_equal(G.clahe_loops(img, 0.0, (1, 1)), lut[img])


def test_a_constant_tile_maps_to_one_value():
    for value in (0, 77, 255):
        for grid, clip in (((2, 2), 2.0), ((4, 4), 0.0), ((1, 1), 40.0)):
            out = G.clahe_numpy(np.full((16, 16), value, np.uint8), clip, grid)
            assert len(np.unique(out)) == 1, (value, grid, clip)
    # and a slice whose tiles are constant, each with its own value: a tile's centre takes its tile's own LUT value
    img = np.repeat(np.repeat(np.array([[10, 200], [90, 30]], np.uint8), 8, axis=0), 8, axis=1)
    out = G.clahe_numpy(img, 0.0, (2, 2))
    assert np.all(out[:4, :4] == 255) and np.all(out[12:, 12:] == 255), "cdf(v) = T in a constant tile"


def test_output_shape_and_dtype():
    img = G.random_u8((2, 12, 20), 3)
    for fn in (G.clahe_numpy, G.clahe_loops):
        assert fn(img, 2.0, (4, 4)).shape == (2, 12, 20) and fn(img, 2.0, (4, 4)).dtype == np.uint8
        assert fn(img[0], 2.0, (4, 4)).shape == (12, 20) and G.bit_equal(fn(img[0], 2.0, (4, 4)), fn(img, 2.0, (4, 4))[0])
    f = G.to_float3(G.clahe_numpy(img, 2.0, (4, 4)))
    assert f.shape == (2, 3, 12, 20) and f.dtype == np.float32 and np.array_equal(f[:, 0], f[:, 2]) and 0.0 <= f.min() <= f.max() <= 1.0
    assert f[0, 1, 3, 4] == F(G.clahe_numpy(img, 2.0, (4, 4))[0, 3, 4]) / F(255)
    assert G.rescale_numpy(np.zeros((2, 9, 7), np.int16), 16, 12, 0).shape == (2, 16, 12)
    assert G.rescale_numpy(np.zeros((2, 9, 7), np.int16), 16, 12, 7).shape == (2, 6, 6)


def test_rescale_follows_the_stated_arithmetic():
    vol = np.array([[[-2.0, 0.0, 1.0, 6.0]]], F)
    scale = 255.0 / 8.0
    want = [0, int(0.0 * scale + 2.0 * scale), int(1.0 * scale + 2.0 * scale), int(6.0 * scale + 2.0 * scale)]
    assert G.rescale_numpy(vol).ravel().tolist() == want == G.rescale_loops(vol).ravel().tolist()
    # the nearest resize reads floor(y / (resize / source)): 4 -> 6 reads 0 0 1 2 2 3; 5 -> 3 reads 0 1 3
    row = np.array([[[0, 85, 170, 255]]], np.uint8)
    assert G.rescale_numpy(row, 1, 6).ravel().tolist() == [0, 0, 85, 170, 170, 255]
    col = np.array([0, 51, 102, 204, 255], np.uint8).reshape(1, 5, 1)
    assert G.rescale_numpy(col, 3, 1).ravel().tolist() == [0, 51, 204] == G.rescale_loops(col, 3, 1).ravel().tolist()
    # crop_volume: rows size // 2 - crop // 2 .. size // 2 + crop // 2
    ramp = np.arange(0, 256, 17, dtype=np.uint8)[:15].reshape(1, 15, 1) * np.ones((1, 1, 15), np.uint8)
    ramp[0, 0, :], ramp[0, -1, :] = 0, 255
    assert np.array_equal(G.rescale_numpy(ramp, 15, 15, 6), G.rescale_numpy(ramp, 15, 15, 0)[:, 4:10, 4:10])


# ---------------------------------------------------------------------------------------------- the host side of the package
def test_argument_validation_raises():
    import torch
    from pointcloududa_amd.utils import preprocess as P
    u8 = torch.zeros((2, 16, 16), dtype=torch.uint8)
    for bad in (torch.zeros((2, 16, 16)), torch.zeros((2, 16, 16), dtype=torch.int16), np.zeros((2, 16, 16), np.uint8)):
        with pytest.raises(TypeError, match="uint8"):
            P.clahe(bad)
    for bad in (torch.zeros((16,), dtype=torch.uint8), torch.zeros((1, 2, 16, 16), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="dimensions"):
            P.clahe(bad)
    for grid in ((0, 4), (4, 17), (-1, 2)):
        with pytest.raises(ValueError, match="tiles per axis"):
            P.clahe(u8, tile_grid_size=grid)
    for grid in (4, (4, 4, 4), None):
        with pytest.raises(TypeError, match="tile_grid_size"):
            P.clahe(u8, tile_grid_size=grid)
    with pytest.raises(ValueError, match="2x2"):
        P.clahe(torch.zeros((1, 1, 16), dtype=torch.uint8), tile_grid_size=(1, 1))
    with pytest.raises(ValueError, match="reflected border"):
        P.clahe(torch.zeros((1, 2, 3), dtype=torch.uint8), tile_grid_size=(2, 2))        # 3 % 2 != 0: the height grows 2 -> 4, a pad of 2 > 1
    with pytest.raises(ValueError, match="clip_limit"):
        P.clahe(u8, clip_limit=float("nan"))
    with pytest.raises(ValueError, match="clip_limit"):
        P.clahe(u8, clip_limit="2")
    for fn in (P.rescale_intensity_u8, P.prepare_mscmrseg_slices):
        for bad in (torch.zeros((2, 8, 8), dtype=torch.float64), torch.zeros((2, 8, 8), dtype=torch.int32), np.zeros((2, 8, 8), np.float32)):
            with pytest.raises(TypeError, match="float32 / int16 / uint8"):
                fn(bad)
        with pytest.raises(ValueError, match="dimensions"):
            fn(torch.zeros((8, 8)))
    for fn in (P.resize_volume, P.crop_volume):
        with pytest.raises(TypeError, match="uint8"):
            fn(torch.zeros((2, 8, 8)))
    with pytest.raises(ValueError, match="1x1"):
        P.resize_volume(u8, w=0, h=4)
    with pytest.raises(ValueError, match="leaves"):
        P.crop_volume(u8, crop_size=9)
    with pytest.raises(ValueError, match="crop_size"):
        P.crop_volume(u8, crop_size=0)
    with pytest.raises(ValueError, match="leaves"):
        P.prepare_mscmrseg_slices(torch.zeros((2, 8, 8)), size=16, crop_size=20)
    with pytest.raises(ValueError, match="to_float=False"):
        P.prepare_mscmrseg_slices(torch.zeros((2, 8, 8)), size=16, crop_size=12, clahe=False)
    with pytest.raises(ValueError, match="reflected border|2x2"):
        P.prepare_mscmrseg_slices(torch.zeros((2, 8, 8)), size=16, crop_size=2)
    # the kernel wrappers have no CPU fallback
    for call in (lambda: P.clahe(u8), lambda: P.preprocess_volume(u8), lambda: P.rescale_intensity_u8(u8), lambda: P.resize_volume(u8),
                 lambda: P.crop_volume(u8, 4), lambda: P.prepare_mscmrseg_slices(torch.zeros((2, 8, 8)), size=16, crop_size=12)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_the_host_checks_equal_the_restatements():
    from pointcloududa_amd.utils import preprocess as P
    for h, w, grid in ((16, 16, (2, 2)), (17, 13, (4, 4)), (3, 16, (4, 4)), (2, 2, (1, 1)), (5, 5, (16, 16)), (9, 40, (16, 8)),
                       (2, 3, (2, 2)), (4, 2, (3, 3))):
        try:
            G.clahe_params(h, w, 2.0, *grid)
            ok = True
        except ValueError:
            ok = False
        if ok:
            assert P._check_grid(h, w, 2.0, grid) == grid
        else:
            with pytest.raises(ValueError):
                P._check_grid(h, w, 2.0, grid)


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_declares_what_the_binding_binds():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p, "double": ctypes.c_double}
    for name, ret in (("pcuda_clahe", "int"), ("pcuda_clahe_workspace_size", "size_t"), ("pcuda_rescale_resize_crop_u8", "int"),
                      ("pcuda_rescale_resize_crop_u8_workspace_size", "size_t")):
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        params = [s.strip() for s in m.group(2).split(",") if s.strip() != "void"]
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in params]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
        assert name in _lib.EXPORTED_SYMBOLS
    m = re.search(r"int pcuda_clahe\(([^;]*)\);", hdr)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "in", "out", "n", "h", "w", "clip_limit", "tiles_x", "tiles_y", "out_mode", "workspace", "workspace_bytes", "s"]
    m = re.search(r"int pcuda_rescale_resize_crop_u8\(([^;]*)\);", hdr)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "in", "in_dtype", "n", "sh", "sw", "resize_h", "resize_w", "crop", "out", "workspace", "workspace_bytes", "s"]
    for define, value in (("PCUDA_CLAHE_U8", 0), ("PCUDA_CLAHE_F32X3", 1), ("PCUDA_PRE_F32", 0), ("PCUDA_PRE_I16", 1),
                          ("PCUDA_PRE_U8", 2), ("PCUDA_PRE_U8_RAW", 3)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % define, hdr).group(1)) == value
    assert "arity with OpenCV / ITK is unpinned" in re.sub(r"[\s*]+", " ", hdr)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "preprocess.hip" in mk and "-ffp-contract=off" in mk
    src = open(os.path.join(CSRC, "preprocess.hip")).read()
    for sym in ('extern "C" int pcuda_clahe(', 'extern "C" size_t pcuda_clahe_workspace_size(',
                'extern "C" int pcuda_rescale_resize_crop_u8(', 'extern "C" size_t pcuda_rescale_resize_crop_u8_workspace_size('):
        assert sym in src, sym


def test_the_docs_state_the_convention_and_the_unpinned_parity():
    for doc in ("README.md", "DESIGN.md"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        assert "arity with OpenCV / ITK is unpinned" in text, doc
        assert "two independent restatements" in text and "tests/golden/preprocess.npz" in text, doc
