"""CPU checks of the native-size evaluation of MS-CMRSeg (csrc/area_resize.hip): the two restatements of
the resize rule against each other and against the committed files, the three anchors that hold for OpenCV by its documentation,
the float32 planes against a float64 evaluation of the same tables, the C declarations against the binding and the exported
symbols, the entry points' argument checks with fake pointers, the wrappers' host-side validation, and the printed table of
evaluate_mscmrseg.evaluate_segmentation against literal strings.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from area_resize_ref import EDGES, G, GOLD, same_bits
from conftest import ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
ENTRIES = ("pcuda_area_resize", "pcuda_reconstruct_resize_argmax")


# ---------------------------------------------------------------------------------------------- the rule
def test_the_two_restatements_agree_and_equal_the_committed_files():
    data = G.build()                     # (raises SystemExit where the vectorised and the looped restatement differ)
    assert sorted(GOLD.files) == sorted(data)
    for k in data:
        if k != "numpy_version":
            assert same_bits(GOLD[k], data[k]), k
    assert sorted(k for k in GOLD.files if k.startswith("out_")) == sorted("out_%dx%d" % s for s in G.SIZES)
    assert G.edges()["cases"] == EDGES["cases"] and sorted(EDGES["cases"]) == ["canvas_480x480", "canvas_511x257"]
    for name in (G.PATH, G.EDGES):
        assert os.path.getsize(name) < 256 * 1024, name


def test_the_cases_reach_both_rules_and_the_unstaged_patch():
    h, w = G.SRC_H, G.SRC_W
    assert [G.is_area(h, w, dh, dw) for dw, dh in G.SIZES] == [False, False, True, True, True, False]
    sw, sh, dw, dh = G.TALL
    # the source patch of its one tile, rows x columns, is above the 4096 texels the kernel stages
    assert not G.is_area(sh, sw, dh, dw) and ((dh - 1) * sh // dh + 2) * ((dw - 1) * sw // dw + 2) > 4096
    # the fractional shrink holds leading, full and trailing taps; the enlargement holds single taps (fx == 0) and pairs
    n = G.table_vec(w, 17, True)[2]
    assert n.min() >= 2 and n.max() == 3
    n = G.table_vec(w, 45, False)[2]
    assert sorted(set(n.tolist())) == [1, 2]
    src = G.source_planes()
    assert np.signbit(src[0, 5, 5]) and src[0, 5, 5] == 0 and 0 < src[1, -1, -1] < np.finfo(np.float32).tiny


@pytest.mark.parametrize("fn", (G.resize_vec, G.resize_loops), ids=("vec", "loops"))
def test_the_three_anchors(fn):
    src = G.source_planes()[0]
    h, w = src.shape
    assert same_bits(fn(src, h, w), src), "equal sizes return the input's bits (the signed zeros and the subnormal included)"
    for k in (2, 3):
        assert same_bits(fn(src, k * h, k * w), np.repeat(np.repeat(src, k, axis=0), k, axis=1)), "x%d is pixel replication" % k
    assert same_bits(fn(src, 2 * h, w), np.repeat(src, 2, axis=0)), "one axis enlarged, one equal: the two-tap rule, still a copy"
    ints = np.random.default_rng(2).integers(-30, 31, (16, 24)).astype(np.float32)
    for k in (2, 4):
        # rows in order, each reduced over its k taps in order: exact for small integers, as is the float32 weight 1 / k
        block = ints.astype(np.float64).reshape(16 // k, k, 24 // k, k).sum(axis=(1, 3)) / (k * k)
        assert np.float32(1.0 / k) == 1.0 / k and same_bits(fn(ints, 16 // k, 24 // k), block.astype(np.float32)), k


def test_float32_planes_lie_within_one_rounding_per_operation_of_float64():
    """every product and every sum rounds once: (taps + 2) * 2^-24 * max|src|, taps = the most horizontal plus the most vertical
    taps of an output pixel (the weights of an axis sum to 1 within a rounding each, which the + 2 covers)"""
    rng = np.random.default_rng(4)
    for sh, sw, dh, dw in ((20, 24, 37, 45), (20, 24, 13, 17), (20, 24, 10, 12), (20, 24, 13, 45), (37, 41, 6, 5), (64, 64, 120, 128)):
        src = (rng.standard_normal((sh, sw)) * 5.0).astype(np.float32)
        got, ref = G.resize_vec(src, dh, dw), G.resize_vec(src, dh, dw, np.float64)
        assert got.dtype == np.float32 and ref.dtype == np.float64
        bound = (G.max_taps(sh, sw, dh, dw) + 2) * 2.0 ** -24 * float(np.abs(src).max())
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print("%dx%d -> %dx%d: error %.3g, bound %.3g" % (sh, sw, dh, dw, err, bound))
        assert err <= bound, (sh, sw, dh, dw, err, bound)


def test_argmax_rule_and_reconstruct():
    planes = np.zeros((1, 3, 1, 4), np.float32)
    planes[0, :, 0, 0] = (1, 2, 2)              # the first of two maxima
    planes[0, :, 0, 1] = (5, np.nan, 9)         # a NaN anywhere: 0
    planes[0, :, 0, 2] = (-1, -1, -0.5)
    assert G.argmax_rule(planes).tolist() == [[[1, 0, 2, 0]]]
    canvas = G.reconstruct(np.ones((1, 2, 4, 4), np.float32), 2, 7)
    assert canvas.shape == (1, 2, 7, 7) and canvas.sum() == 32 and canvas[0, 0, 1:5, 1:5].all() and not canvas[0, 0, 0].any()


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_binding_and_exported_symbols_agree():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "pcuda_stream_t": ctypes.c_void_p, "long long": ctypes.c_longlong}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == "int", name
        params = [re.sub(r"\s+", " ", s).strip() for s in m.group(2).split(",")]
        want = [ctypes.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0]] for a in params]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and list(args) == want, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert int(re.search(r"#define\s+PCUDA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _lib.PCUDA_ABI_VERSION == _lib.lib().pcuda_version()
    assert "area_resize.hip" in open(os.path.join(CSRC, "Makefile")).read()
    src = open(os.path.join(CSRC, "area_resize.hip")).read()
    for entry in ENTRIES:
        assert 'extern "C" int %s(' % entry in src, entry


def test_bad_arguments_are_rejected_without_a_gpu():
    """fake pointers: every call below must return before any launch"""
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    IN, OUT = 0x10000, 0x20000

    def resize(inp=IN, sn=480, sr=24, n=2, sh=20, sw=24, out=OUT, dh=37, dw=45):
        return lib.pcuda_area_resize(inp, sn, sr, n, sh, sw, out, dh, dw, None)

    def fused(inp=IN, sn=4 * 144, sc=144, sr=12, n=2, c=4, h=12, w=12, crop=6, origin=16, out=OUT, dh=29, dw=23):
        return lib.pcuda_reconstruct_resize_argmax(inp, sn, sc, sr, n, c, h, w, crop, origin, out, dh, dw, None)

    for kw in (dict(inp=None), dict(out=None), dict(out=IN), dict(sh=0), dict(sw=-1), dict(dh=0), dict(dw=0), dict(dw=16385), dict(sh=16385),
               dict(n=-1), dict(n=65536), dict(sr=23), dict(sn=-480), dict(sn=0)):
        assert resize(**kw) == -1 and lib.pcuda_last_error().startswith(b"area_resize"), (kw, lib.pcuda_last_error())
    assert resize(n=0) == 0
    for kw in (dict(inp=None), dict(out=None), dict(c=9), dict(c=0), dict(crop=9), dict(crop=0), dict(origin=10), dict(h=10), dict(w=14),
               dict(h=14, w=14), dict(dh=0), dict(dw=16385), dict(origin=0), dict(n=-1), dict(n=65536), dict(sr=11), dict(sc=0),
               dict(sn=0), dict(sc=-144)):
        assert fused(**kw) == -1 and lib.pcuda_last_error().startswith(b"reconstruct_resize_argmax"), (kw, lib.pcuda_last_error())
    assert fused(n=0) == 0
    # an odd canvas: the window is int(origin / 2) +- crop, as the reference slices it
    assert fused(origin=13, n=0) == 0 and fused(origin=12, n=0) == 0 and fused(origin=11, n=0) == -1


# ---------------------------------------------------------------------------------------------- the host side of the package
def test_argument_validation_raises_before_touching_the_device():
    import torch
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd import validate as V
    from pointcloududa_amd.utils import utils as U
    x = torch.zeros((2, 20, 24))
    for h, w in ((0, 4), (4, 16385), (4.0, 4), (True, 4)):
        with pytest.raises(ValueError, match="output size"):
            K.area_resize(x, h, w)
        with pytest.raises(ValueError, match="output size"):
            K.reconstruct_resize_argmax(torch.zeros((1, 4, 12, 12)), h, w, 6, 16)
    with pytest.raises(ValueError, match="planes"):
        K.area_resize(torch.zeros((1, 2, 20, 24)), 4, 4)
    for shape, crop, origin, what in (((1, 9, 12, 12), 6, 16, "1..8 classes"), ((1, 4, 12, 12), 9, 16, "does not fit"),
                                      ((1, 4, 10, 12), 6, 16, "the window is 12x12"), ((1, 4, 12, 12), 6, 11, "does not fit")):
        with pytest.raises(ValueError, match=what):
            K.reconstruct_resize_argmax(torch.zeros(shape), 4, 4, crop, origin)
    # no CPU fallback
    for call in (lambda: K.area_resize(x, 4, 4), lambda: K.reconstruct_resize_argmax(torch.zeros((1, 4, 12, 12)), 4, 4, 6, 16),
                 lambda: U.resize_volume(x, 4, 4), lambda: EM.reconstuct_volume(torch.zeros((1, 12, 12, 4)), 6, 16),
                 lambda: EM.read_volume(torch.zeros((2, 16, 16, 3), dtype=torch.uint8), 12)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(TypeError, match="float32 planes"):
        U.resize_volume(np.zeros((2, 20, 24), np.float64))
    with pytest.raises(TypeError, match="uint8"):
        EM.read_volume(np.zeros((2, 16, 16, 3), np.float32))
    with pytest.raises(TypeError, match="float32"):
        EM.reconstuct_volume(torch.zeros((1, 12, 12, 4), dtype=torch.float64))
    for bad in ((320,), (320, 0), (320.5, 288), (True, 4)):
        with pytest.raises(ValueError, match="native_shape"):
            V._native_size("evaluate_volume", bad, "mscmrseg")
    with pytest.raises(ValueError, match="variant='mscmrseg'"):
        V._native_size("evaluate_volume", (320, 288), "mmwhs")
    assert V._native_size("evaluate_volume", (320, 288), "mscmrseg") == (288, 320) and V._native_size("e", None, "mmwhs") is None


# ---------------------------------------------------------------------------------------------- the table
RES = [[0.9, 2.0, 0.5, 0.8, 3.0, 1.0, 0.7, 4.0, 1.5],
       [0.5, 4.0, 1.5, -1, -1, -1, 0.3, 2.0, 0.5],              # a patient whose RV is empty on one side: the -1 triplet
       [0.4, 4.5, 1.0, 0.6, 5.0, 2.0, 0.2, 3.0, 2.5]]


def test_the_printed_table_character_for_character(capsys):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    t = EM.summary_table(RES)
    assert list(t["DC"]) == ["endo", "rv", "myo"] and set(t) == {"DC", "HD", "ASD", "Ave"}
    # by hand: the -1 stays in RV's Dice list ((0.8 - 1 + 0.6) / 3) and leaves its HD and ASD lists ((3 + 5) / 2, (1 + 2) / 2)
    assert t["DC"]["rv"] == (0.133, 0.806) and t["HD"]["rv"] == (4.0, 1.0) and t["ASD"]["rv"] == (1.5, 0.5)
    EM.print_table(t)
    assert capsys.readouterr().out.splitlines() == [
        "Ave endo DC: 0.6, 0.216, Ave rv DC: 0.133, 0.806, Ave myo DC: 0.4, 0.216",
        "Ave Dice: 0.378, 0.413",
        "Ave endo HD: 3.5, 1.08, Ave rv HD: 4.0, 1.0, Ave myo HD: 3.0, 0.816",
        "Ave HD: 3.500, 0.965",
        "Ave endo ASD: 1.0, 0.408, Ave rv ASD: 1.5, 0.5, Ave myo ASD: 1.5, 0.816",
        "Ave ASD: 1.333, 0.575",
        "0.4, 0.216, 0.6, 0.216, 0.133, 0.806",                 # the closing lines: myo, endo, rv
        "3.0, 0.816, 3.5, 1.08, 4.0, 1.0",
        "1.5, 0.816, 1.0, 0.408, 1.5, 0.5"]
    EM.print_table(EM.summary_table(RES, ifhd=False))
    assert capsys.readouterr().out.splitlines() == [
        "Ave endo DC: 0.6, 0.216, Ave rv DC: 0.133, 0.806, Ave myo DC: 0.4, 0.216",
        "Ave Dice: 0.378, 0.413",
        "Ave endo ASD: 1.0, 0.408, Ave rv ASD: 1.5, 0.5, Ave myo ASD: 1.5, 0.816",
        "Ave ASD: 1.333, 0.575",
        "0.4, 0.216, 0.6, 0.216, 0.133, 0.806",
        "1.5, 0.816, 1.0, 0.408, 1.5, 0.5"]
    EM.print_table(EM.summary_table(RES, ifhd=False, ifasd=False))
    assert len(capsys.readouterr().out.splitlines()) == 3
    EM.print_table(EM.summary_table([]))
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Ave endo DC: nan, nan, Ave rv DC: nan, nan, Ave myo DC: nan, nan" and lines[1] == "Ave Dice: nan, nan"
    assert lines[3] == "Ave HD: nan, nan" and lines[5] == "Ave ASD: nan, nan" and lines[6:] == ["nan, nan, nan, nan, nan, nan"] * 3
    # the extended lists hold five values per class; the table and the rows read the first three
    ext = [[v for k in range(3) for v in r[3 * k:3 * k + 3] + [9.0, 9.0]] for r in RES]
    assert EM.summary_table(ext, extended=True) == t
    assert EM.save_rows(ext[1], "m", 7, extended=True) == EM.save_rows(RES[1], "m", 7) == [
        [0.5, 4.0, 1.5, "lv", "m", 7], [-1, -1, -1, "rv", "m", 7], [0.3, 2.0, 0.5, "myo", "m", 7]]
    assert EM.SAVE_COLUMNS == ["DSC", "HD", "ASD", "cat", "model", "pad_id"]


def test_an_empty_set_of_patients_needs_no_device(capsys):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    out = EM.evaluate_segmentation(None, [], toprint=True)
    assert out["per_patient"] == {} and out["rows"] == [] and np.isnan(out["table"]["Ave"]["DC"][0])
    assert capsys.readouterr().out.splitlines()[1] == "Ave Dice: nan, nan"


# ---------------------------------------------------------------------------------------------- documents
def test_the_docs_name_the_new_entries_and_say_that_opencv_parity_is_unpinned():
    for doc in ("README.md", "DESIGN.md"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        assert "pcuda_reconstruct_resize_argmax" in text and "pcuda_area_resize" in text and "reconstuct_volume" in text, doc
        assert "parity with OpenCV" in text and "not pinned" in text, doc
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert "pcuda_reconstruct_resize_argmax" in text and "pcuda_area_resize" in text
    design = re.sub(r"\s+", " ", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert "f15" in design and "profiles/area_resize_bench.json" in design and "native_shape" in design
    for name in ("pointcloududa_amd/utils/volume.py", "pointcloududa_amd/evaluate_mscmrseg.py"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, name)).read())
        assert "cv2 resize, pandas) is not part" not in text and "the cv2 ``INTER_AREA`` resize and ``reconstuct_volume`` of the" not in text, name
