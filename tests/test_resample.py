"""CPU checks of the device-side spacing resample (pointcloududa_amd/utils/resample.py, csrc/resample.hip; DESIGN.md section 6,
f12): the committed fixture (outputs of scipy.ndimage.zoom / numpy themselves next to the plain restatement of
scripts/make_resample_golden.py), the reference's shape arithmetic, the C declarations against the binding, the entry points'
argument checks with fake pointers, and the host-side validation.  No GPU."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLD, ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
GEN = os.path.join(ROOT, "scripts", "make_resample_golden.py")
_spec = importlib.util.spec_from_file_location("make_resample_golden", GEN)
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
FILE = np.load(os.path.join(GOLD, "resample.npz"))
ZOOM, LABELS, STATS = G.load_cases(FILE)
ENTRIES = ("pcuda_zoom_linear_crop", "pcuda_zoom_standardize", "pcuda_zoom_labels")


def _have_scipy():
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except ImportError:
        return False


# ---------------------------------------------------------------------------------------------- the fixture
def test_the_restatement_arrays_equal_the_scipy_arrays_bit_for_bit():
    assert len(ZOOM) == 30 and len(LABELS) == 6 and len(STATS) == 6
    for c in ZOOM:
        assert G.bit_equal(c["rule"], c["scipy"]) and c["scipy"].dtype == c["vol"].dtype, c["name"]
        assert G.bit_equal(G.zoom_rule(c["vol"], c["zh"], c["zw"], c["crop"]), c["scipy"]), c["name"]
    for c in LABELS:
        assert G.bit_equal(c["rule"], c["scipy"]) and c["scipy"].dtype == np.uint8, c["name"]
        lab, stray = G.label_rule(c["raw"], c["zh"], c["zw"], c["num_classes"], c["remap"], c["crop"])
        assert G.bit_equal(lab, c["scipy"]) and stray == 0, c["name"]
    assert str(FILE["scipy_version"]) and str(FILE["numpy_version"])
    assert os.path.getsize(os.path.join(GOLD, "resample.npz")) < 1000 * 1000


def test_the_fixture_holds_the_cases_it_is_there_for():
    names = {c["name"]: c for c in ZOOM}
    for tag, dt in G.DTYPES:
        for stem, src, dst in (("20x24_to_21x25", (20, 24), (21, 25)), ("20x24_to_13x9", (20, 24), (13, 9)), ("7x5_to_16x3", (7, 5), (16, 3)),
                               ("5x6_identity", (5, 6), (5, 6)), ("9x9_to_1x4", (9, 9), (1, 4)), ("37x41_to_50x33_crop24", (37, 41), (24, 24)),
                               ("256x256_to_267x267_crop224", (256, 256), (224, 224))):
            c = names["%s_%s" % (tag, stem)]
            assert c["vol"].dtype == dt and c["vol"].shape[1:] == src and c["scipy"].shape[1:] == dst, c["name"]
        assert names["%s_256x256_to_267x267_crop224" % tag]["vol"].shape[0] == 2
        assert np.array_equal(names["%s_5x6_identity" % tag]["scipy"], names["%s_5x6_identity" % tag]["vol"])
        a, b = names["%s_37x41_to_50x33_crop24" % tag], names["%s_37x41_to_50x33" % tag]
        assert np.array_equal(a["scipy"][0], b["scipy"][0, 13:37, 4:28]), "crop_volume: rows 25 - 12 .. 25 + 12, columns 16 - 12 .. 16 + 12"
    assert names["i16_20x24_to_21x25"]["vol"].min() < 0 and names["f32_20x24_to_21x25"]["vol"].min() < 0
    # the overshooting pair: double(out - 1) ((in - 1) / (out - 1)) > in - 1; scipy's last row / column is cval = 0 there
    i, o = (int(v) for v in FILE["overshoot_pair"])
    assert float(o - 1) * ((i - 1) / (o - 1)) > i - 1 and (i, o) == G.overshoot_pairs(64)[0] and int(FILE["overshoot_pairs_up_to_512"]) > 0
    for tag, _ in G.DTYPES:
        r, c = names["%s_overshoot_rows_%dx5_to_%dx7" % (tag, i, o)], names["%s_overshoot_cols_5x%d_to_6x%d" % (tag, i, o)]
        assert r["vol"].min() > 0 and not r["scipy"][:, -1, :].any() and r["scipy"][:, -2, :].all()
        assert c["vol"].min() > 0 and not c["scipy"][:, :, -1].any() and c["scipy"][:, :, -2].all()
    by = {c["name"]: c for c in LABELS}
    for size in ("25x29", "31x37", "17x19"):
        c = by["i16_discs_to_%s" % size]
        assert sorted(np.unique(c["raw"]).tolist()) == [0, 200, 500, 600] and c["raw"].dtype == np.int16
        differ, none, two = (int(v) for v in c["counts"])
        assert differ >= 10 and two >= 1 and (none >= 1 or size == "17x19"), c["name"]
    assert by["u8_discs5_to_31x37"]["num_classes"] == 5 and by["u8_discs5_to_31x37"]["raw"].dtype == np.uint8
    assert by["u8_discs5_to_31x37"]["remap"] == () and by["i16_discs_to_25x29"]["remap"] == G.REMAP
    sby = {c["name"]: c for c in STATS}
    assert sby["i16_constant"]["rule_stats"][1] == 0.0 and np.isnan(sby["i16_constant"]["rule"]).all(), "0 / 0 as numpy gives it"
    for c in STATS:
        if c["vol"].dtype != np.float32:
            assert c["rule_stats"][0] == c["numpy_stats"][0], "the integer mean equals numpy.mean: %s" % c["name"]
        n = c["rule"].size
        assert abs(c["rule_stats"][1] - c["numpy_stats"][1]) <= n * 2.0 ** -53 * c["numpy_stats"][1], c["name"]
        assert np.count_nonzero(c["rule"].view(np.uint32) != c["numpy"].view(np.uint32)) * 100 <= n, c["name"]
    assert sby["f32_exact_sums_37x41_to_50x33_crop24"]["rule_stats"][0] == sby["f32_exact_sums_37x41_to_50x33_crop24"]["numpy_stats"][0]


@pytest.mark.skipif(not _have_scipy(), reason="scipy is not installed")
def test_scipy_reproduces_the_stored_outputs():
    for c in ZOOM:
        assert G.bit_equal(G.zoom_scipy(c["vol"], c["zh"], c["zw"], c["crop"]), c["scipy"]), c["name"]
    for c in LABELS:
        assert G.bit_equal(G.labels_scipy(c["raw"], c["zh"], c["zw"], c["num_classes"], c["remap"], c["crop"])[0], c["scipy"]), c["name"]
    for c in STATS:
        z = G.zoom_scipy(c["vol"], c["zh"], c["zw"], c["crop"])
        d = z if z.dtype != np.float32 else z.astype(np.float64)
        assert (float(np.mean(d)), float(np.std(d))) == tuple(c["numpy_stats"].tolist()), c["name"]


@pytest.mark.skipif(not _have_scipy(), reason="scipy is not installed")
def test_the_fixture_regenerates_exactly():
    assert G.check_file() == len(FILE.files) - 2


def test_the_exact_integer_statistics_follow_the_stated_arithmetic():
    x = np.array([[-3, 5, 7, 7]], np.int16)
    n, s1, s2 = 4, 16, 9 + 25 + 49 + 49
    assert G.int_stats(x) == (s1 / n, math.sqrt(float(n * s2 - s1 * s1) / (float(n) * float(n))))
    assert G.int_stats(x)[0] == float(np.mean(x)) and abs(G.int_stats(x)[1] - float(np.std(x))) <= 4 * 2.0 ** -53 * float(np.std(x))
    assert G.int_stats(np.full((3, 3), 9, np.uint8)) == (9.0, 0.0)


# ---------------------------------------------------------------------------------------------- the reference's shape arithmetic
def test_output_shape_and_factors_reproduce_the_reference():
    from pointcloududa_amd.utils import resample as R
    fy, fx = R.spacing_zoom_factors((256, 256), (1.25, 1.25))
    assert (fy, fx) == (267.0 / 256.0, 267.0 / 256.0) and R.zoom_output_shape((256, 256), (fy, fx)) == (267, 267)
    # the reference's own lines
    spacing, shape, new = np.array([1.25, 1.25, 12.0]), (256, 256, 8), (1.2, 1.2, 5.0)
    real = np.round(shape * (spacing / new)) / shape
    assert (fy, fx) == (float(real[0]), float(real[1]))
    assert R.spacing_zoom_factors((480, 512), (0.729, 0.75), (1.2, 1.2)) == (292.0 / 480.0, 320.0 / 512.0)
    for shape_hw, zoom in (((20, 24), (21 / 20, 25 / 24)), ((7, 5), (16 / 7, 3 / 5)), ((9, 9), (1 / 9, 4 / 9)), ((5, 5), (0.5, 0.3)), ((5, 3), (0.5, 0.5))):
        assert R.zoom_output_shape(shape_hw, zoom) == G.zoom_output_shape(shape_hw, zoom) == tuple(int(round(d * f)) for d, f in zip(shape_hw, zoom))
    assert R.zoom_output_shape((5, 3), (0.5, 0.5)) == (2, 2), "round half to even, as Python's round in scipy's zoom"
    if _have_scipy():
        from scipy import ndimage
        for shape_hw, zoom in (((20, 24), (21 / 20, 25 / 24)), ((7, 5), (16 / 7, 3 / 5)), ((5, 3), (0.5, 0.5))):
            assert ndimage.zoom(np.zeros((1,) + shape_hw), [1, zoom[0], zoom[1]], order=1).shape[1:] == R.zoom_output_shape(shape_hw, zoom)
    for bad in ((0.0, 1.0), (1.0, -2.0), (float("nan"), 1.0), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="zoom factors"):
            R.zoom_output_shape((8, 8), bad)
    with pytest.raises(TypeError, match="shape_hw"):
        R.zoom_output_shape((8, 8), 1.5)
    with pytest.raises(ValueError, match="spacing"):
        R.spacing_zoom_factors((256, 256), (1.25, 0.0))
    with pytest.raises(ValueError, match="two in-plane"):
        R.spacing_zoom_factors((256, 256, 8), (1.25, 1.25, 12.0))


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_declares_what_the_binding_binds():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p, "double": ctypes.c_double}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for entry in ENTRIES:
        for name, ret in ((entry, "int"), (entry + "_workspace_size", "size_t")):
            m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
            assert m and m.group(1) == ret, name
            params = [s.strip() for s in m.group(2).split(",") if s.strip() != "void"]
            want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in params]
            res, args = _lib._PROTOS[name]
            assert res is kinds[ret] and list(args) == want, name
            assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert int(re.search(r"#define\s+PCUDA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _lib.PCUDA_ABI_VERSION == _lib.lib().pcuda_version()
    flat = re.sub(r"[\s*]+", " ", hdr)
    assert "THIS BUILD'S OWN convention" in flat and "numpy's float32 pairwise accumulation of a float32 array is not reproduced" in flat
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "resample.hip" in mk and "-ffp-contract=off" in mk
    src = open(os.path.join(CSRC, "resample.hip")).read()
    for entry in ENTRIES:
        assert 'extern "C" int %s(' % entry in src and 'extern "C" size_t %s_workspace_size(' % entry in src, entry
    assert "resample" not in open(os.path.join(CSRC, "preprocess.hip")).read()


def test_workspace_sizes_are_positive_and_aligned():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    for zh, zw, crop in ((267, 267, 224), (1, 4, 0), (16, 3, 0), (50, 33, 24), (32768, 32768, 0)):
        sizes = [lib.pcuda_zoom_linear_crop_workspace_size(zh, zw, crop), lib.pcuda_zoom_labels_workspace_size(zh, zw, crop)]
        if zh < 32768:
            sizes += [lib.pcuda_zoom_standardize_workspace_size(dt, 3, zh, zw, crop) for dt in (0, 1, 2)]
        assert all(s > 0 and s % 16 == 0 for s in sizes), (zh, zw, crop, sizes)
    oh = 224
    table = (oh + oh) * 12
    assert lib.pcuda_zoom_linear_crop_workspace_size(267, 267, 224) == table and lib.pcuda_zoom_labels_workspace_size(267, 267, 224) == 16 + table
    assert lib.pcuda_zoom_standardize_workspace_size(1, 16, 267, 267, 224) == table + 1024 * 16 + 16 * oh * oh * 2
    for bad in ((0, 8, 0), (8, 0, 0), (8, 8, -1), (8, 8, 10), (8, 8, 1), (32769, 8, 0)):
        assert lib.pcuda_zoom_linear_crop_workspace_size(*bad) == 0 and lib.pcuda_zoom_labels_workspace_size(*bad) == 0, bad
        assert lib.pcuda_zoom_standardize_workspace_size(1, 2, *bad) == 0, bad
    assert lib.pcuda_zoom_standardize_workspace_size(3, 2, 8, 8, 0) == 0 and lib.pcuda_zoom_standardize_workspace_size(1, 0, 8, 8, 0) == 0


def test_bad_arguments_are_rejected_without_a_gpu():
    """fake pointers: every call below must return before any launch"""
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    IN, OUT, WS, ST = 0x10000, 0x20000, 0x30000, 0x40000
    remap = (ctypes.c_int * 6)(200, 1, 500, 2, 600, 3)

    def zoom(inp=IN, dt=1, n=2, sh=8, sw=8, zh=10, zw=10, crop=0, out=OUT, ws=WS, nbytes=1 << 20):
        return lib.pcuda_zoom_linear_crop(inp, dt, n, sh, sw, zh, zw, crop, out, ws, nbytes, None)

    def std(inp=IN, dt=1, n=2, sh=8, sw=8, zh=10, zw=10, crop=0, ch=3, out=OUT, st=ST, ws=WS, nbytes=1 << 20):
        return lib.pcuda_zoom_standardize(inp, dt, n, sh, sw, zh, zw, crop, ch, out, st, ws, nbytes, None)

    def lab(inp=IN, dt=1, n=2, sh=8, sw=8, zh=10, zw=10, crop=0, ncls=4, rm=ctypes.cast(remap, ctypes.c_void_p), nrm=3, out=OUT, ws=WS, nbytes=1 << 20):
        return lib.pcuda_zoom_labels(inp, dt, n, sh, sw, zh, zw, crop, ncls, rm, nrm, out, ws, nbytes, None)

    geometry = (dict(zh=0), dict(zw=0), dict(zh=-3), dict(sh=0), dict(sw=0), dict(n=-1), dict(crop=-2), dict(crop=12), dict(crop=1),
                dict(sh=32769), dict(zw=32769), dict(dt=3), dict(dt=-1), dict(inp=None), dict(out=None), dict(out=IN),
                dict(n=40000, zh=32768, zw=32768))
    for call, tag in ((zoom, b"zoom_linear_crop"), (std, b"zoom_standardize"), (lab, b"zoom_labels")):
        for kw in geometry:
            assert call(**kw) == -1 and lib.pcuda_last_error().startswith(tag), (tag, kw, lib.pcuda_last_error())
        assert call(n=0, inp=None, out=None, ws=None, nbytes=0) == 0, "an empty volume is a no-op"
        for kw in (dict(ws=None), dict(nbytes=8), dict(ws=WS + 4)):
            assert call(**kw) == -4 and lib.pcuda_last_error().startswith(tag), (tag, kw)
    assert zoom(out=IN) == -1 and b"in == out" in lib.pcuda_last_error()
    for kw in (dict(ch=2), dict(ch=0), dict(st=None), dict(st=ST + 4)):
        assert std(**kw) == -1 and lib.pcuda_last_error().startswith(b"zoom_standardize"), kw
    for kw in (dict(dt=0), dict(ncls=1), dict(ncls=9), dict(nrm=9), dict(nrm=-1), dict(rm=None)):
        assert lab(**kw) == -1 and lib.pcuda_last_error().startswith(b"zoom_labels"), kw
    need = lib.pcuda_zoom_standardize_workspace_size(1, 2, 10, 10, 0)
    assert std(nbytes=need - 1) == -4


# ---------------------------------------------------------------------------------------------- the host side of the package
def test_argument_validation_raises_before_touching_the_device():
    import torch
    from pointcloududa_amd.utils import resample as R
    v = torch.zeros((2, 16, 16), dtype=torch.int16)
    calls = ((R.zoom_linear, "float32 / int16 / uint8"), (R.standardize_zoomed, "float32 / int16 / uint8"), (R.zoom_labels, "int16 / uint8"),
             (lambda x, z, **kw: R.prepare_mscmrseg_npy(x, (1.25, 1.25), **kw), "float32 / int16 / uint8"),
             (lambda x, z, **kw: R.prepare_mscmrseg_npy_labels(x, (1.25, 1.25), **kw), "int16 / uint8"))
    for fn, dtypes in calls:
        for bad in (torch.zeros((2, 16, 16), dtype=torch.float64), torch.zeros((2, 16, 16), dtype=torch.int32), np.zeros((2, 16, 16), np.int16)):
            with pytest.raises(TypeError, match=dtypes):
                fn(bad, (1.0, 1.0))
        for bad in (torch.zeros((16, 16), dtype=torch.int16), torch.zeros((1, 2, 16, 16), dtype=torch.int16)):
            with pytest.raises(ValueError, match="dimensions"):
                fn(bad, (1.0, 1.0))
        with pytest.raises(ValueError, match="leaves"):
            fn(v, (1.0, 1.0), crop_size=18)
    with pytest.raises(TypeError, match="int16 / uint8"):
        R.zoom_labels(torch.zeros((2, 16, 16)), (1.0, 1.0))
    with pytest.raises(ValueError, match="leaves"):
        R.zoom_linear(v, (1.0, 1.0), crop_size=1)
    with pytest.raises(ValueError, match="leaves"):
        R.zoom_linear(v, (1.0, 0.5), crop_size=12)
    with pytest.raises(ValueError, match="zoomed slice has sides"):
        R.zoom_linear(v, (0.01, 1.0))
    with pytest.raises(ValueError, match="zoom factors"):
        R.zoom_linear(v, (0.0, 1.0))
    with pytest.raises(ValueError, match="channels"):
        R.standardize_zoomed(v, (1.0, 1.0), crop_size=8, channels=2)
    for ncls in (1, 9, 4.0, True):
        with pytest.raises(ValueError, match="classes"):
            R.zoom_labels(v, (1.0, 1.0), num_classes=ncls, crop_size=8)
    with pytest.raises(ValueError, match="at most 8"):
        R.zoom_labels(v, (1.0, 1.0), remap=tuple((k, 1) for k in range(9)), crop_size=8)
    with pytest.raises(TypeError, match="pairs"):
        R.zoom_labels(v, (1.0, 1.0), remap=(200, 1), crop_size=8)
    # the kernel wrappers have no CPU fallback
    for call in (lambda: R.zoom_linear(v, (1.0, 1.0)), lambda: R.standardize_zoomed(v, (1.0, 1.0), crop_size=8),
                 lambda: R.zoom_labels(v, (1.0, 1.0), crop_size=8), lambda: R.prepare_mscmrseg_npy(v, (1.25, 1.25), crop_size=8),
                 lambda: R.prepare_mscmrseg_npy_labels(v, (1.25, 1.25), crop_size=8)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_the_docs_name_the_resample_and_what_is_not_built():
    for doc in ("README.md", "DESIGN.md"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        assert "tests/golden/resample.npz" in text and "pcuda_zoom_standardize" in text, doc
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "pointcloududa_amd", "utils", "preprocess.py")).read())
    assert "utils/resample.py" in text
