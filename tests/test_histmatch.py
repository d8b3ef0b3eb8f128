"""CPU checks of the device-side histogram matching (pointcloududa_amd/utils/histmatch.py, csrc/histmatch.hip; DESIGN.md
section 6, f10): the two plain-numpy restatements of skimage's match_histograms against each other (bit for bit, in float64
and after the cast), the fixture regenerating exactly, its case set, ``reference_tables`` against np.unique / np.cumsum, the
host-side validation, and the C declaration against the binding.  No GPU and no library load."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
GEN = os.path.join(ROOT, "scripts", "make_match_hist_golden.py")


def _helper():
    sys.path.insert(0, os.path.dirname(GEN))
    try:
        spec = importlib.util.spec_from_file_location("make_match_hist_golden", GEN)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(os.path.dirname(GEN))
    return m


G = _helper()
CASES = G.load_cases(np.load(os.path.join(GOLD, "match_hist.npz")))


# ---------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_two_restatements_agree_bit_for_bit_on_every_fixture_case(case):
    """np.unique / np.interp against np.sort / np.searchsorted / explicit arithmetic: equal in float64 and after the cast, and
    equal to the stored expectation"""
    img, ref = case["images"], case["reference"]
    a64, b64 = G.match_unique64(img, ref), G.match_sorted64(img, ref)
    assert a64.dtype == np.float64 and G.bit_equal(a64, b64)
    a, b = G.cast(a64, img.dtype), G.cast(b64, img.dtype)
    assert G.bit_equal(a, b) and G.bit_equal(a, case["expected"])
    assert case["expected"].dtype == img.dtype and case["expected"].shape == img.shape


def test_the_restatements_agree_at_the_workload_sizes():
    """one 256x256x3 fp32 sample and one 512x512x1 plane (not stored: the fixture stays small)"""
    for shape, rshape, seed in (((1, 256, 256, 3), (256, 256, 3), 30), ((1, 512, 512, 1), (300, 200, 1), 32)):
        img, ref = G.normal_f32(shape, seed, 100.0, 300.0), G.normal_f32(rshape, seed + 1, 0.0, 1.0)
        a64, b64 = G.match_unique64(img, ref), G.match_sorted64(img, ref)
        assert G.bit_equal(a64, b64) and G.bit_equal(G.cast(a64, np.float32), G.cast(b64, np.float32))


def test_the_fixture_regenerates_exactly_and_is_small():
    assert G.check_file() == 4 * len(CASES)
    assert os.path.getsize(os.path.join(GOLD, "match_hist.npz")) < 1000 * 1000


def test_fixture_case_set():
    """fp32: B = 3 with M != N, the key-coverage plane (both signs, 1e-30 .. 1e30, subnormals, both zeros, +-inf, every key byte
    varying), 37-level ties, a constant plane, tiny and ragged planes; uint8: 64x64x3, 33x47x1, a constant plane"""
    by = {c["name"]: c for c in CASES}
    assert len(by) == len(CASES) == 12
    c = by["f32_normal_b3_64x64x3"]
    assert c["images"].shape == (3, 64, 64, 3) and c["reference"].shape == (48, 80, 3) and c["images"].dtype == np.float32
    assert not np.array_equal(c["images"][0], c["images"][1]) and not np.array_equal(c["images"][1], c["images"][2])
    k = by["f32_keys_40x24x2"]["images"]
    assert k.shape == (1, 40, 24, 2) and not np.isnan(k).any()
    fin = k[np.isfinite(k) & (k != 0)]
    assert (k < 0).any() and (k > 0).any() and np.isposinf(k).any() and np.isneginf(k).any()
    assert np.abs(fin).min() < 1.2e-38 and np.abs(fin).max() > 1e30 and ((np.abs(fin) > 1e-30) & (np.abs(fin) < 1e-20)).any()
    zeros = k[k == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    bits = k.view(np.uint32).ravel()
    for shift in (0, 8, 16, 24):
        assert len(np.unique((bits >> shift) & 0xFF)) > 128, shift
    t = by["f32_ties_33x47x3"]["images"]
    assert t.shape == (1, 33, 47, 3) and all(len(np.unique(t[..., ch])) <= 37 for ch in range(3))
    cst = by["f32_constant_16x16x1"]
    assert len(np.unique(cst["images"])) == 1 and np.all(cst["expected"] == cst["reference"].max()), "cnt = N, q = 1: the maximum"
    z = by["f32_zeros_8x8x1"]["images"]
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert {by[n]["images"].shape[1:] for n in ("f32_tiny_1x1x1", "f32_tiny_5x3x1", "f32_ragged_63x65x1")} == {
        (1, 1, 1), (5, 3, 1), (63, 65, 1)}
    for n, shape in (("u8_random_64x64x3", (64, 64, 3)), ("u8_smooth_33x47x1", (33, 47, 1)), ("u8_constant_16x16x3", (16, 16, 3))):
        assert by[n]["images"].dtype == by[n]["reference"].dtype == by[n]["expected"].dtype == np.uint8
        assert by[n]["images"].shape[1:] == shape
    u = by["u8_constant_16x16x3"]
    assert np.all(u["expected"] == u["reference"].reshape(-1, 3).max(axis=0))


def test_the_uint8_cast_truncates_toward_zero():
    assert G.cast(np.array([0.0, 0.999, 1.0, 1.5, 254.9999, 255.0]), np.uint8).tolist() == [0, 0, 1, 1, 254, 255]
    assert G.cast(np.array([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]), np.float32).tolist() == [1.0, 1.0 + 2.0 ** -22]


# ---------------------------------------------------------------------------------------------- the host side of the package
def test_reference_tables_equal_np_unique_and_cumsum():
    from pointcloududa_amd.utils.histmatch import reference_tables
    rng = np.random.default_rng(5)
    ref = np.stack([rng.integers(0, 7, (20, 30)), rng.integers(0, 200, (20, 30)), np.full((20, 30), 9)], axis=-1).astype(np.float32)
    ref[0, 0, 1], ref[0, 1, 1] = 0.0, -0.0
    values, quantiles, lengths = reference_tables(ref)
    assert values.dtype == quantiles.dtype == np.float64 and lengths.dtype == np.int32
    assert values.shape == quantiles.shape == (3, int(lengths.max())) and lengths.shape == (3,)
    for ch in range(3):
        tv, tc = np.unique(ref[..., ch].ravel(), return_counts=True)
        n = len(tv)
        assert lengths[ch] == n
        assert np.array_equal(values[ch, :n], tv.astype(np.float64)) and np.array_equal(quantiles[ch, :n], np.cumsum(tc) / 600)
        assert np.all(values[ch, n:] == tv[-1]) and np.all(quantiles[ch, n:] == 1.0), "padding repeats the last entry"
        assert quantiles[ch, n - 1] == 1.0
    assert lengths[2] == 1 and lengths[0] <= 7 < lengths[1]
    # uint8 references and the fixture's own
    for case in CASES:
        values, quantiles, lengths = reference_tables(case["reference"])
        for ch in range(case["reference"].shape[2]):
            tv, tc = np.unique(case["reference"][..., ch].ravel(), return_counts=True)
            assert lengths[ch] == len(tv) and np.array_equal(values[ch, :len(tv)], tv.astype(np.float64))
            assert np.array_equal(quantiles[ch, :len(tv)], np.cumsum(tc) / (case["reference"].shape[0] * case["reference"].shape[1]))


def test_reference_tables_refuse_what_the_device_cannot_take():
    from pointcloududa_amd.utils.histmatch import reference_tables
    good = np.ones((4, 4, 3), dtype=np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        ref = good.copy()
        ref[1, 2, 0] = bad
        with pytest.raises(ValueError, match="finite"):
            reference_tables(ref)
    with pytest.raises(ValueError, match="empty"):
        reference_tables(np.zeros((0, 4, 3), dtype=np.float32))
    for nd in (np.ones((4, 4), dtype=np.float32), np.ones((2, 4, 4, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match="dimensions"):
            reference_tables(nd)


def test_match_histograms_validates_on_the_host():
    import torch
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import histmatch as H
    assert A.HistReference is H.HistReference and A.match_histograms is H.match_histograms and A.reference_tables is H.reference_tables
    f32 = H.HistReference(np.random.default_rng(0).standard_normal((6, 5, 3)).astype(np.float32), "cpu")
    u8 = H.HistReference(np.random.default_rng(1).integers(0, 256, (6, 5, 3)).astype(np.uint8), "cpu")
    assert (f32.dtype, f32.channels, u8.dtype, u8.channels) == (np.float32, 3, np.uint8, 3)
    assert f32.values.dtype == f32.quantiles.dtype == torch.float64 and f32.lengths.dtype == torch.int32
    assert f32.values.shape == f32.quantiles.shape == (3, 30) and tuple(f32.lengths.shape) == (3,)
    with pytest.raises(ValueError, match="channels"):
        H.match_histograms(torch.zeros((2, 8, 8, 1)), f32)
    with pytest.raises(ValueError, match="channels"):
        H.match_histograms(torch.zeros((8, 8, 4), dtype=torch.uint8), u8)
    with pytest.raises(TypeError, match="uint8 reference"):
        H.match_histograms(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), f32)
    for dt in (torch.float64, torch.int16, torch.float16):
        with pytest.raises(TypeError, match="fp32 or uint8"):
            H.match_histograms(torch.zeros((2, 8, 8, 3), dtype=dt), f32)
    with pytest.raises(TypeError, match="multichannel"):
        H.match_histograms(torch.zeros((2, 8, 8, 3)), f32, multichannel=False)
    with pytest.raises(TypeError, match="HistReference"):
        H.match_histograms(torch.zeros((2, 8, 8, 3)), np.zeros((4, 4, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="dimensions"):
        H.match_histograms(torch.zeros((8, 3)), f32)
    # the kernel wrapper has no CPU fallback
    with pytest.raises(RuntimeError, match="HIP device"):
        H.match_histograms(torch.zeros((2, 8, 8, 3)), f32)


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_declares_what_the_binding_binds():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p}
    for name, ret in (("pcuda_match_hist", "int"), ("pcuda_match_hist_workspace_size", "size_t")):
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (s.strip() for s in m.group(2).split(","))]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
        assert name in _lib.EXPORTED_SYMBOLS
    m = re.search(r"int pcuda_match_hist\(([^;]*)\);", hdr)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "in", "out", "is_u8", "b", "h", "w", "c", "tvalues", "tquantiles", "tlen", "tstride", "workspace", "workspace_bytes", "s"]
    m = re.search(r"size_t pcuda_match_hist_workspace_size\(([^;]*)\);", hdr)
    assert [a.split()[-1] for a in m.group(1).split(",")] == ["b", "h", "w", "c", "is_u8"]
    assert int(re.search(r"#define\s+PCUDA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _lib.PCUDA_ABI_VERSION
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "histmatch.hip" in mk and "-ffp-contract=off" in mk
    src = open(os.path.join(CSRC, "histmatch.hip")).read()
    for sym in ('extern "C" int pcuda_match_hist(', 'extern "C" size_t pcuda_match_hist_workspace_size('):
        assert sym in src, sym
