"""GPU checks of the device-side spacing resample (csrc/resample.hip) at its dispatch edges, against the committed fixture
tests/golden/resample_edges.npz (scipy's / numpy's own outputs; tests/test_resample_edges.py asserts on the CPU that each case
reaches the branch it is there for): labels over more than one band of rows, with real ties, eight classes and eight remap
pairs; rows wider than 1024 columns, one output column, an input axis of one sample, weights of exactly 0.5; a statistics
reduce that loops, a variance numerator beyond 64 bits, the capped second pass of the fp32 statistics.  The zoom and the labels
equal scipy BIT FOR BIT; the statistics are held to the bounds of test_standardize_zoomed_against_numpy (test_resample_gpu.py)
and, for integers, to 2 ulp of the exact route.  Only committed files are read: scipy is not needed here."""
import functools
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_resample_golden", os.path.join(ROOT, "scripts", "make_resample_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
ZOOM, LABELS, STATS = G.load_edge_cases(np.load(os.path.join(GOLD, "resample_edges.npz")))
LBY, SBY = ({c["name"]: c for c in cases} for cases in (LABELS, STATS))


def _diff(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    bits = "u%d" % want.itemsize
    bad = np.flatnonzero(np.ascontiguousarray(got).ravel().view(bits) != np.ascontiguousarray(want).ravel().view(bits))
    return "%d of %d values differ, first at %s: got %s, want %s" % (
        len(bad), want.size, np.unravel_index(bad[0], want.shape) if len(bad) else None,
        got.ravel()[bad[:4]].tolist(), want.ravel()[bad[:4]].tolist()) if len(bad) else ""


def _factors(case, key="vol"):
    """zoom factors that give the case's zoomed size, as a caller of scipy.ndimage.zoom passes them"""
    from pointcloududa_amd.utils.resample import zoom_output_shape
    h, w = case[key].shape[1:]
    f = (case["zh"] / h, case["zw"] / w)
    assert zoom_output_shape((h, w), f) == (case["zh"], case["zw"])
    return f


def _ulps(got, want):
    """distance in fp32 units in the last place; NaN against NaN and equal infinities count 0"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    a, b = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7fffffff), a), np.where(b < 0, -(b & 0x7fffffff), b)
    d = np.abs(a - b)
    d[same] = 0
    d[~same & ~(np.isfinite(got) & np.isfinite(want))] = 1 << 40
    return d


def _ulps64(a, b):
    """distance of two positive finite doubles in units in the last place"""
    assert a > 0.0 and b > 0.0
    return abs(struct.unpack("<q", struct.pack("<d", a))[0] - struct.unpack("<q", struct.pack("<d", b))[0])


@functools.lru_cache(maxsize=None)
def _expected(name):
    """of a statistics case, computed once and left unchanged: (the zoomed values -- the restatement's, trusted after their digest
    equalled the one of scipy's bytes --, numpy's standardised outputs, the restatement's statistics)"""
    case = SBY[name]
    z, numpy_out = G.expected_stat_arrays(case)
    rule = G.f32_stats(z) if z.dtype == np.float32 else G.int_stats(z)
    assert rule == tuple(float(v) for v in case["rule_stats"]), name
    z.setflags(write=False)
    numpy_out.setflags(write=False)
    return z, numpy_out, rule


@pytest.mark.parametrize("case", ZOOM, ids=[c["name"] for c in ZOOM])
def test_zoom_linear_at_the_edges_equals_scipy_bit_for_bit(dev, case):
    """9x5 -> 17x17: weights of exactly 0.5 and 0.25, round_int decided on ties of either sign; 3x300 -> 5x1030 / 5x1028: 258 / 257
    column groups, the second trip of the group loop with scalar / vector stores; 6x1 -> 9x4 and 1x6 -> 4x9: an input axis of one
    sample; 6x7 -> 40x1: one output column over two bands; the int16 limits: the clamp of round_int"""
    from pointcloududa_amd.utils.resample import zoom_linear
    x = torch.from_numpy(case["vol"]).to(dev)
    out = zoom_linear(x, _factors(case), case["crop"])
    assert out.dtype == x.dtype and out.data_ptr() != x.data_ptr()
    assert not _diff(out, case["scipy"]), _diff(out, case["scipy"])
    assert np.array_equal(x.cpu().numpy().view(np.uint8), case["vol"].view(np.uint8)), "the input is never written"


@pytest.mark.parametrize("case", LABELS, ids=[c["name"] for c in LABELS])
def test_zoom_labels_at_the_edges_equals_argmax_of_the_zoomed_one_hot_bit_for_bit(dev, case):
    """7, 2 and 3 bands of rows (img = blockIdx.x / bands), eight classes, eight remap pairs with a chained one, uint8 with vector
    stores, pixels with two channels at 1 (the first class wins) and with none (class 0), one-sample axes, 258 column groups"""
    from pointcloududa_amd.utils.resample import zoom_labels
    x = torch.from_numpy(case["raw"]).to(dev)
    out = zoom_labels(x, _factors(case, "raw"), case["num_classes"], case["remap"], case["crop"])
    assert out.dtype == torch.uint8 and not _diff(out, case["scipy"]), _diff(out, case["scipy"])
    assert np.array_equal(x.cpu().numpy(), case["raw"]), "the input is never written"


def test_the_production_label_call_runs_seven_bands(dev):
    """prepare_mscmrseg_npy_labels(..., crop_size=224) on 40x44 slices.  The reference hands the factor of GetSize()[0] = 44 to the
    first array axis (40 rows) and the other to the second: 294 / 44 and 243 / 40 give round(40 * 6.68..) x round(44 * 6.075) =
    267x267, the fixture's zoomed size (the kernel takes the size, not the factors)"""
    from pointcloududa_amd.utils import resample as R
    case = LBY["u8_blocks8_to_267x267_crop224"]
    spacing = (1.2 * 294 / 44, 1.2 * 243 / 40)                         # GetSpacing()[:2]
    assert R.spacing_zoom_factors((44, 40), spacing) == (294 / 44, 243 / 40)
    assert R.zoom_output_shape((40, 44), R.spacing_zoom_factors((44, 40), spacing)) == (267, 267)
    x = torch.from_numpy(case["raw"]).to(dev)
    out = R.prepare_mscmrseg_npy_labels(x, spacing, crop_size=224, num_classes=8, remap=())
    assert tuple(out.shape) == (3, 224, 224) and not _diff(out, case["scipy"]), _diff(out, case["scipy"])


def test_labels_into_a_misaligned_output_take_the_scalar_stores_with_the_same_bits(dev):
    """ow % 4 == 0 but the output starts one byte into an allocation: no dword stores there"""
    from pointcloududa_amd import kernels as K
    case = LBY["u8_noise8_to_70x76_crop64"]
    want = case["scipy"]
    x = torch.from_numpy(case["raw"]).to(dev)
    obuf = torch.full((want.size + 16,), 0xA5, dtype=torch.uint8, device=dev)
    out = obuf[1:1 + want.size].view(want.shape)
    assert out.data_ptr() % 4 == 1 and want.shape[2] % 4 == 0
    _, counter = K.zoom_labels(x, (case["zh"], case["zw"]), 8, case["remap"], case["crop"], out=out)
    assert not _diff(out, want), _diff(out, want)
    assert int(counter.item()) == 0
    assert obuf[0] == 0xA5 and bool((obuf[1 + want.size:] == 0xA5).all()), "nothing is written outside the output"


@pytest.mark.parametrize("case", STATS, ids=[c["name"] for c in STATS])
def test_standardize_zoomed_at_the_edges_against_numpy(dev, case):
    """The bounds of test_standardize_zoomed_against_numpy.  Integer volumes: the mean EQUALS numpy.mean's double; |std -
    numpy.std| <= n 2^-53 std; every output within 1 fp32 ulp of float32((x - mean) / std) by numpy's statistics, at most 1 % not
    bit-equal.  The exact-sum fp32 volume: the mean equals the restatement's, the same bounds (the mixed-sign fp32 volume of
    many_520: the mean within n 2^-53 mean(|x|), as there).  One tighter bound for integers:
    the std within 2 ulp of int_stats on the zoomed values -- both sides convert the same exact integer n Sxx - Sx Sx with one
    rounding and divide by the same exact n n, which leaves one ulp for a division and one for a sqrt that are not correctly
    rounded on the device.  many_520: 1040 partials, every lane of the one-workgroup reduce takes 4 or 5; fullscale and
    nearconstant: n Sxx beyond 2^64, the shift and sticky-bit path of u128_to_double; f32_exact: sqdev_partial_kernel capped at
    1024 workgroups, 294 partials into the first reduce."""
    from pointcloududa_amd.utils.resample import standardize_zoomed
    z, want, rule = _expected(case["name"])
    x = torch.from_numpy(case["vol"]).to(dev)
    is_f32 = case["vol"].dtype == np.float32
    ref_mean, ref_std = rule if is_f32 else (float(v) for v in case["numpy_stats"])
    if is_f32:
        want = G.standardize_rule(z, ref_mean, ref_std)
    out, mean, std = standardize_zoomed(x, _factors(case), case["crop"], channels=1, return_stats=True)
    got = out.cpu().numpy()
    n = want.size
    ulps = _ulps(got, want)
    print("%s: mean %r (want %r), std %r (want %r, bound %.3g; the exact route %r: %d ulp away), %d of %d outputs not bit-equal, max %d ulp"
          % (case["name"], mean, ref_mean, std, ref_std, n * 2.0 ** -53 * ref_std, rule[1], _ulps64(std, rule[1]),
             int(np.count_nonzero(ulps)), n, int(ulps.max())))
    if is_f32 and "exact" not in case["name"]:
        assert abs(mean - ref_mean) <= n * 2.0 ** -53 * float(np.mean(np.abs(z.astype(np.float64))))
    else:
        assert mean == ref_mean
    assert abs(std - ref_std) <= n * 2.0 ** -53 * ref_std
    if not is_f32:
        assert _ulps64(std, rule[1]) <= 2
    assert got.shape == want.shape and int(ulps.max()) <= 1
    assert int(np.count_nonzero(ulps)) * 100 <= n
    assert np.array_equal(x.cpu().numpy().view(np.uint8), case["vol"].view(np.uint8)), "the input is never written"
    # the three-channel layout holds the same plane three times
    out3 = standardize_zoomed(x, _factors(case), case["crop"], channels=3)
    assert tuple(out3.shape) == (want.shape[0], 3) + want.shape[1:]
    for ch in range(3):
        assert torch.equal(out3[:, ch].view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("tag", ["f32", "i16", "u8"])
def test_the_entry_point_stays_inside_the_workspace_it_asks_for_past_the_reduce_floor(dev, tag):
    """n * bands = 1040 > kReduceBlocks: partial_bytes leaves its floor.  pcuda_zoom_standardize called through the binding with
    256 bytes of sentinel behind the workspace it asked for: they stay untouched and the result is the wrapper's."""
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    case = SBY["%s_many_520x3x3_to_33x4" % tag]
    x = torch.from_numpy(case["vol"]).to(dev)
    n, sh, sw = x.shape
    dt = {"f32": 0, "i16": 1, "u8": 2}[tag]
    base, base_stats = K.zoom_standardize(x, (case["zh"], case["zw"]), case["crop"], 1)
    need = L.lib().pcuda_zoom_standardize_workspace_size(dt, n, case["zh"], case["zw"], case["crop"])
    table = (36 + 4) * 12                                              # 33 rows padded to 36, 4 columns; 12 bytes an entry
    assert need == (table + 15) // 16 * 16 + 1040 * 16 + (n * 33 * 4 * x.element_size() + 15) // 16 * 16
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    out = torch.empty((n, 33, 4), dtype=torch.float32, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    L.check(L.lib().pcuda_zoom_standardize(x.data_ptr(), dt, n, sh, sw, case["zh"], case["zw"], case["crop"], 1, out.data_ptr(),
                                           stats.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "zoom_standardize")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "the 256 bytes behind the workspace are untouched"
    assert torch.equal(out.view(torch.int32), base.view(torch.int32)) and torch.equal(stats.view(torch.int64), base_stats.view(torch.int64))
    if tag != "f32":
        assert stats.tolist()[0] == float(case["rule_stats"][0])
