"""GPU checks of the device-side spacing resample (csrc/resample.hip, pointcloududa_amd/utils/resample.py; DESIGN.md section 6,
f12) against the committed fixture tests/golden/resample.npz, whose expected arrays are the outputs of scipy.ndimage.zoom /
numpy themselves: the zoom and the labels equal them BIT FOR BIT; the statistics and the standardised values are held to the
bounds written at each test.  Only the fixture is read: scipy is not needed here."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_resample_golden", os.path.join(ROOT, "scripts", "make_resample_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
ZOOM, LABELS, STATS = G.load_cases(np.load(os.path.join(GOLD, "resample.npz")))
ZBY, LBY, SBY = ({c["name"]: c for c in cases} for cases in (ZOOM, LABELS, STATS))


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


@pytest.mark.parametrize("case", ZOOM, ids=[c["name"] for c in ZOOM])
def test_zoom_linear_equals_scipy_bit_for_bit(dev, case):
    from pointcloududa_amd.utils.resample import zoom_linear
    x = torch.from_numpy(case["vol"]).to(dev)
    out = zoom_linear(x, _factors(case), case["crop"])
    assert out.dtype == x.dtype and out.data_ptr() != x.data_ptr()
    assert not _diff(out, case["scipy"]), _diff(out, case["scipy"])
    assert np.array_equal(x.cpu().numpy().view(np.uint8), case["vol"].view(np.uint8)), "the input is never written"


@pytest.mark.parametrize("tag", ["f32", "i16", "u8"])
def test_zoom_into_a_misaligned_output_takes_the_scalar_stores_with_the_same_bits(dev, tag):
    """ow % 4 == 0 but the output starts one element into an allocation: no 4 / 8 / 16-byte stores there; the input starts one
    element into another"""
    from pointcloududa_amd import kernels as K
    for name in ("%s_37x41_to_50x33_crop24" % tag, "%s_256x256_to_267x267_crop224" % tag):
        case = ZBY[name]
        vol, want = torch.from_numpy(case["vol"]), case["scipy"]
        ibuf = torch.zeros(vol.numel() + 8, dtype=vol.dtype, device=dev)
        x = ibuf[1:1 + vol.numel()].view(vol.shape)
        x.copy_(vol.to(dev))
        obuf = torch.zeros(want.size + 8, dtype=vol.dtype, device=dev)
        out = obuf[1:1 + want.size].view(want.shape)
        assert out.data_ptr() % (4 * vol.element_size()) != 0 and want.shape[2] % 4 == 0
        K.zoom_linear_crop(x, (case["zh"], case["zw"]), case["crop"], out=out)
        assert not _diff(out, want), name
        assert obuf[0] == 0 and not obuf[1 + want.size:].any(), "nothing is written outside the output"


@pytest.mark.parametrize("case", LABELS, ids=[c["name"] for c in LABELS])
def test_zoom_labels_equals_argmax_of_the_zoomed_one_hot_bit_for_bit(dev, case):
    from pointcloududa_amd.utils.resample import zoom_labels
    x = torch.from_numpy(case["raw"]).to(dev)
    out = zoom_labels(x, _factors(case, "raw"), case["num_classes"], case["remap"], case["crop"])
    assert out.dtype == torch.uint8 and not _diff(out, case["scipy"]), _diff(out, case["scipy"])
    assert np.array_equal(x.cpu().numpy(), case["raw"]), "the input is never written"


def test_zoom_labels_check_raises_on_one_stray_code_and_only_then(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.resample import zoom_labels
    case = LBY["i16_discs_to_31x37_crop24"]
    f = _factors(case, "raw")
    raw = case["raw"].copy()
    raw[1, 0, 27] = 421                                            # one stray code, in a corner the crop window does not reach
    x = torch.from_numpy(raw).to(dev)
    with pytest.raises(ValueError, match="1 values of the volume are outside 0..3"):
        zoom_labels(x, f, 4, case["remap"], case["crop"])
    out = zoom_labels(x, f, 4, case["remap"], case["crop"], check=False)
    assert not _diff(out, case["scipy"]), "outside the window the stray code changes nothing"
    assert not _diff(zoom_labels(torch.from_numpy(case["raw"]).to(dev), f, 4, case["remap"], case["crop"], check=True), case["scipy"])
    # inside the window it matches no class: where every tap is the stray code all channels are 0 and argmax gives 0
    raw = case["raw"].copy()
    raw[0, 8:16, 8:16] = -5
    want, stray = G.label_rule(raw, case["zh"], case["zw"], 4, case["remap"], case["crop"])
    out, counter = K.zoom_labels(torch.from_numpy(raw).to(dev), (case["zh"], case["zw"]), 4, case["remap"], case["crop"])
    assert stray == 64 and int(counter.item()) == 64 and not _diff(out, want)
    # the pairs apply in order, like the chained np.where: 7 -> 200 -> 1
    raw = case["raw"].copy()
    raw[raw == 200] = 7
    chained = ((7, 200),) + tuple(case["remap"])
    assert not _diff(zoom_labels(torch.from_numpy(raw).to(dev), f, 4, chained, case["crop"]), case["scipy"])
    # a remapped value of 3 needs four classes
    with pytest.raises(ValueError, match="outside 0..2"):
        zoom_labels(torch.from_numpy(case["raw"]).to(dev), f, 3, case["remap"], case["crop"])


@pytest.mark.parametrize("case", STATS, ids=[c["name"] for c in STATS])
def test_standardize_zoomed_against_numpy(dev, case):
    """Integer volumes against numpy itself: the mean EQUALS numpy.mean's double; |std - numpy.std| <= n 2^-53 std (the worst-case
    bound of numpy's own float64 summation of n terms); every output within 1 fp32 ulp of float32((x - mean) / std) and at most
    1 % of them not bit-equal.  fp32 volumes against the fixture's float64-statistics restatement (this build's own convention)
    with the same bounds; the mean is compared for equality where the fixture's sums are exact in float64 in any order (the
    'exact_sums' volume), and within n 2^-53 mean(|x|) -- the same summation bound -- on the mixed-sign volume, whose float64
    sum depends on the order in its last bits."""
    from pointcloududa_amd.utils.resample import standardize_zoomed
    x = torch.from_numpy(case["vol"]).to(dev)
    is_f32 = case["vol"].dtype == np.float32
    ref_mean, ref_std = (float(v) for v in (case["rule_stats"] if is_f32 else case["numpy_stats"]))
    want = case["rule"] if is_f32 else case["numpy"]
    out, mean, std = standardize_zoomed(x, _factors(case), case["crop"], channels=1, return_stats=True)
    got = out.cpu().numpy()
    n = want.size
    ulps = _ulps(got, want)
    print("%s: mean %r (want %r), std %r (want %r, bound %.3g), %d of %d outputs not bit-equal, max %d ulp"
          % (case["name"], mean, ref_mean, std, ref_std, n * 2.0 ** -53 * ref_std, int(np.count_nonzero(ulps)), n, int(ulps.max())))
    if is_f32 and "exact" not in case["name"]:
        z = G.zoom_rule(case["vol"], case["zh"], case["zw"], case["crop"]).astype(np.float64)
        assert abs(mean - ref_mean) <= n * 2.0 ** -53 * float(np.mean(np.abs(z)))
    else:
        assert mean == ref_mean
    assert abs(std - ref_std) <= n * 2.0 ** -53 * ref_std
    assert got.shape == want.shape and int(ulps.max()) <= 1
    assert int(np.count_nonzero(ulps)) * 100 <= n
    assert np.array_equal(x.cpu().numpy().view(np.uint8), case["vol"].view(np.uint8)), "the input is never written"
    # the three-channel layout holds the same plane three times
    out3 = standardize_zoomed(x, _factors(case), case["crop"], channels=3)
    assert tuple(out3.shape) == (want.shape[0], 3) + want.shape[1:]
    for ch in range(3):
        assert np.array_equal(out3[:, ch].cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_standardize_takes_the_scalar_map_on_an_odd_plane_and_a_misaligned_output(dev):
    from pointcloududa_amd import kernels as K
    case = SBY["u8_20x24_to_21x25"]                                   # 21 * 25 values per slice: not a multiple of four
    x = torch.from_numpy(case["vol"]).to(dev)
    base, stats = K.zoom_standardize(x, (case["zh"], case["zw"]), case["crop"], 3)
    assert _ulps(base[:, 1].cpu().numpy(), case["numpy"]).max() <= 1
    case = SBY["i16_37x41_to_50x33_crop24"]
    x = torch.from_numpy(case["vol"]).to(dev)
    base, stats = K.zoom_standardize(x, (case["zh"], case["zw"]), case["crop"], 3)
    buf = torch.zeros(base.numel() + 8, dtype=torch.float32, device=dev)
    out = buf[1:1 + base.numel()].view(base.shape)
    assert out.data_ptr() % 16 != 0
    K.zoom_standardize(x, (case["zh"], case["zw"]), case["crop"], 3, out=out, stats=stats)
    assert torch.equal(out, base) and buf[0] == 0 and not buf[1 + base.numel():].any()
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (2,) and stats.tolist()[0] == float(case["numpy_stats"][0])


def test_two_runs_of_every_entry_point_give_identical_bits(dev):
    from pointcloududa_amd.utils import resample as R
    for name in ("f32_256x256_to_267x267_crop224", "i16_256x256_to_267x267_crop224", "u8_37x41_to_50x33_crop24"):
        case = ZBY[name]
        x, f = torch.from_numpy(case["vol"]).to(dev), _factors(case)
        for _ in range(2):
            a, b = R.zoom_linear(x, f, case["crop"]), R.zoom_linear(x, f, case["crop"])
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            (sa, ma, da), (sb, mb, db) = (R.standardize_zoomed(x, f, case["crop"], 3, return_stats=True) for _ in range(2))
            assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)) and (ma, da) == (mb, db)
    case = LBY["i16_discs_to_31x37"]
    x, f = torch.from_numpy(case["raw"]).to(dev), _factors(case, "raw")
    assert torch.equal(R.zoom_labels(x, f, 4, case["remap"], 0), R.zoom_labels(x, f, 4, case["remap"], 0))


def test_empty_volumes_views_and_out_arguments(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import resample as R
    e = torch.zeros((0, 16, 16), dtype=torch.int16, device=dev)
    assert tuple(R.zoom_linear(e, (1.5, 1.25)).shape) == (0, 24, 20) and R.zoom_linear(e, (1.5, 1.25)).dtype == torch.int16
    assert tuple(R.standardize_zoomed(e, (1.5, 1.5), crop_size=12, channels=3).shape) == (0, 3, 12, 12)
    assert tuple(R.zoom_labels(e, (1.5, 1.5), crop_size=12).shape) == (0, 12, 12)
    # a non-contiguous view gives what its contiguous copy gives
    case = ZBY["i16_37x41_to_50x33_crop24"]
    wide = torch.zeros((2, 37, 60), dtype=torch.int16, device=dev)
    wide[:, :, 5:46] = torch.from_numpy(case["vol"]).to(dev)
    view = wide[:, :, 5:46]
    assert not view.is_contiguous()
    f = _factors(case)
    assert not _diff(R.zoom_linear(view, f, 24), case["scipy"])
    assert torch.equal(R.standardize_zoomed(view, f, 24), R.standardize_zoomed(view.contiguous(), f, 24))
    lcase = LBY["i16_discs_to_31x37_crop24"]
    lwide = torch.zeros((3, 24, 40), dtype=torch.int16, device=dev)
    lwide[:, :, 3:31] = torch.from_numpy(lcase["raw"]).to(dev)
    assert not _diff(R.zoom_labels(lwide[:, :, 3:31], _factors(lcase, "raw"), 4, lcase["remap"], 24), lcase["scipy"])
    # out= of the wrong shape or dtype raises; in == out is rejected by the library
    x = torch.from_numpy(case["vol"]).to(dev)
    with pytest.raises(ValueError, match="out does not match"):
        K.zoom_linear_crop(x, (50, 33), 24, out=torch.empty((2, 24, 20), dtype=torch.int16, device=dev))
    with pytest.raises(TypeError):
        K.zoom_linear_crop(x, (50, 33), 24, out=torch.empty((2, 24, 24), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="out does not match"):
        K.zoom_standardize(x, (50, 33), 24, 3, out=torch.empty((2, 24, 24), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="out does not match"):
        K.zoom_labels(x, (50, 33), 4, (), 24, out=torch.empty((2, 24, 25), dtype=torch.uint8, device=dev))
    same = torch.zeros((2, 8, 8), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="in == out"):
        K.zoom_linear_crop(same, (8, 8), 0, out=same)
    with pytest.raises(RuntimeError, match="in == out"):
        K.zoom_labels(same, (8, 8), 4, (), 0, out=same)
    with pytest.raises(TypeError):
        K.zoom_labels(torch.zeros((2, 8, 8), device=dev), (8, 8))
    torch.cuda.synchronize()


def test_prepare_mscmrseg_npy_equals_the_composition_of_its_parts(dev):
    from pointcloududa_amd.utils import resample as R
    case, lcase = SBY["i16_256x256_to_267x267_crop224"], LBY["i16_discs_to_25x29"]
    x = torch.from_numpy(case["vol"]).to(dev)
    f = R.spacing_zoom_factors((256, 256), (1.25, 1.25))
    assert R.zoom_output_shape((256, 256), f) == (267, 267)
    got = R.prepare_mscmrseg_npy(x, (1.25, 1.25))
    assert tuple(got.shape) == (2, 3, 224, 224) and torch.equal(got, R.standardize_zoomed(x, f, 224, channels=3))
    one = R.prepare_mscmrseg_npy(x, (1.25, 1.25), channels=1)
    assert _ulps(one.cpu().numpy(), case["numpy"]).max() <= 1 and torch.equal(one, got[:, 0])
    # ... and of the zoom on its own, the statistics by torch in float64, the map in float64
    z = R.zoom_linear(x, f, 224)
    assert not _diff(z, G.zoom_rule(case["vol"], 267, 267, 224))
    from pointcloududa_amd import kernels as K
    _, stats = K.zoom_standardize(x, (267, 267), 224, 1)
    assert torch.equal(((z.double() - stats[0]) / stats[1]).float(), one), "a tensor by a tensor: torch divides, it does not multiply by 1 / std"
    # labels: 0.25 mm on a 24x28 slice to 0.24 mm gives 25x29, whichever axis the reference hands each factor to
    raw = torch.from_numpy(lcase["raw"]).to(dev)
    assert not _diff(R.prepare_mscmrseg_npy_labels(raw, (0.25, 0.25), (0.24, 0.24), crop_size=0), lcase["scipy"])
    square = torch.from_numpy(np.ascontiguousarray(lcase["raw"][:, :, :24])).to(dev)
    sf = R.spacing_zoom_factors((24, 24), (1.25, 1.25), (1.2, 1.2))
    assert torch.equal(R.prepare_mscmrseg_npy_labels(square, (1.25, 1.25), crop_size=20), R.zoom_labels(square, sf, crop_size=20))


def test_the_resample_adds_no_host_synchronisation(dev):
    from pointcloududa_amd.utils import resample as R
    case, lcase = ZBY["i16_37x41_to_50x33_crop24"], LBY["i16_discs_to_31x37_crop24"]
    x, f = torch.from_numpy(case["vol"]).to(dev), _factors(case)
    raw, lf = torch.from_numpy(lcase["raw"]).to(dev), _factors(lcase, "raw")
    fx = torch.from_numpy(ZBY["f32_37x41_to_50x33_crop24"]["vol"]).to(dev)
    want = (R.zoom_linear(x, f, 24), R.standardize_zoomed(x, f, 24, channels=3), R.standardize_zoomed(fx, f, 24),
            R.zoom_labels(raw, lf, 4, lcase["remap"], 24, check=False))       # (warm: allocator, library load)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = (R.zoom_linear(x, f, 24), R.standardize_zoomed(x, f, 24, channels=3, return_stats=False), R.standardize_zoomed(fx, f, 24),
               R.zoom_labels(raw, lf, 4, lcase["remap"], 24, check=False))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(got, want):
        assert torch.equal(a, b)
