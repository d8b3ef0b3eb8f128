"""Device-side histogram matching on the GPU, through the public surface (utils/augment.py,
utils/histmatch.py) and the C ABI, against the committed fixture tests/golden/match_hist.npz and the plain-numpy restatement
of skimage's match_histograms run live (scripts/make_match_hist_golden.py: two forms that equal each other bit for bit).

Rule: EXACT equality, no tolerance.  The count of values <= s is an integer, the quantile one float64 division, the
interpolation four float64 operations rounded one by one (the library is built with -ffp-contract=off), the cast a
round-to-nearest-even (fp32) or a truncation (uint8).  A difference is a rank error or a contraction, never noise."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "scripts"))
try:
    _spec = importlib.util.spec_from_file_location("make_match_hist_golden", os.path.join(ROOT, "scripts", "make_match_hist_golden.py"))
    G = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(G)
finally:
    sys.path.remove(os.path.join(ROOT, "scripts"))
CASES = G.load_cases(np.load(os.path.join(GOLD, "match_hist.npz")))
F32 = [c["name"] for c in CASES if c["images"].dtype == np.float32]
U8 = [c["name"] for c in CASES if c["images"].dtype == np.uint8]
SORT_TILE = 4096      # csrc/histmatch.hip: kSortTile = 1024 lanes x 4 keys; a wave takes 256 consecutive keys in rounds of 64


def _case(name):
    return [c for c in CASES if c["name"] == name][0]


def _run(dev, images, reference):
    from pointcloududa_amd.utils.histmatch import HistReference, match_histograms
    x = torch.from_numpy(images).to(dev)
    keep = x.clone()
    out = match_histograms(x, HistReference(reference, dev))
    assert out.dtype == x.dtype and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x.view(torch.uint8), keep.view(torch.uint8)), "the input is never written"
    return out.cpu().numpy()


def _check(got, want, name):
    bad = got != want
    print("%s: %d values, %d differ" % (name, got.size, int(bad.sum())))
    assert got.dtype == want.dtype and got.shape == want.shape
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


# ---------------------------------------------------------------------------------------------- fp32
@pytest.mark.parametrize("name", F32)
def test_fp32_fixture_cases_are_exact(dev, name):
    """B = 3 with different content per sample and M != N (plane indexing); the key-coverage plane (every radix pass moves
    data); 37-level ties and a constant plane (cnt = N, q = 1: the template's maximum); both zeros; 1x1, 5x3 (less than a
    wave) and 63x65"""
    c = _case(name)
    _check(_run(dev, c["images"], c["reference"]), c["expected"], name)


def test_fp32_constant_plane_takes_the_template_maximum(dev):
    c = _case("f32_constant_16x16x1")
    got = _run(dev, c["images"], c["reference"])
    assert np.all(got == c["reference"].max())


@pytest.mark.parametrize("shape", [(1, 64, 64, 1), (1, 17, 241, 1), (1, 63, 65, 2), (1, 31, 33, 1), (2, 257, 130, 1)],
                         ids=["one_tile", "one_tile_plus_1", "one_tile_minus_1", "wave_chunks_ragged", "257x130"])
def test_fp32_tile_edges_against_the_live_restatement(dev, shape):
    """H W exactly the sort's tile, one more, one less, a quarter of a tile that ends inside a wave's last round, and more than
    twice the tile without being a multiple of it"""
    n = shape[1] * shape[2]
    assert abs(n - SORT_TILE) <= 1 or n == 1023 or (n > 2 * SORT_TILE and n % SORT_TILE != 0)
    img = G.normal_f32(shape, 40 + n % 7, 3.0, 10.0)
    img[0, :5, :7, 0] = img[0, 6, 6, 0]                  # some ties across the first tile
    ref = G.normal_f32((40, 30, shape[3]), 41, -1.0, 2.0)
    _check(_run(dev, img, ref), G.match_unique(img, ref), "tile edge %r" % (shape,))


def test_fp32_the_workload_plane(dev):
    """B = 2, 256x256x3 (the reference's slices), a 256x256x3 template"""
    img, ref = G.normal_f32((2, 256, 256, 3), 50, 100.0, 300.0), G.normal_f32((256, 256, 3), 51, 0.0, 1.0)
    _check(_run(dev, img, ref), G.match_unique(img, ref), "workload plane")


def test_a_single_hwc_image_is_taken_as_the_reference_does(dev):
    from pointcloududa_amd.utils.histmatch import HistReference, match_histograms
    c = _case("f32_normal_b3_64x64x3")
    out = match_histograms(torch.from_numpy(c["images"][1]).to(dev), HistReference(c["reference"], dev))
    assert out.shape == (64, 64, 3)
    _check(out.cpu().numpy(), c["expected"][1], "single [H,W,C] image")


# ---------------------------------------------------------------------------------------------- uint8
@pytest.mark.parametrize("name", U8)
def test_uint8_fixture_cases_are_exact(dev, name):
    """64x64x3, 33x47x1 and a constant plane: the histogram / LUT path, truncation toward zero"""
    c = _case(name)
    _check(_run(dev, c["images"], c["reference"]), c["expected"], name)


def test_uint8_images_refuse_a_non_uint8_reference(dev):
    from pointcloududa_amd.utils.histmatch import HistReference, match_histograms
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError, match="uint8 reference"):
        match_histograms(x, HistReference(G.normal_f32((8, 8, 3), 1), dev))
    with pytest.raises(ValueError, match="channels"):
        match_histograms(x, HistReference(G.random_u8((8, 8, 1), 1), dev))


# ---------------------------------------------------------------------------------------------- contract
def test_entry_point_returns_status_codes(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd.utils.histmatch import HistReference
    lib = _lib.lib()
    b, h, w, c = 2, 24, 40, 3
    x = torch.from_numpy(G.normal_f32((b, h, w, c), 60)).to(dev)
    out = torch.full_like(x, 7.0)
    ref = HistReference(G.normal_f32((10, 10, c), 61), dev)
    need = lib.pcuda_match_hist_workspace_size(b, h, w, c, 0)
    assert need >= 8 * b * h * w * c and need % 16 == 0
    assert lib.pcuda_match_hist_workspace_size(0, h, w, c, 0) == 0 and lib.pcuda_match_hist_workspace_size(b, h, w, c, 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    tstride = ref.values.shape[1]

    def call(inp=x.data_ptr(), outp=out.data_ptr(), u8=0, b=b, h=h, w=w, c=c, tv=ref.values.data_ptr(), tq=ref.quantiles.data_ptr(),
             tl=ref.lengths.data_ptr(), ts=tstride, wsp=ws.data_ptr(), nbytes=need):
        return lib.pcuda_match_hist(inp, outp, u8, b, h, w, c, tv, tq, tl, ts, wsp, nbytes, stream)
    assert call(outp=x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(wsp=None) == -4
    for kw in (dict(inp=None), dict(outp=None), dict(b=-1), dict(h=-1), dict(c=0), dict(c=5), dict(tv=None), dict(tq=None),
               dict(tl=None), dict(ts=0)):
        assert call(**kw) == -1, kw
    assert call(b=0) == 0 and call(h=0) == 0 and call(w=0, inp=None, outp=None, wsp=None, nbytes=0) == 0, "b h w == 0 is a no-op"
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a rejected call and a no-op launch nothing"
    assert call() == 0
    torch.cuda.synchronize()
    _check(out.cpu().numpy(), G.match_unique(x.cpu().numpy(), G.normal_f32((10, 10, c), 61)), "C ABI call")


def test_the_kernel_wrapper_checks_the_tables(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.histmatch import HistReference
    ref = HistReference(G.normal_f32((10, 10, 2), 61), dev)
    x = torch.zeros((1, 8, 8, 3), device=dev)
    with pytest.raises(ValueError, match="channels"):
        K.match_hist(x, ref.values, ref.quantiles, ref.lengths)
    with pytest.raises(TypeError):
        K.match_hist(x[..., :2].contiguous(), ref.values.float(), ref.quantiles, ref.lengths)


def test_two_calls_give_identical_bits(dev):
    from pointcloududa_amd.utils.histmatch import HistReference, match_histograms
    for img, refimg in ((G.levels_f32((2, 70, 90, 3), 70), G.normal_f32((30, 30, 3), 71)),
                        (G.random_u8((2, 70, 90, 3), 72), G.random_u8((30, 30, 3), 73))):
        x, ref = torch.from_numpy(img).to(dev), HistReference(refimg, dev)
        a, b = match_histograms(x, ref), match_histograms(x, ref)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        _check(a.cpu().numpy(), G.match_unique(img, refimg), "repeat")


# ---------------------------------------------------------------------------------------------- integration
def _batch(dev, dtype, b=3, h=64, w=64, c=3, seed=80):
    rng = np.random.default_rng(seed)
    img = G.normal_f32((b, h, w, c), seed, 200.0, 400.0) if dtype == np.float32 else G.smooth_u8((b, h, w, c), seed)
    lab = rng.integers(0, 5, (b, h, w)).astype(np.int64)
    refimg = G.normal_f32((48, 80, c), seed + 1, 0.0, 1.0) if dtype == np.float32 else G.random_u8((48, 80, c), seed + 1, 20, 230)
    return img, lab, refimg, torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)


def test_augment_batch_without_augmentation_is_assemble_batch_of_the_matched_images(dev):
    """params=None, rescale=None with match_hist: the generator's aug='' branch with -mh"""
    from pointcloududa_amd.utils.augment import HistReference, augment_batch, match_histograms
    from pointcloududa_amd.utils.batch import assemble_batch
    img, lab, refimg, tx, tl = _batch(dev, np.float32)
    ref = HistReference(refimg, dev)
    got = augment_batch(tx, tl, None, 5, 48, rescale=None, match_hist=ref)
    matched = match_histograms(tx, ref)
    want = assemble_batch(matched, tl, 5, 48)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] is None and want[2] is None
    _check(matched.cpu().numpy(), G.match_unique(img, refimg), "matched batch")
    plain = augment_batch(tx, tl, None, 5, 48, rescale=None)
    assert torch.equal(plain[1], got[1]) and not torch.equal(plain[0], got[0]), "masks are untouched, images are not"


def test_augment_batch_minmax_sees_the_matched_images(dev):
    """the batch min / max are those of the matched images: the same light parameters on pre-matched images"""
    from pointcloududa_amd.utils.augment import HistReference, augment_batch, match_histograms, sample_params
    img, lab, refimg, tx, tl = _batch(dev, np.float32, seed=82)
    ref = HistReference(refimg, dev)
    params = sample_params(3, "mmwhs_light", np.random.default_rng(6))
    params.affine_on[:2] = True
    one = augment_batch(tx, tl, params, 5, 48, rescale="minmax", match_hist=ref)
    two = augment_batch(match_histograms(tx, ref), tl, params, 5, 48, rescale="minmax")
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    assert not torch.equal(one[0], augment_batch(tx, tl, params, 5, 48, rescale="minmax")[0])
    # None changes nothing by a bit
    a, b = augment_batch(tx, tl, params, 5, 48, rescale="minmax"), augment_batch(tx, tl, params, 5, 48, rescale="minmax", match_hist=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_uint8_path_composes_with_a_photometric_program(dev):
    from pointcloududa_amd.utils.augment import (HistReference, augment_batch, match_histograms, photometric_aug, sample_params,
                                                 sample_program)
    img, lab, refimg, tx, tl = _batch(dev, np.uint8, seed=84)
    ref = HistReference(refimg, dev)
    params = sample_params(3, "mscmrseg_simple", np.random.default_rng(3))
    prog = sample_program(3, "mscmrseg_aug2_photometric", np.random.default_rng(4))
    one = augment_batch(tx, tl, params, 5, 48, rescale="div255", photometric=prog, match_hist=ref)
    matched = match_histograms(tx, ref)
    two = augment_batch(photometric_aug(matched, prog), tl, params, 5, 48, rescale="div255")
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    _check(matched.cpu().numpy(), G.match_unique(img, refimg), "matched uint8 batch")


def test_augmented_batches_with_a_reference_yield_the_manual_sequence(dev):
    from pointcloududa_amd.utils.augment import AugmentedBatches, HistReference, augment_batch, sample_params
    raw, refimg = [], None
    for i in range(2):
        img, lab, refimg, _, _ = _batch(dev, np.float32, seed=90 + 2 * i)
        raw.append((img, lab[..., None]))
    refimg = G.normal_f32((40, 40, 3), 99)
    it = AugmentedBatches(iter(raw), dev, "mmwhs_light", np.random.default_rng(77), num_classes=5, crop_size=48, rescale="minmax",
                          resample_verts=False, match_hist_reference=refimg)
    assert it.match_hist.channels == 3 and it.match_hist.dtype == np.float32
    twin, ref, n = np.random.default_rng(77), HistReference(refimg, dev), 0
    for (x, y, z), (img, lab) in zip(it, raw):
        want = augment_batch(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), sample_params(3, "mmwhs_light", twin), 5, 48,
                             "minmax", match_hist=ref)
        assert torch.equal(x, want[0]) and torch.equal(y, want[1]) and z is None
        n += 1
    assert n == 2
    plain = AugmentedBatches(iter(raw), dev, "mmwhs_light", np.random.default_rng(77), num_classes=5, crop_size=48, rescale="minmax",
                             resample_verts=False)
    assert plain.match_hist is None


def test_the_match_hist_path_adds_no_host_synchronisation(dev):
    """match_histograms (fp32 and uint8) and augment_batch(.., match_hist=..) under torch.cuda.set_sync_debug_mode("error"); the
    mode is first shown to be enforced (a ``.item()`` raises under it)"""
    from pointcloududa_amd.utils.augment import HistReference, augment_batch, match_histograms, sample_params
    img, lab, refimg, tx, tl = _batch(dev, np.float32, seed=86)
    q, _, refq, tq, _ = _batch(dev, np.uint8, seed=87)
    ref, ref8 = HistReference(refimg, dev), HistReference(refq, dev)
    params = sample_params(3, "mmwhs_light", np.random.default_rng(3))
    want_m, want_q = match_histograms(tx, ref), match_histograms(tq, ref8)               # (warm: allocator, library load)
    want = augment_batch(tx, tl, params, 5, 48, rescale="minmax", match_hist=ref)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        a, a8 = match_histograms(tx, ref), match_histograms(tq, ref8)
        b = augment_batch(tx, tl, params, 5, 48, rescale="minmax", match_hist=ref)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, want_m) and torch.equal(a8, want_q) and torch.equal(b[0], want[0]) and torch.equal(b[1], want[1])
