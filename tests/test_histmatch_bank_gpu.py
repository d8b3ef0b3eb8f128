"""Histogram matching against a reference bank on the GPU, through the public surface
(utils/histmatch.py, utils/augment.py) and the C ABI.  The expected arrays are ``match_unique`` of
scripts/make_match_hist_golden.py applied sample by sample with ``references[index[i]] + 0.0`` and cross-checked against
``match_sorted`` (tests/histmatch_bank_ref.py ``expected``).

Rule: EXACT equality, no tolerance, no excused element: the ranks are integers, the quantiles single float64 divisions, the
interpolation four float64 operations rounded one by one, the cast a round-to-nearest-even (fp32) or a truncation (uint8)."""
import numpy as np
import pytest
import torch

import histmatch_bank_ref as R

pytestmark = pytest.mark.gpu

G = R.G
SORT_TILE = 4096      # csrc/histmatch_device.h: kSortTile


def _check(got, want, name):
    bad = got != want
    print("%s: %d values, %d differ" % (name, got.size, int(bad.sum())))
    assert got.dtype == want.dtype and got.shape == want.shape
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def _run(dev, images, refs, index, **kw):
    from pointcloududa_amd.utils.histmatch import HistReferenceBank, match_histograms
    x = torch.from_numpy(images).to(dev)
    keep = x.clone()
    bank = HistReferenceBank(refs, dev, **kw)
    assert (bank.size, bank.channels, bank.dtype, bank.shape) == (refs.shape[0], refs.shape[3], refs.dtype, refs.shape)
    out = match_histograms(x, bank, index=index)
    assert out.dtype == x.dtype and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x.view(torch.uint8), keep.view(torch.uint8)), "the input is never written"
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------- fp32
@pytest.mark.parametrize("name", sorted(R.IMAGE_SHAPES))
def test_fp32_tile_edges_against_every_reference_plane(dev, name):
    """image planes of exactly one sort tile, one key more, one less (C = 2), below a tile and several tiles (B = 2), each
    against reference planes of 64x64, 31x33, 17x241 and 32x64 (M != N but for 64x64 / 64x64; 64x64 / 32x64: cnt / N equals
    e / M exactly with different operands); normal, 37-level and key-coverage content on both sides"""
    n = R.IMAGE_SHAPES[name][1] * R.IMAGE_SHAPES[name][2]
    assert abs(n - SORT_TILE) <= 1 or n < SORT_TILE // 2 or (n > 2 * SORT_TILE and n % SORT_TILE != 0)
    for images, refs, index in R.f32_pairings(name):
        _check(_run(dev, images, refs, index), R.expected(images, refs, index), "%s / %dx%d" % (name, refs.shape[1], refs.shape[2]))


@pytest.mark.parametrize("c", [3, 4])
def test_fp32_three_and_four_channels(dev, c):
    images, refs = R.f32_set(3, 31, 33, c, 300 + c, False), R.f32_set(2, 20, 27, c, 310 + c, True)
    _check(_run(dev, images, refs, [1, 0, 1]), R.expected(images, refs, [1, 0, 1]), "C = %d" % c)


def test_fp32_degenerate_planes(dev):
    """a constant and a two-level reference plane, a constant image plane, references that hold -0.0"""
    images = R.f32_set(3, 31, 33, 1, 320, False)
    refs = np.stack([np.full((9, 11, 1), -7.5, np.float32), np.where(np.arange(99).reshape(9, 11, 1) % 3 == 0, np.float32(-2.0),
                                                                    np.float32(5.0))])
    got = _run(dev, images, refs, [0, 1, 0])
    _check(got, R.expected(images, refs, [0, 1, 0]), "constant / two-level reference")
    assert np.all(got[0] == np.float32(-7.5)) and got[1].min() == np.float32(-2.0) and got[1].max() == np.float32(5.0)
    const, ref = np.full((1, 16, 16, 1), 3.25, dtype=np.float32), R.f32_set(1, 9, 9, 1, 330, True)
    got = _run(dev, const, ref, [0])
    _check(got, R.expected(const, ref, [0]), "constant image")
    assert np.all(got == ref.max()), "cnt = N, q = 1: the reference's maximum"
    zeros = np.where(np.arange(35).reshape(1, 7, 5, 1) % 2 == 0, np.float32(-0.0), np.float32(1.0)).astype(np.float32)
    _check(_run(dev, images, zeros, None), R.expected(images, zeros, [0, 0, 0]), "-0.0 in a reference")


def test_fp32_an_image_matched_to_itself_returns_its_own_bits(dev):
    from pointcloududa_amd.utils.histmatch import HistReferenceBank, match_histograms
    own = np.concatenate([G.normal_f32((1, 70, 61, 2), 340), G.levels_f32((1, 70, 61, 2), 341)])
    x = torch.from_numpy(own).to(dev)
    out = match_histograms(x, HistReferenceBank(x, check=True))                  # (a device tensor; index=None: R == B)
    assert torch.equal(out.view(torch.int32), x.view(torch.int32))
    keys = R.f32_set(3, 31, 33, 1, 342, True)                                   # with both zeros: equal as values
    _check(_run(dev, keys, keys, None), R.expected(keys, keys, [0, 1, 2]), "key coverage against itself")
    assert np.array_equal(_run(dev, keys, keys, None), keys)


def test_fp32_the_workload_plane(dev):
    """B = 2, R = 2, 256x256x3 on both sides"""
    images, refs = G.normal_f32((2, 256, 256, 3), 50, 100.0, 300.0), G.normal_f32((2, 256, 256, 3), 51, 0.0, 1.0)
    _check(_run(dev, images, refs, [1, 0]), R.expected(images, refs, [1, 0]), "workload plane")


# ---------------------------------------------------------------------------------------------- uint8
def _u8_inputs():
    images = np.concatenate([G.random_u8((1, 64, 48, 3), 400), G.random_u8((1, 64, 48, 3), 401, 90, 140), G.smooth_u8((1, 64, 48, 3), 402)])
    refs = np.concatenate([G.smooth_u8((1, 40, 56, 3), 403), G.random_u8((1, 40, 56, 3), 404), G.random_u8((1, 40, 56, 3), 405, 10, 60)])
    return images, refs


def test_uint8_against_the_count_bank(dev):
    """64x48x3 images (full range, narrow range, smooth) against 40x56x3 references; a constant reference and one using one
    value per channel; 1x1x1"""
    images, refs = _u8_inputs()
    for index in ([0, 1, 2], [2, 2, 0]):
        _check(_run(dev, images, refs, index), R.expected(images, refs, index), "uint8 %r" % (index,))
    special = np.stack([np.full((40, 56, 3), 200, np.uint8), np.broadcast_to(np.array([3, 128, 255], np.uint8), (40, 56, 3))])
    got = _run(dev, images, special, [0, 1, 1])
    _check(got, R.expected(images, special, [0, 1, 1]), "constant / one value per channel")
    assert np.all(got[0] == 200) and np.all(got[1:] == np.array([3, 128, 255], np.uint8))
    one = np.array([[[[17]]]], dtype=np.uint8)
    _check(_run(dev, one, one + 5, [0]), R.expected(one, one + 5, [0]), "1x1x1")


def test_fp32_images_against_a_uint8_bank_that_keeps_the_key_form(dev):
    images, refs = G.normal_f32((3, 40, 37, 3), 410, 100.0, 60.0), _u8_inputs()[1]
    got = _run(dev, images, refs, [2, 0, 1], float_images=True)
    _check(got, R.expected(images, refs.astype(np.float32), [2, 0, 1]), "fp32 images, uint8 bank")


# ---------------------------------------------------------------------------------------------- indexing
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_indexing(dev, kind):
    """R = 3, B = 5: repeats, a permutation, a bank of one, index=None with R == B, and a device index whose out-of-range
    entries clamp to 0 and R - 1"""
    from pointcloududa_amd.utils.histmatch import HistReferenceBank, match_histograms
    if kind == "f32":
        images, refs = R.f32_set(5, 23, 19, 2, 500, False), R.f32_set(3, 17, 29, 2, 510, True)
    else:
        images, refs = G.random_u8((5, 23, 19, 2), 520), G.smooth_u8((3, 17, 29, 2), 521)
    x, bank = torch.from_numpy(images).to(dev), HistReferenceBank(refs, dev)
    for index in ([0, 0, 2, 2, 1], [1, 1, 1, 1, 1], np.array([2, 0, 1, 0, 2], dtype=np.int64), (2, 1, 0, 1, 2)):
        _check(match_histograms(x, bank, index=index).cpu().numpy(), R.expected(images, refs, list(index)), "%s %r" % (kind, index))
    _check(match_histograms(x[:3], bank, index=[2, 0, 1]).cpu().numpy(), R.expected(images[:3], refs, [2, 0, 1]), "a permutation")
    _check(match_histograms(x[:3], bank).cpu().numpy(), R.expected(images[:3], refs, [0, 1, 2]), "index=None, R == B")
    one = HistReferenceBank(refs[1], dev)                                       # one [H,W,C] image: a bank of one
    assert one.size == 1 and one.shape == (1,) + refs.shape[1:]
    _check(match_histograms(x, one).cpu().numpy(), R.expected(images, refs[1:2], [0] * 5), "R = 1 broadcast")
    _check(match_histograms(x[4], one).cpu().numpy(), R.expected(images[4:5], refs[1:2], [0])[0], "a single [H,W,C] image")
    didx = torch.tensor([-5, 1, 3, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=dev)
    _check(match_histograms(x, bank, index=didx).cpu().numpy(), R.expected(images, refs, [0, 1, 2, 2, 0]), "clamped device index")
    with pytest.raises(ValueError, match="as many references"):
        match_histograms(x, bank)
    with pytest.raises(TypeError, match="int32"):
        match_histograms(x, bank, index=didx.long())


# ---------------------------------------------------------------------------------------------- against the old path
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_a_bank_of_one_equals_the_fixed_reference_path(dev, kind):
    from pointcloududa_amd.utils.histmatch import HistReference, HistReferenceBank, match_histograms
    if kind == "f32":
        images, ref = R.f32_set(3, 70, 90, 3, 600, False), R.f32_set(1, 48, 80, 3, 601, True)[0]
    else:
        images, ref = G.smooth_u8((3, 70, 90, 3), 602), G.random_u8((48, 80, 3), 603, 20, 230)
    x = torch.from_numpy(images).to(dev)
    old = match_histograms(x, HistReference(ref, dev))
    new = match_histograms(x, HistReferenceBank(ref, dev))
    assert torch.equal(old.view(torch.uint8), new.view(torch.uint8))
    _check(new.cpu().numpy(), G.match_unique(images, ref + (0 if kind == "u8" else np.float32(0.0))), "bank of one")


# ---------------------------------------------------------------------------------------------- contract
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_rebuild_refills_the_same_storage(dev, kind):
    from pointcloududa_amd.utils.histmatch import HistReferenceBank, match_histograms
    if kind == "f32":
        images, a, b = R.f32_set(2, 40, 50, 3, 700, False), R.f32_set(2, 33, 31, 3, 701, True), R.f32_set(2, 33, 31, 3, 702, True)
    else:
        images, a, b = G.random_u8((2, 40, 50, 3), 703), G.smooth_u8((2, 33, 31, 3), 704), G.random_u8((2, 33, 31, 3), 705, 0, 50)
    x, ta, tb = (torch.from_numpy(v).to(dev) for v in (images, a, b))
    bank = HistReferenceBank(ta)
    first = match_histograms(x, bank).cpu().numpy()
    ptr, before = bank.bank.data_ptr(), torch.cuda.memory_allocated(dev)
    assert bank.rebuild(tb) is bank
    assert bank.bank.data_ptr() == ptr and torch.cuda.memory_allocated(dev) == before, "a rebuild allocates nothing"
    second = match_histograms(x, bank)
    _check(first, R.expected(images, a, [0, 1]), "before the rebuild")
    _check(second.cpu().numpy(), R.expected(images, b, [0, 1]), "after the rebuild")
    assert torch.equal(second.view(torch.uint8), match_histograms(x, bank).view(torch.uint8)), "two calls give identical bits"
    with pytest.raises(ValueError, match="shape"):
        bank.rebuild(tb[:1])
    bank.rebuild(a)                                                             # (numpy references: staged through the bank's own copy)
    _check(match_histograms(x, bank).cpu().numpy(), first, "rebuilt from numpy")


def test_two_builds_and_two_calls_give_identical_bits(dev):
    from pointcloududa_amd.utils.histmatch import HistReferenceBank, match_histograms
    images, refs = R.f32_set(3, 70, 90, 2, 710, False), R.f32_set(3, 60, 70, 2, 711, True)
    x = torch.from_numpy(images).to(dev)
    b1, b2 = HistReferenceBank(refs, dev), HistReferenceBank(refs, dev)
    assert torch.equal(b1.bank, b2.bank)
    o1, o2, o3 = match_histograms(x, b1), match_histograms(x, b1), match_histograms(x, b2)
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(o1.view(torch.int32), o3.view(torch.int32))
    keys = b1.bank.view(torch.int32).view(3 * 2, -1)[:, :60 * 70].cpu().numpy().view(np.uint32)
    want = np.stack([np.sort(R.float_key(refs[r, ..., c].ravel())) for r in range(3) for c in range(2)])
    assert np.array_equal(keys, want), "the fp32 bank is every plane's sorted keys, 4 bytes per value"


def test_a_non_finite_reference_raises_when_checked(dev):
    from pointcloududa_amd.utils.histmatch import HistReferenceBank
    refs = R.f32_set(2, 70, 70, 2, 720, True)
    good = HistReferenceBank(refs, dev, check=True)
    assert int(good.flag.item()) == 0
    for bad in (np.nan, np.inf, -np.inf):
        r = refs.copy()
        r[1, 69, 3, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            HistReferenceBank(r, dev, check=True)
        assert int(HistReferenceBank(r, dev).flag.item()) == 1, "the default leaves the flag on the device"
        with pytest.raises(ValueError, match="finite"):
            good.rebuild(r, check=True)
    assert int(good.rebuild(refs, check=True).flag.item()) == 0, "a rebuild clears the flag"


def test_the_bank_path_adds_no_host_synchronisation(dev):
    """build, rebuild, match (fp32 and uint8; host, device and default indices) and augment_batch under
    torch.cuda.set_sync_debug_mode("error"); the mode is first shown to be enforced (a ``.item()`` raises under it)"""
    from pointcloududa_amd.utils.augment import HistReferenceBank, augment_batch, match_histograms, sample_params
    images, refs = G.normal_f32((3, 64, 64, 3), 730, 200.0, 400.0), G.normal_f32((3, 48, 80, 3), 731)   # (max - min stays finite)
    q, refq = _u8_inputs()
    lab = torch.from_numpy(np.random.default_rng(5).integers(0, 5, (3, 64, 64))).to(dev)
    tx, tr, tq, trq = (torch.from_numpy(v).to(dev) for v in (images, refs, q, refq))
    didx = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev)
    params = sample_params(3, "mmwhs_light", np.random.default_rng(3))
    bank, bank8 = HistReferenceBank(tr), HistReferenceBank(trq)                # (warm: allocator, library load)
    want = (match_histograms(tx, bank, index=[2, 0, 1]), match_histograms(tq, bank8),
            augment_batch(tx, lab, params, 5, 48, rescale="minmax", match_hist=bank, match_hist_index=didx))
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        fresh = HistReferenceBank(tr)
        bank.rebuild(tr), bank8.rebuild(trq)
        got = (match_histograms(tx, fresh, index=[2, 0, 1]), match_histograms(tq, bank8),
               augment_batch(tx, lab, params, 5, 48, rescale="minmax", match_hist=bank, match_hist_index=didx))
        dev_idx = match_histograms(tx, bank, index=didx)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(dev_idx, want[0])
    assert torch.equal(got[2][0], want[2][0]) and torch.equal(got[2][1], want[2][1])


def test_entry_points_return_status_codes(dev):
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    b, h, w, c, r, rh, rw = 2, 24, 40, 3, 2, 10, 13
    images, refs = G.normal_f32((b, h, w, c), 60), G.normal_f32((r, rh, rw, c), 61)
    x, t = torch.from_numpy(images).to(dev), torch.from_numpy(refs).to(dev)
    out = torch.full_like(x, 7.0)
    stream = torch.cuda.current_stream().cuda_stream
    size, bws = lib.pcuda_hist_bank_size(r, rh, rw, c, 0), lib.pcuda_hist_bank_workspace_size(r, rh, rw, c, 0)
    assert size == bws == (4 * r * rh * rw * c + 15) // 16 * 16
    bank = torch.full((size + 16,), 9, dtype=torch.uint8, device=dev)
    bw = torch.empty(bws + 16, dtype=torch.uint8, device=dev)
    flag = torch.full((1,), 5, dtype=torch.int32, device=dev)

    def build(refs=t.data_ptr(), u8=0, r=r, rh=rh, rw=rw, c=c, bank=bank.data_ptr(), nbank=size, flag=flag.data_ptr(),
              ws=bw.data_ptr(), nws=bws):
        return lib.pcuda_hist_bank_build(refs, u8, r, rh, rw, c, bank, nbank, flag, ws, nws, stream)
    for kw in (dict(refs=None), dict(bank=None), dict(flag=None), dict(r=-1), dict(rh=-1), dict(c=0), dict(c=5), dict(rw=32769),
               dict(refs=bank.data_ptr())):
        assert build(**kw) == -1, kw
    assert build(nbank=size - 1) == -4 and b"bank" in lib.pcuda_last_error()
    assert build(bank=bank.data_ptr() + 4) == -4
    assert build(nws=bws - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert build(ws=None) == -4 and build(ws=bw.data_ptr() + 8) == -4
    assert build(r=0) == 0 and build(rh=0, refs=None, bank=None, flag=None, ws=None) == 0, "an empty set is a no-op"
    torch.cuda.synchronize()
    assert bool((bank == 9).all()) and int(flag.item()) == 5, "a rejected call and a no-op launch nothing"
    assert build() == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and bool((bank[size:] == 9).all())

    need = lib.pcuda_match_hist_bank_workspace_size(b, h, w, c, 0)
    assert need >= 8 * b * h * w * c and need % 16 == 0
    assert lib.pcuda_match_hist_bank_workspace_size(0, h, w, c, 0) == 0 and lib.pcuda_match_hist_bank_workspace_size(b, h, w, c, 1) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    idx = torch.tensor([1, 0], dtype=torch.int32, device=dev)

    def call(inp=x.data_ptr(), outp=out.data_ptr(), u8=0, b=b, h=h, w=w, c=c, bank=bank.data_ptr(), r=r, rh=rh, rw=rw,
             idx=idx.data_ptr(), wsp=ws.data_ptr(), nbytes=need):
        return lib.pcuda_match_hist_bank(inp, outp, u8, b, h, w, c, bank, r, rh, rw, idx, wsp, nbytes, stream)
    assert call(outp=x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    for kw in (dict(inp=None), dict(outp=None), dict(b=-1), dict(h=-1), dict(c=0), dict(c=5), dict(bank=None), dict(idx=None),
               dict(r=0), dict(rh=0), dict(rw=-1), dict(r=-1)):
        assert call(**kw) == -1, kw
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(wsp=None) == -4 and call(wsp=ws.data_ptr() + 4) == -4 and call(bank=bank.data_ptr() + 8) == -4
    assert call(b=0) == 0 and call(h=0) == 0 and call(w=0, inp=None, outp=None, wsp=None, nbytes=0) == 0, "b h w == 0 is a no-op"
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a rejected call and a no-op launch nothing"
    assert call() == 0
    torch.cuda.synchronize()
    _check(out.cpu().numpy(), R.expected(images, refs, [1, 0]), "C ABI call")


def test_the_kernel_wrappers_check_their_arguments(dev):
    from pointcloududa_amd import kernels as K
    refs = torch.from_numpy(G.normal_f32((2, 10, 10, 2), 61)).to(dev)
    bank, ws, flag = K.hist_bank_build(refs)
    x = torch.zeros((2, 8, 8, 3), device=dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="channels"):
        K.match_hist_bank(x, bank, refs.shape, idx)
    with pytest.raises(ValueError, match="ref_index"):
        K.match_hist_bank(x[..., :2].contiguous(), bank, refs.shape, idx[:1])
    with pytest.raises(ValueError, match="smaller"):
        K.match_hist_bank(x[..., :2].contiguous(), bank, (4, 10, 10, 2), idx)
    with pytest.raises(TypeError):
        K.match_hist_bank(x[..., :2].contiguous(), bank, refs.shape, idx.long())
    with pytest.raises(TypeError):
        K.hist_bank_build(refs.double())
    with pytest.raises(TypeError, match="contiguous"):
        K.hist_bank_build(refs[:, ::2])


# ---------------------------------------------------------------------------------------------- integration
def _batch(dev, dtype, b=3, h=64, w=64, c=3, seed=80):
    rng = np.random.default_rng(seed)
    img = G.normal_f32((b, h, w, c), seed, 200.0, 400.0) if dtype == np.float32 else G.smooth_u8((b, h, w, c), seed)
    lab = rng.integers(0, 5, (b, h, w)).astype(np.int64)
    refs = G.normal_f32((4, 48, 80, c), seed + 1, 0.0, 1.0) if dtype == np.float32 else G.random_u8((4, 48, 80, c), seed + 1, 20, 230)
    return img, lab, refs, torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_augment_batch_with_a_bank_is_assemble_batch_of_the_matched_images(dev, dtype):
    from pointcloududa_amd.utils.augment import HistReferenceBank, augment_batch, match_histograms
    from pointcloududa_amd.utils.batch import assemble_batch
    img, lab, refs, tx, tl = _batch(dev, dtype)
    bank, idx = HistReferenceBank(refs, dev), [3, 0, 3]
    got = augment_batch(tx, tl, None, 5, 48, rescale=None, match_hist=bank, match_hist_index=idx)
    matched = match_histograms(tx, bank, index=idx)
    # (assemble_batch takes fp32 images; the uint8 batch goes through the assembler without a match instead)
    want = assemble_batch(matched, tl, 5, 48) if dtype == np.float32 else augment_batch(matched, tl, None, 5, 48, rescale=None)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] is None and want[2] is None
    _check(matched.cpu().numpy(), R.expected(img, refs, idx), "matched batch")
    plain = augment_batch(tx, tl, None, 5, 48, rescale=None)
    assert torch.equal(plain[1], got[1]) and not torch.equal(plain[0], got[0]), "masks are untouched, images are not"


def test_augmented_batches_with_a_bank_yield_the_manual_sequence(dev):
    from pointcloududa_amd.utils.augment import AugmentedBatches, HistReferenceBank, augment_batch, sample_params
    raw, refs = [], None
    for i in range(2):
        img, lab, refs, _, _ = _batch(dev, np.float32, seed=90 + 2 * i)
        raw.append((img, lab[..., None]))
    bank = HistReferenceBank(refs, dev)
    it = AugmentedBatches(iter(raw), dev, "mmwhs_light", np.random.default_rng(77), num_classes=5, crop_size=48, rescale="minmax",
                          resample_verts=False, match_hist_bank=bank)
    twin, n = np.random.default_rng(77), 0
    for (x, y, z), (img, lab) in zip(it, raw):
        idx = twin.integers(4, size=3)
        assert np.array_equal(it.last_match_index, idx)
        want = augment_batch(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), sample_params(3, "mmwhs_light", twin), 5, 48,
                             "minmax", match_hist=bank, match_hist_index=idx)
        assert torch.equal(x, want[0]) and torch.equal(y, want[1]) and z is None and bool(torch.isfinite(x).all())
        n += 1
    assert n == 2
