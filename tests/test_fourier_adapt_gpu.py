"""GPU checks of Fourier domain adaptation (pointcloududa_amd/utils/fourier.py, csrc/fourier.hip)
against the full-FFT definition in numpy float64 (tests/fourier_refs.py) on the ten cases of fourier_refs.CASES.

fp32: ``|out - ref| <= 2^-24 |ref| + 1e-9`` on every pixel.  The output is ONE float32 rounding of a float64 value (half an ulp:
2^-24 relative) and that float64 value may differ from the reference's by summation order only; 1e-9 is about 500 times the
1.8e-12 measured between two float64 algorithms on these inputs and two orders below an fp32 ulp at 1.0.
uint8: equal to ``uint8(clip(rint(ref), 0, 255))`` on EVERY pixel; the test first asserts on the reference alone that no value lies
within 1e-8 of a half-integer and that every block bin of the source has ``|S| >= 1`` (smallest tie distance 1.0e-6 at case 7,
smallest ``|S|`` 76: tests/test_fourier_adapt.py prints both)."""
import numpy as np
import pytest
import torch

import fourier_refs as R

pytestmark = pytest.mark.gpu


def _mods():
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import fourier as F
    return K, A, F


def _same(got, want, what):
    got, want = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (got, want))
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = (a.view(np.uint32) if a.dtype == np.float32 else a for a in (got, want))
    bad = g != w
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _within_f32(got, ref, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    excess = np.abs(got.astype(np.float64) - ref) - (2.0 ** -24 * np.abs(ref) + 1e-9)
    print("%s: max (|out - ref| - bound) = %.3g, max |out - ref| = %.3g" % (what, excess.max(), np.abs(got - ref).max()))
    assert excess.max() <= 0.0, (what, int((excess > 0).sum()), float(excess.max()))


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_fp32_within_one_rounding_of_the_full_fft_definition(dev, i):
    _, _, F = _mods()
    src, refs, ref = R.case_reference(i)
    b = R.CASES[i][4]
    x = torch.from_numpy(src.astype(np.float32)).to(dev)
    bank = F.FourierBank(refs.astype(np.float32), dev, radius=b)
    assert (bank.size, bank.radius, bank.shape) == (refs.shape[0], b, refs.shape)
    out = F.fourier_adapt(x, bank)
    _within_f32(out, ref, "case %d %r" % (i, R.CASES[i]))
    _same(F.fourier_adapt(x, bank), out, "two runs")
    _same(F.FourierBank(torch.from_numpy(refs.astype(np.float32)).to(dev), radius=b).bank, bank.bank, "two builds")


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_uint8_equals_the_rounded_definition_on_every_pixel(dev, i):
    _, _, F = _mods()
    src, refs, ref = R.case_reference(i)
    b = R.CASES[i][4]
    tie = float(np.abs(ref - np.floor(ref) - 0.5).min())
    amp = R.block_min_amplitude(src, b)
    print("case %d: smallest tie distance %.3g, smallest |S| %.4g" % (i, tie, amp))
    assert tie >= 1e-8 and amp >= 1.0, "the reference alone decides every pixel"
    x = torch.from_numpy(src).to(dev)
    bank = F.FourierBank(refs, dev, radius=b)
    out = F.fourier_adapt(x, bank)
    _same(out, R.to_u8(ref), "case %d %r" % (i, R.CASES[i]))
    _same(F.fourier_adapt(x, bank), out, "two runs")
    _same(x, src, "the input is never written")


def _setup(dev, i, dtype):
    _, _, F = _mods()
    src, refs, _ = R.case_reference(i)
    x = torch.from_numpy(src.astype(dtype)).to(dev)
    return F, src, refs, x, F.FourierBank(refs.astype(dtype), dev, radius=R.CASES[i][4])


@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("f32", "u8"))
def test_index_rules_pass_through_clamp_and_per_sample_radii(dev, dtype):
    F, src, refs, x, bank = _setup(dev, 5, dtype)                       # (2, 70, 130, 4, 7)
    x3 = torch.cat([x, x[:1]])
    if dtype == np.float32:
        x3[1, 0, :4, 0] = torch.tensor([-0.0, 1e-42, 3.4e38, -7.25], device=dev)   # bits a recomputation would not keep
    src3 = x3.cpu().numpy()
    # a negative index returns the input's bits; host and device indices agree
    out = F.fourier_adapt(x3, bank, index=[1, -1, 0])
    _same(out[1], x3[1], "index -1 passes the sample through")
    dev_idx = torch.tensor([1, -5, 0], dtype=torch.int32, device=dev)
    _same(F.fourier_adapt(x3, bank, index=dev_idx), out, "a device index, any negative entry")
    want = R.adapt_batch(src3, refs, 7, [1, -1, 0])
    if dtype == np.float32:
        _within_f32(out[[0, 2]], want[[0, 2]], "index [1, -1, 0]")
    else:
        _same(out, R.to_u8(want), "index [1, -1, 0]")
    # an index >= R is clamped on the device
    big = torch.tensor([7, 1, 2], dtype=torch.int32, device=dev)
    _same(F.fourier_adapt(x3, bank, index=big), F.fourier_adapt(x3, bank, index=[1, 1, 1]), "index >= R is clamped")
    # per-sample radii: 0, one inside, one above the bank's (clamped)
    rad = [0, 3, 40]
    out = F.fourier_adapt(x3, bank, index=[0, 1, 1], radius=rad)
    want = R.adapt_batch(src3, refs, 7, [0, 1, 1], rad)
    if dtype == np.float32:
        _within_f32(out[[0, 2]], want[[0, 2]], "radii [0, 3, 40]")     # (sample 1 holds the odd bit patterns)
        x3[1] = x3[0]
        out = F.fourier_adapt(x3, bank, index=[0, 1, 1], radius=rad)
        _within_f32(out, R.adapt_batch(x3.cpu().numpy(), refs, 7, [0, 1, 1], rad), "radii [0, 3, 40], plain values")
    else:
        _same(out, R.to_u8(want), "radii [0, 3, 40]")
    dev_rad = torch.tensor([0, 3, 40], dtype=torch.int32, device=dev)
    _same(F.fourier_adapt(x3, bank, index=[0, 1, 1], radius=dev_rad), out, "device radii")
    _same(F.fourier_adapt(x3, bank, index=[0, 1, 1], radius=-3 + dev_rad), F.fourier_adapt(x3, bank, index=[0, 1, 1], radius=[0, 0, 7]),
          "device radii are clamped into [0, radius]")
    _same(F.fourier_adapt(x3, bank, index=[0, 1, 1], radius=3), F.fourier_adapt(x3, bank, index=[0, 1, 1], radius=[3, 3, 3]), "an int radius")
    _same(F.fourier_adapt(x3, bank, index=[0, 1, 1], radius=9), F.fourier_adapt(x3, bank, index=[0, 1, 1]), "an int above the bank's")
    # radius 0 moves every pixel of a plane by the same amount
    z = F.fourier_adapt(x3[:1], bank, index=[1], radius=0)
    if dtype == np.float32:
        s, t = src3[0].astype(np.float64), refs[1].astype(np.float64)
        shift = (t.mean(axis=(0, 1)) - s.mean(axis=(0, 1))) * np.sign(s.sum(axis=(0, 1)))
        _within_f32(z[0], s + shift, "radius 0 is the DC swap")
    # one [H,W,C] image against a bank of one
    one = F.FourierBank(refs[1].astype(dtype), dev, radius=7)
    assert one.size == 1 and one.shape == (1,) + refs.shape[1:]
    _same(F.fourier_adapt(x3[0], one), F.fourier_adapt(x3[:1], bank, index=[1])[0], "one image, a bank of one")


def test_clip_on_fp32(dev):
    F, src, refs, x, bank = _setup(dev, 4, np.float32)                   # (2, 33, 64, 3, 2)
    ref = R.case_reference(4)[2]
    assert ref.min() < 0.0 and ref.max() > 255.0, "the case leaves 0..255, so the clip acts"
    _within_f32(F.fourier_adapt(x, bank, clip=(0, 255)), np.clip(ref, 0.0, 255.0), "clip (0, 255)")
    _within_f32(F.fourier_adapt(x, bank, clip=(50.5, 60.25)), np.clip(ref, 50.5, 60.25), "clip (50.5, 60.25)")
    out = F.fourier_adapt(x, bank)
    assert float(out.min()) < 0.0 and float(out.max()) > 255.0, "without clip the range is not clipped"


@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("f32", "u8"))
def test_misaligned_views_and_out(dev, dtype):
    K, _, F = _mods()
    _, src, refs, x, bank = _setup(dev, 3, dtype)                       # (3, 17, 23, 2, 1)
    want = F.fourier_adapt(x, bank)
    buf_in = torch.zeros(x.numel() + 1, dtype=x.dtype, device=dev)
    buf_out = torch.full((x.numel() + 2,), 77, dtype=x.dtype, device=dev)
    xin = buf_in[1:].view(x.shape)
    xin.copy_(x)
    xout = buf_out[1:-1].view(x.shape)
    assert xin.data_ptr() % 16 != 0 and xout.data_ptr() % 16 != 0
    got = F.fourier_adapt(xin, bank, out=xout)
    assert got.data_ptr() == xout.data_ptr()
    _same(xout, want, "one element into both allocations")
    assert buf_out[0].item() == 77 and buf_out[-1].item() == 77, "nothing is written around out"
    idx = torch.arange(3, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        K.fourier_adapt(x, bank.bank, bank.size, bank.radius, idx, out=torch.empty_like(x).transpose(1, 2))
    with pytest.raises(RuntimeError, match="in == out"):
        K.fourier_adapt(x, bank.bank, bank.size, bank.radius, idx, out=x)
    refs_mis = torch.zeros(x.numel() + 1, dtype=x.dtype, device=dev)[1:].view(x.shape)
    refs_mis.copy_(torch.from_numpy(refs.astype(dtype)))
    _same(F.FourierBank(refs_mis, radius=1).bank, bank.bank, "references one element into their allocation")


@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("f32", "u8"))
def test_rebuild_from_a_device_tensor_gives_a_fresh_banks_bits(dev, dtype):
    F, src, refs, x, bank = _setup(dev, 4, dtype)
    other = F.FourierBank(np.ascontiguousarray(refs[::-1]).astype(dtype), dev, radius=2)
    assert not torch.equal(other.bank, bank.bank)
    ptr = other.bank.data_ptr()
    assert other.rebuild(torch.from_numpy(refs.astype(dtype)).to(dev)) is other and other.bank.data_ptr() == ptr
    _same(other.bank, bank.bank, "rebuilt in place")
    _same(F.fourier_adapt(x, other), F.fourier_adapt(x, bank), "and adapts alike")
    with pytest.raises(ValueError, match="rebuild"):
        other.rebuild(refs[:1].astype(dtype))
    with pytest.raises(ValueError, match="rebuild"):
        other.rebuild(refs.astype(np.uint8 if dtype == np.float32 else np.float32))
    # this step's target batch as the bank: the source batch adapted to itself comes back
    self_bank = F.FourierBank(x, radius=2)
    got = F.fourier_adapt(x, self_bank)
    if dtype == np.uint8:
        _same(got, x, "target == source")
    else:
        _within_f32(got, src.astype(np.float64), "target == source")


@pytest.mark.parametrize("rescale,dtype", (("minmax", np.float32), ("div255", np.uint8), (None, np.float32)))
def test_augment_batch_runs_the_stage_first_and_is_unchanged_without_it(dev, rescale, dtype):
    _, A, F = _mods()
    _, src, refs, x, bank = _setup(dev, 4, dtype)                       # (2, 33, 64, 3, 2)
    rng = np.random.default_rng(3)
    masks = torch.from_numpy(rng.integers(0, 5, (2, 33, 64))).to(dev)
    params = A.sample_params(2, "mmwhs_light", np.random.default_rng(4))
    kw = dict(num_classes=5, crop_size=0, rescale=rescale, resample_verts=False)
    idx, rad = [1, 0], [2, 1]
    fused = A.augment_batch(x, masks, params, fourier=bank, fourier_index=idx, fourier_radius=rad, **kw)
    staged = A.augment_batch(F.fourier_adapt(x, bank, index=idx, radius=rad), masks, params, **kw)
    plain = A.augment_batch(x, masks, params, **kw)
    again = A.augment_batch(x, masks, params, fourier=None, **kw)
    for k in range(2):
        _same(fused[k], staged[k], "fourier= is fourier_adapt in front of augment_batch")
        _same(again[k], plain[k], "fourier=None is the call without it")
    assert not torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1]), "images change, masks do not"
    skipped = A.augment_batch(x, masks, params, fourier=bank, fourier_index=[-1, -1], **kw)
    _same(skipped[0], plain[0], "every sample passed through")


def test_the_stage_adds_no_host_synchronisation(dev):
    """rebuild and adapt (host, device and default indices and radii) under torch.cuda.set_sync_debug_mode("error"); the mode
    is first shown to be enforced (a ``.item()`` raises under it)"""
    F, src, refs, x, bank = _setup(dev, 4, np.float32)
    tr = torch.from_numpy(refs.astype(np.float32)).to(dev)
    didx = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    drad = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    want = (F.fourier_adapt(x, bank), F.fourier_adapt(x, bank, index=[1, 0], radius=[1, 2]))        # (warm: allocator, code load)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        bank.rebuild(tr)
        got = (F.fourier_adapt(x, bank), F.fourier_adapt(x, bank, index=[1, 0], radius=[1, 2]))
        dev_idx = F.fourier_adapt(x, bank, index=didx, radius=drad)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _same(got[0], want[0], "default index")
    _same(got[1], want[1], "host index and radii")
    _same(dev_idx, want[1], "device index and radii")


def test_augmented_batches_with_a_bank_yield_the_manual_sequence(dev):
    _, A, F = _mods()
    rng = np.random.default_rng(21)
    raw = [(rng.integers(0, 256, (3, 40, 48, 3)).astype(np.float32), rng.integers(0, 5, (3, 40, 48, 1))) for _ in range(2)]
    bank = F.FourierBank(rng.integers(0, 256, (4, 40, 48, 3)).astype(np.float32), dev, radius=4)
    kw = dict(num_classes=5, crop_size=0, rescale="minmax", resample_verts=False)
    it = A.AugmentedBatches(iter(raw), dev, "mmwhs_light", np.random.default_rng(77), fourier_bank=bank, fourier_p=0.6,
                            fourier_radius_range=(0, 4), **kw)
    twin, n = np.random.default_rng(77), 0
    for (x, y, z), (img, lab) in zip(it, raw):
        idx = twin.integers(4, size=3)
        idx = np.where(twin.random(3) >= 0.6, -1, idx)
        rad = twin.integers(0, 5, size=3)
        assert np.array_equal(it.last_fourier_index, idx) and np.array_equal(it.last_fourier_radius, rad)
        adapted = F.fourier_adapt(torch.from_numpy(img).to(dev), bank, index=idx, radius=rad)
        want = A.augment_batch(adapted, torch.from_numpy(lab).to(dev), A.sample_params(3, "mmwhs_light", twin), **kw)
        _same(x, want[0], "images")
        _same(y, want[1], "one-hot masks")
        assert z is None and bool(torch.isfinite(x).all())
        n += 1
    assert n == 2
