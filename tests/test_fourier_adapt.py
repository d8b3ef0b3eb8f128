"""CPU checks of Fourier domain adaptation (pointcloududa_amd/utils/fourier.py, csrc/fourier.hip):
the low-rank form the kernels compute against the full-FFT definition (tests/fourier_refs.py) on every input the GPU tests use;
three anchors that hold by the definition; ``fourier_radius``; the index rules; the loader's use of the generator; the
rejections of the wrappers and of the entry points; the C declarations against the binding.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import fourier_refs as R
from conftest import ROOT


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_the_low_rank_form_equals_the_full_fft_definition(i):
    src, refs, ref = R.case_reference(i)
    low = R.adapt_batch(src, refs, R.CASES[i][4], fn=R.adapt_plane_lowrank)
    err = float(np.abs(low - ref).max())
    print("case %d %r: max |low-rank - full FFT| = %.3g" % (i, R.CASES[i], err))
    assert err <= 1e-9


@pytest.mark.parametrize("fn", (R.adapt_plane_fft, R.adapt_plane_lowrank), ids=("fft", "lowrank"))
def test_three_anchors_hold_by_the_definition(fn):
    rng = np.random.default_rng(5)
    for h, w, b in ((9, 12, 3), (16, 16, 0), (33, 20, 9), (7, 7, 3)):
        s = rng.integers(0, 256, (h, w)).astype(np.float64)
        t = rng.integers(0, 256, (h, w)).astype(np.float64)
        # the target's own amplitudes change nothing
        assert np.abs(fn(s, s, b) - s).max() <= 1e-9
        # b = 0 swaps the DC bin: |sum(t)| takes the sign of sum(s), every pixel moves by the same amount
        shift = (t.mean() - s.mean()) * np.sign(s.sum())
        assert np.abs(fn(s, t, 0) - (s + shift)).max() <= 1e-9
        # an all-zero source has phase 0 everywhere: the inverse transform of |T| on the block
        T = np.fft.fft2(t)
        keep = np.zeros((h, w))
        keep[np.ix_(R.block_index(h, b), R.block_index(w, b))] = 1.0
        want = np.real(np.fft.ifft2(np.abs(T) * keep))
        assert np.abs(fn(np.zeros((h, w)), t, b) - want).max() <= 1e-9
    # signed DC: a source whose sum is negative keeps its sign
    s = -np.ones((4, 4)); t = np.full((4, 4), 3.0)
    assert np.abs(fn(s, t, 0) + 3.0).max() <= 1e-9


def test_the_uint8_cases_have_no_tie_and_no_vanishing_bin():
    """what makes 'equal on every pixel' a fair demand of the GPU tests: measured here, asserted there again"""
    for i, (_, _, _, _, b) in enumerate(R.CASES):
        src, _, ref = R.case_reference(i)
        tie = float(np.abs(ref - np.floor(ref) - 0.5).min())
        amp = R.block_min_amplitude(src, b)
        print("case %d: smallest tie distance %.3g, smallest |S| %.4g" % (i, tie, amp))
        assert tie >= 1e-8 and amp >= 1.0


# ---------------------------------------------------------------------------------------------- the host side
def test_fourier_radius():
    from pointcloududa_amd.utils.fourier import check_radius, fourier_radius
    assert fourier_radius(256, 256, 0.01) == 2 and fourier_radius(256, 256, 0.05) == 12 and fourier_radius(256, 256, 0.1) == 25
    assert fourier_radius(224, 224, 0.1) == 22 and fourier_radius(224, 300, 0.01) == 2 and fourier_radius(50, 50, 0.01) == 0
    assert fourier_radius(1, 1, 0.0) == 0
    for bad in (-0.1, 0.5, 1.0, float("nan")):
        with pytest.raises(ValueError, match="beta"):
            fourier_radius(64, 64, bad)
    with pytest.raises(ValueError, match="sides"):
        fourier_radius(0, 64, 0.1)
    assert check_radius("t", 32, 65, 65) == 32 and check_radius("t", np.int64(0), 1, 1) == 0
    with pytest.raises(ValueError, match="alias"):
        check_radius("t", 32, 64, 65)
    with pytest.raises(ValueError, match=r"\[0, 32\]"):
        check_radius("t", 33, 256, 256)
    with pytest.raises(ValueError, match=r"\[0, 32\]"):
        check_radius("t", -1, 256, 256)
    with pytest.raises(TypeError, match="integer"):
        check_radius("t", 2.0, 256, 256)


def test_index_and_radius_validation_allows_minus_one():
    import torch
    from pointcloududa_amd.utils import fourier as F
    assert F.validate_index((2, -1, 0), 3, 3).tolist() == [2, -1, 0] and F.validate_index((2, -1, 0), 3, 3).dtype == np.int32
    assert F.validate_index(torch.tensor([0, 1]), 2, 2).tolist() == [0, 1]
    with pytest.raises(ValueError, match=r"\[-1, 3\)"):
        F.validate_index((2, -2, 0), 3, 3)
    with pytest.raises(ValueError, match=r"\[-1, 3\)"):
        F.validate_index((3, 0, 0), 3, 3)
    with pytest.raises(ValueError, match="one entry per sample"):
        F.validate_index((0, 0), 3, 3)
    with pytest.raises(TypeError, match="integers"):
        F.validate_index((0.0, 1.0, 2.0), 3, 3)
    assert F.validate_radius((0, 40, 3), 3, 12).tolist() == [0, 12, 3]          # above the bank's: clamped
    with pytest.raises(ValueError, match="non-negative"):
        F.validate_radius((0, -1, 3), 3, 12)
    with pytest.raises(ValueError, match="one entry per sample"):
        F.validate_radius((0, 1), 3, 12)


class _Bank:
    """a FourierBank without its device side: what the host-side validation reads"""

    def __new__(cls, size, shape_hwc, dtype, radius):
        import torch
        from pointcloududa_amd.utils.fourier import FourierBank
        bank = object.__new__(FourierBank)
        bank.size, bank.channels, bank.dtype, bank.shape = size, shape_hwc[2], np.dtype(dtype), (size,) + tuple(shape_hwc)
        bank.radius, bank.device, bank._index_cache = radius, torch.device("cpu"), {}
        bank.bank = torch.zeros(size * shape_hwc[2] * (2 * radius + 1) * (radius + 1) * 8, dtype=torch.uint8)
        return bank


def test_the_wrappers_reject_on_the_host():
    import torch
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import fourier as F
    assert A.FourierBank is F.FourierBank and A.fourier_adapt is F.fourier_adapt
    for bad in (np.zeros((2, 8, 8, 3), np.float64), np.zeros((2, 8, 8, 3), np.int16), torch.zeros((2, 8, 8, 3), dtype=torch.float16)):
        with pytest.raises(TypeError, match="fp32 or uint8"):
            F.FourierBank(bad, "cpu", radius=1)
    with pytest.raises(ValueError, match="dimensions"):
        F.FourierBank(np.zeros((8, 8), np.float32), "cpu", radius=1)
    with pytest.raises(ValueError, match="1..4 channels"):
        F.FourierBank(np.zeros((2, 8, 8, 5), np.float32), "cpu", radius=1)
    with pytest.raises(ValueError, match="alias"):                              # 2 b + 1 > min(H, W)
        F.FourierBank(np.zeros((2, 8, 6, 3), np.float32), "cpu", radius=3)
    with pytest.raises(ValueError, match=r"\[0, 32\]"):                         # radius > 32
        F.FourierBank(np.zeros((1, 128, 128, 1), np.uint8), "cpu", radius=33)
    with pytest.raises(ValueError, match="beta"):
        F.FourierBank(np.zeros((1, 16, 16, 1), np.uint8), "cpu", beta=0.7)

    f32, u8 = _Bank(4, (8, 8, 3), np.float32, 2), _Bank(4, (8, 8, 3), np.uint8, 2)
    x = torch.zeros((5, 8, 8, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match="FourierBank"):
        F.fourier_adapt(x, np.zeros((4, 8, 8, 3), np.float32))
    with pytest.raises(TypeError, match="dtypes must match"):
        F.fourier_adapt(x, u8, index=[0] * 5)
    with pytest.raises(TypeError, match="dtypes must match"):
        F.fourier_adapt(x.to(torch.uint8), f32, index=[0] * 5)
    with pytest.raises(TypeError, match="fp32 or uint8"):
        F.fourier_adapt(x.double(), f32, index=[0] * 5)
    for shape in ((5, 8, 9, 3), (5, 9, 8, 3), (5, 8, 8, 2)):
        with pytest.raises(ValueError, match="must match"):
            F.fourier_adapt(torch.zeros(shape), f32, index=[0] * 5)
    with pytest.raises(ValueError, match="dimensions"):
        F.fourier_adapt(torch.zeros((8, 8)), f32)
    for bad in ((1.0,), (2.0, 1.0), (0.0, float("inf")), 3.0):
        with pytest.raises(ValueError, match="clip"):
            F.fourier_adapt(x, f32, index=[0] * 5, clip=bad)
    with pytest.raises(TypeError, match="clip goes with fp32"):
        F.fourier_adapt(x.to(torch.uint8), u8, index=[0] * 5, clip=(0, 255))
    with pytest.raises(ValueError, match="index=None"):
        F.fourier_adapt(x, f32)
    with pytest.raises(ValueError, match=r"\[-1, 4\)"):
        F.fourier_adapt(x, f32, index=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="non-negative"):
        F.fourier_adapt(x, f32, index=[0] * 5, radius=[0, 1, 2, -1, 0])
    with pytest.raises(TypeError, match="go with fourier"):
        A.augment_batch(x, torch.zeros((5, 8, 8), dtype=torch.int64), None, fourier_index=[0] * 5)
    with pytest.raises(RuntimeError, match="HIP device"):                       # valid arguments reach the kernel wrapper
        F.fourier_adapt(x, f32, index=[0, -1, 2, 1, 0], radius=[0, 1, 2, 5, 0], clip=(0.0, 255.0))


# ---------------------------------------------------------------------------------------------- the loader
def _raw(n=2, b=3):
    rng = np.random.default_rng(1)
    return [(rng.standard_normal((b, 16, 16, 3)).astype(np.float32), rng.integers(0, 5, (b, 16, 16, 1))) for _ in range(n)]


def test_augmented_batches_draw_order_with_a_bank_and_nothing_without(monkeypatch):
    import torch
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils.histmatch import HistReferenceBank
    calls = []
    monkeypatch.setattr(A, "augment_batch", lambda *a, **kw: calls.append(kw) or "batch")
    kw = dict(num_classes=5, crop_size=8, rescale="minmax", resample_verts=False)
    cpu = torch.device("cpu")
    plain = A.AugmentedBatches(iter(_raw()), cpu, "mmwhs_light", np.random.default_rng(77), **kw)
    assert next(plain) == "batch"
    twin = np.random.default_rng(77)
    A.sample_params(3, "mmwhs_light", twin)
    assert plain.rng.bit_generator.state == twin.bit_generator.state, "without a bank the generator is consumed as before"
    assert not any(k.startswith("fourier") for k in calls[-1]), "and augment_batch is called as before"
    assert plain.last_fourier_index is None and plain.last_fourier_radius is None

    bank = _Bank(4, (16, 16, 3), np.float32, 5)
    # index only
    it = A.AugmentedBatches(iter(_raw()), cpu, "mmwhs_light", np.random.default_rng(77), fourier_bank=bank, **kw)
    twin = np.random.default_rng(77)
    for _ in range(2):
        next(it)
        want = twin.integers(4, size=3)
        A.sample_params(3, "mmwhs_light", twin)
        assert np.array_equal(it.last_fourier_index, want) and calls[-1]["fourier"] is bank
        assert np.array_equal(calls[-1]["fourier_index"], want) and calls[-1]["fourier_radius"] is None
        assert it.rng.bit_generator.state == twin.bit_generator.state
    # after the histogram bank's index draw; then the probability draw; then the radii
    hist = object.__new__(HistReferenceBank)                                    # (the loader reads its size only)
    hist.size = 6
    it = A.AugmentedBatches(iter(_raw()), cpu, "mmwhs_light", np.random.default_rng(78), match_hist_bank=hist, fourier_bank=bank,
                            fourier_p=0.5, fourier_radius_range=(1, 4), **kw)
    twin = np.random.default_rng(78)
    seen_skip = False
    for _ in range(2):
        next(it)
        hidx = twin.integers(6, size=3)
        fidx = twin.integers(4, size=3)
        fidx = np.where(twin.random(3) >= 0.5, -1, fidx)
        frad = twin.integers(1, 5, size=3)
        params = A.sample_params(3, "mmwhs_light", twin)
        assert np.array_equal(it.last_match_index, hidx) and np.array_equal(calls[-1]["match_hist_index"], hidx)
        assert np.array_equal(it.last_fourier_index, fidx) and np.array_equal(calls[-1]["fourier_index"], fidx)
        assert np.array_equal(it.last_fourier_radius, frad) and np.array_equal(calls[-1]["fourier_radius"], frad)
        assert np.array_equal(it.last_params.affine_on, params.affine_on)
        assert it.rng.bit_generator.state == twin.bit_generator.state
        seen_skip = seen_skip or bool((fidx < 0).any())
    assert seen_skip, "the seed of this test draws at least one pass-through"
    with pytest.raises(TypeError, match="FourierBank"):
        A.AugmentedBatches(iter(_raw()), cpu, "mmwhs_light", np.random.default_rng(1), fourier_bank=np.ones((2, 4, 4, 3), np.float32), **kw)
    with pytest.raises(ValueError, match="go with fourier_bank"):
        A.AugmentedBatches(iter(_raw()), cpu, "mmwhs_light", np.random.default_rng(1), fourier_p=0.5, **kw)
    with pytest.raises(ValueError, match="fourier_radius_range"):
        A.AugmentedBatches(iter(_raw()), cpu, "mmwhs_light", np.random.default_rng(1), fourier_bank=bank, fourier_radius_range=(2, 9), **kw)
    with pytest.raises(ValueError, match="fourier_p"):
        A.AugmentedBatches(iter(_raw()), cpu, "mmwhs_light", np.random.default_rng(1), fourier_bank=bank, fourier_p=1.5, **kw)


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_declares_what_the_binding_binds_and_the_entry_points_reject():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p, "double": ctypes.c_double}
    names = {"pcuda_fourier_bank_size": ("size_t", ["r", "c", "radius"]),
             "pcuda_fourier_bank_workspace_size": ("size_t", ["r", "h", "w", "c", "radius"]),
             "pcuda_fourier_bank_build": ("int", ["refs", "is_u8", "r", "h", "w", "c", "radius", "bank", "bank_bytes", "workspace",
                                                  "workspace_bytes", "s"]),
             "pcuda_fourier_adapt_workspace_size": ("size_t", ["b", "h", "w", "c", "radius"]),
             "pcuda_fourier_adapt": ("int", ["in", "out", "is_u8", "b", "h", "w", "c", "bank", "r", "radius", "ref_index",
                                             "sample_radius", "clip", "clip_lo", "clip_hi", "workspace", "workspace_bytes", "s"])}
    src = open(os.path.join(ROOT, "pointcloududa_amd", "csrc", "fourier.hip")).read()
    for name, (ret, params) in names.items():
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        decl = [s.strip() for s in m.group(2).split(",")]
        assert [a.split()[-1].lstrip("*") for a in decl] == params, name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in decl]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
        assert 'extern "C" %s %s(' % (ret, name) in src, name
    mk = open(os.path.join(ROOT, "pointcloududa_amd", "csrc", "Makefile")).read()
    assert "fourier.hip" in mk.split("SRCS")[1].splitlines()[0]
    lib = _lib.lib()
    assert lib.pcuda_fourier_bank_size(3, 2, 12) == 3 * 2 * 25 * 13 * 8 and lib.pcuda_fourier_bank_size(1, 1, 0) == 16
    assert lib.pcuda_fourier_bank_size(3, 2, 33) == 0 and lib.pcuda_fourier_bank_size(0, 2, 1) == 0 and lib.pcuda_fourier_bank_size(3, 5, 1) == 0
    assert lib.pcuda_fourier_adapt_workspace_size(2, 64, 64, 3, 2) > 0 and lib.pcuda_fourier_adapt_workspace_size(2, 64, 64, 3, 2) % 16 == 0
    assert lib.pcuda_fourier_adapt_workspace_size(2, 64, 64, 3, 32) == 0 and lib.pcuda_fourier_bank_workspace_size(2, 64, 64, 3, 32) == 0
    assert lib.pcuda_fourier_adapt_workspace_size(2, 65, 65, 1, 32) > lib.pcuda_fourier_bank_workspace_size(2, 65, 65, 1, 32) > 0
    # the argument checks that need no device: fake, never dereferenced, addresses
    IN, OUT, BANK, IDX, WS = 4096, 8192, 12288, 16384, 20480

    def adapt(in_=IN, out=OUT, b=2, h=64, w=64, c=3, bank=BANK, r=2, radius=2, idx=IDX, ws=WS, nbytes=1 << 30, clip=0, lo=0.0, hi=0.0):
        return lib.pcuda_fourier_adapt(in_, out, 0, b, h, w, c, bank, r, radius, idx, None, clip, lo, hi, ws, nbytes, None)
    assert adapt(radius=33, h=256, w=256) == -2 and b"radius" in lib.pcuda_last_error()
    assert adapt(radius=32, h=64, w=65) == -2 and b"alias" in lib.pcuda_last_error()
    assert adapt(radius=1, h=2, w=9) == -2 and adapt(c=5) == -2 and adapt(c=0) == -2
    assert adapt(h=4097, w=64) == -2
    assert adapt(out=IN) == -1 and b"in == out" in lib.pcuda_last_error()
    assert adapt(in_=None) == -1 and adapt(idx=None) == -1 and adapt(bank=None) == -1 and adapt(r=0) == -1 and adapt(radius=-1) == -1
    assert adapt(clip=1, lo=2.0, hi=1.0) == -1
    assert adapt(nbytes=16) == -4 and adapt(ws=WS + 8) == -4 and adapt(ws=None) == -4 and adapt(bank=BANK + 8) == -4
    assert adapt(b=0) == 0 and adapt(h=0) == 0 and adapt(w=0, radius=3) == 0, "an empty batch is a no-op"

    def build(refs=IN, r=2, h=64, w=64, c=3, radius=2, bank=BANK, bank_bytes=1 << 30, ws=WS, nbytes=1 << 30):
        return lib.pcuda_fourier_bank_build(refs, 1, r, h, w, c, radius, bank, bank_bytes, ws, nbytes, None)
    assert build(radius=33, h=256, w=256) == -2 and build(radius=4, h=8, w=64) == -2 and build(c=5) == -2
    assert build(refs=None) == -1 and build(refs=BANK) == -1 and b"refs == bank" in lib.pcuda_last_error()
    assert build(bank_bytes=16) == -4 and build(bank=BANK + 8) == -4 and build(nbytes=16) == -4 and build(ws=None) == -4
    assert build(r=0) == 0, "an empty set is a no-op"
