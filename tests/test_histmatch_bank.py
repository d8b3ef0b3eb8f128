"""CPU checks of histogram matching against a reference bank (pointcloududa_amd/utils/histmatch.py HistReferenceBank,
csrc/histmatch_bank.hip): the sorted-plane rule the kernels implement, restated in plain numpy
(tests/histmatch_bank_ref.py), equals skimage's algorithm (``match_unique`` of scripts/make_match_hist_golden.py, cross-checked
against ``match_sorted``) BIT FOR BIT on every input the GPU tests use; step 1 of the rule against its definition; the loader's
use of the generator; the host-side validation; the C declarations against the binding.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import histmatch_bank_ref as R
from conftest import ROOT

G = R.G


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", sorted(R.IMAGE_SHAPES))
def test_the_sorted_plane_rule_equals_match_unique_on_the_tile_edge_pairings(name):
    pairings = R.f32_pairings(name)
    assert len(pairings) == (3 if "17x241" in name or "31x33" in name else 4), "the equal pairing is 64x64 against 64x64 only"
    for images, refs, index in pairings:
        _same(R.match_bank(images, refs, index), R.expected(images, refs, index), (name, refs.shape))


def test_the_pairings_have_one_equal_size_and_the_exact_quantile_hit():
    sizes = [(im.shape[1] * im.shape[2], rf.shape[1] * rf.shape[2]) for n in R.IMAGE_SHAPES for im, rf, _ in R.f32_pairings(n)]
    assert len(sizes) == 18 and sum(n == m for n, m in sizes) == 1 and (4096, 4096) in sizes
    assert (4096, 2048) in sizes, "64x64 against 32x64: cnt / N equals e / M exactly with different operands"
    assert {n for n, _ in sizes} == {4096, 4097, 4095, 1023, 33410}


def test_the_rule_on_the_other_fp32_inputs():
    """C = 3 and 4 at 31x33, a constant and a two-level reference plane, a constant image plane, an image against itself
    (its own bits come back) and references that hold -0.0"""
    for c in (3, 4):
        images, refs = R.f32_set(3, 31, 33, c, 300 + c, False), R.f32_set(2, 20, 27, c, 310 + c, True)
        _same(R.match_bank(images, refs, [1, 0, 1]), R.expected(images, refs, [1, 0, 1]), "C = %d" % c)
    images = R.f32_set(3, 31, 33, 1, 320, False)
    refs = np.stack([np.full((9, 11, 1), -7.5, np.float32), np.where(np.arange(99).reshape(9, 11, 1) % 3 == 0, np.float32(-2.0),
                                                                    np.float32(5.0))])
    _same(R.match_bank(images, refs, [0, 1, 0]), R.expected(images, refs, [0, 1, 0]), "constant / two-level reference")
    assert np.all(R.match_bank(images, refs, [0, 0, 0]) == np.float32(-7.5))
    const = np.full((1, 16, 16, 1), 3.25, dtype=np.float32)
    got = R.match_bank(const, R.f32_set(1, 9, 9, 1, 330, True), [0])
    _same(got, R.expected(const, R.f32_set(1, 9, 9, 1, 330, True), [0]), "constant image")
    own = R.f32_set(3, 31, 33, 2, 340, True)
    _same(R.match_bank(own, own, [0, 1, 2]), R.expected(own, own, [0, 1, 2]), "an image against itself")
    assert np.array_equal(R.match_bank(own, own, [0, 1, 2]) + np.float32(0.0), own + np.float32(0.0))
    zeros = np.where(np.arange(35).reshape(1, 7, 5, 1) % 2 == 0, np.float32(-0.0), np.float32(1.0)).astype(np.float32)
    _same(R.match_bank(images, zeros, [0, 0, 0]), R.expected(images, zeros, [0, 0, 0]), "-0.0 in a reference")


def test_the_rule_at_the_workload_plane():
    images, refs = G.normal_f32((2, 256, 256, 3), 50, 100.0, 300.0), G.normal_f32((2, 256, 256, 3), 51, 0.0, 1.0)
    _same(R.match_bank(images, refs, [1, 0]), R.expected(images, refs, [1, 0]), "256x256x3")


def test_the_count_form_equals_match_unique_on_the_uint8_inputs():
    images = np.concatenate([G.random_u8((1, 64, 48, 3), 400), G.random_u8((1, 64, 48, 3), 401, 90, 140), G.smooth_u8((1, 64, 48, 3), 402)])
    refs = np.concatenate([G.smooth_u8((1, 40, 56, 3), 403), G.random_u8((1, 40, 56, 3), 404), G.random_u8((1, 40, 56, 3), 405, 10, 60)])
    for index in ([0, 1, 2], [2, 2, 0]):
        _same(R.match_bank(images, refs, index), R.expected(images, refs, index), "uint8 %r" % (index,))
    special = np.stack([np.full((40, 56, 3), 200, np.uint8), np.broadcast_to(np.array([3, 128, 255], np.uint8), (40, 56, 3))])
    _same(R.match_bank(images, special, [0, 1, 1]), R.expected(images, special, [0, 1, 1]), "constant / one value per channel")
    one = np.array([[[[17]]]], dtype=np.uint8)
    _same(R.match_bank(one, one + 5, [0]), R.expected(one, one + 5, [0]), "1x1x1")


def test_step_one_against_its_definition_where_the_product_alone_is_wrong():
    """e* = max{e : float64(e) / float64(M) <= q} against trunc(q M): the search over N, M <= 512 finds (N, M, cnt) where the
    product alone is one short (q M rounds below an integer e with e / M == q: N = M = 49, cnt = 1 is the smallest square
    one); ``e_star`` (guess + neighbours by the division) equals the definition on all of them, and planes of those sizes
    -- every value and every reference value distinct, so every cnt occurs -- still equal match_unique"""
    misses = R.floor_guess_misses(512)
    assert misses and (49, 49, 1) in misses
    print("%d (N, M, cnt) with trunc(q M) != e*, first %r" % (len(misses), misses[:3]))
    rng = np.random.default_rng(3)
    for n, m, cnt in [misses[i] for i in rng.choice(len(misses), 200, replace=False)] + [(49, 49, 1)]:
        q = np.float64(cnt) / np.float64(n)
        assert int(R.e_star(q, m)) == R.e_star_brute(q, m) != int(R.e_star_guess(q, m)), (n, m, cnt)
    for n, m in ((5, 7), (64, 48), (100, 1), (1, 100), (511, 512)):            # and where the guess is right
        q = np.arange(1, n + 1, dtype=np.float64) / np.float64(n)
        assert [int(e) for e in R.e_star(q, m)] == [R.e_star_brute(x, m) for x in q]
    for n, m, _ in (misses[0], misses[len(misses) // 2], misses[-1], (49, 49, 1)):
        images = rng.permutation(n).astype(np.float32).reshape(1, n, 1, 1) * np.float32(0.37)
        refs = (rng.permutation(m).astype(np.float32).reshape(1, m, 1, 1) - np.float32(m / 3)) * np.float32(1.7)
        _same(R.match_bank(images, refs, [0]), R.expected(images, refs, [0]), (n, m))


def test_keys_order_like_the_values_and_invert():
    v = np.sort(R.finite_key_coverage((4000,), 9))
    k = R.float_key(v)
    assert np.all(np.diff(k.astype(np.int64)) >= 0)
    assert np.array_equal(R.key_value(k), (v + np.float32(0.0)).astype(np.float64))
    assert R.float_key(np.float32([-0.0]))[0] == R.float_key(np.float32([0.0]))[0]


# ---------------------------------------------------------------------------------------------- the loader
class _Bank:
    """a HistReferenceBank without its device side: what the host-side validation reads"""

    def __new__(cls, size, channels, dtype):
        from pointcloududa_amd.utils.histmatch import HistReferenceBank
        import torch
        bank = object.__new__(HistReferenceBank)
        bank.size, bank.channels, bank.dtype, bank.shape = size, channels, np.dtype(dtype), (size, 8, 8, channels)
        bank.device, bank.float_bank, bank._index_cache = torch.device("cpu"), None, {}
        bank.bank = torch.zeros(size * channels * 64 * 4, dtype=torch.uint8)
        return bank


def _raw(n=2, b=3):
    rng = np.random.default_rng(1)
    return [(rng.standard_normal((b, 16, 16, 3)).astype(np.float32), rng.integers(0, 5, (b, 16, 16, 1))) for _ in range(n)]


def test_augmented_batches_draw_the_indices_first_and_only_with_a_bank(monkeypatch):
    import torch
    from pointcloududa_amd.utils import augment as A
    calls = []
    monkeypatch.setattr(A, "augment_batch", lambda *a, **kw: calls.append(kw) or "batch")
    kw = dict(num_classes=5, crop_size=8, rescale="minmax", resample_verts=False)
    plain = A.AugmentedBatches(iter(_raw()), torch.device("cpu"), "mmwhs_light", np.random.default_rng(77), **kw)
    assert next(plain) == "batch" and plain.match_hist is None and plain.match_hist_bank is None
    twin = np.random.default_rng(77)
    A.sample_params(3, "mmwhs_light", twin)
    assert plain.rng.bit_generator.state == twin.bit_generator.state, "without a bank the generator is consumed as before"
    assert calls[-1]["match_hist"] is None and calls[-1]["match_hist_index"] is None and plain.last_match_index is None

    bank = _Bank(4, 3, np.float32)
    it = A.AugmentedBatches(iter(_raw()), torch.device("cpu"), "mmwhs_light", np.random.default_rng(77), match_hist_bank=bank, **kw)
    twin = np.random.default_rng(77)
    for _ in range(2):
        next(it)
        want = twin.integers(4, size=3)                                        # the first draw of the batch
        params = A.sample_params(3, "mmwhs_light", twin)
        assert np.array_equal(it.last_match_index, want) and calls[-1]["match_hist"] is bank
        assert np.array_equal(calls[-1]["match_hist_index"], want)
        assert np.array_equal(it.last_params.affine_on, params.affine_on)
        assert it.rng.bit_generator.state == twin.bit_generator.state
    with pytest.raises(ValueError, match="not both"):
        A.AugmentedBatches(iter(_raw()), torch.device("cpu"), "mmwhs_light", np.random.default_rng(1),
                           match_hist_reference=np.ones((4, 4, 3), np.float32), match_hist_bank=bank, **kw)
    with pytest.raises(TypeError, match="HistReferenceBank"):
        A.AugmentedBatches(iter(_raw()), torch.device("cpu"), "mmwhs_light", np.random.default_rng(1),
                           match_hist_bank=np.ones((2, 4, 4, 3), np.float32), **kw)


# ---------------------------------------------------------------------------------------------- validation
def test_the_wrappers_validate_on_the_host():
    import torch
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import histmatch as H
    assert A.HistReferenceBank is H.HistReferenceBank
    for bad in (np.zeros((2, 4, 4, 3), np.float64), np.zeros((2, 4, 4, 3), np.int16), torch.zeros((2, 4, 4, 3), dtype=torch.float16)):
        with pytest.raises(TypeError, match="fp32 or uint8"):
            H.HistReferenceBank(bad, "cpu")
    with pytest.raises(ValueError, match="dimensions"):
        H.HistReferenceBank(np.zeros((4, 4), np.float32), "cpu")
    with pytest.raises(ValueError, match="1..4 channels"):
        H.HistReferenceBank(np.zeros((2, 4, 4, 5), np.float32), "cpu")
    with pytest.raises(RuntimeError, match="HIP device"):                       # no CPU fallback
        H.HistReferenceBank(np.zeros((2, 4, 4, 3), np.float32), "cpu")
    f32, u8 = _Bank(3, 3, np.float32), _Bank(3, 3, np.uint8)
    x, x8 = torch.zeros((5, 8, 8, 3)), torch.zeros((5, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="channels"):
        H.match_histograms(torch.zeros((5, 8, 8, 1)), f32, index=[0] * 5)
    with pytest.raises(TypeError, match="uint8 bank"):
        H.match_histograms(x8, f32, index=[0] * 5)
    with pytest.raises(TypeError, match="float_images"):
        H.match_histograms(x, u8, index=[0] * 5)
    with pytest.raises(TypeError, match="fp32 or uint8"):
        H.match_histograms(x.double(), f32, index=[0] * 5)
    with pytest.raises(ValueError, match="one entry per sample"):
        H.match_histograms(x, f32, index=[0, 1, 2])
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        H.match_histograms(x, f32, index=[0, 1, 2, 3, 0])
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        H.match_histograms(x, f32, index=np.array([0, -1, 2, 1, 0]))
    with pytest.raises(TypeError, match="integers"):
        H.match_histograms(x, f32, index=[0.0, 1.0, 2.0, 1.0, 0.0])
    with pytest.raises(ValueError, match="as many references as samples"):
        H.match_histograms(x, f32)
    with pytest.raises(TypeError, match="HistReferenceBank"):
        H.match_histograms(x, H.HistReference(np.ones((4, 4, 3), np.float32), "cpu"), index=[0] * 5)
    with pytest.raises(TypeError, match="match_hist_index"):
        A.augment_batch(x, torch.zeros((5, 8, 8), dtype=torch.int64), None, match_hist_index=[0] * 5)
    assert H.validate_index((2, 0, 1), 3, 3).dtype == np.int32 and H.validate_index(np.array([2, 0], np.int64), 2, 3).tolist() == [2, 0]
    with pytest.raises(RuntimeError, match="HIP device"):                       # valid arguments reach the kernel wrapper
        H.match_histograms(x, f32, index=[0, 1, 2, 1, 0])


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_declares_what_the_binding_binds():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p}
    names = {"pcuda_hist_bank_size": ("size_t", ["r", "rh", "rw", "c", "is_u8"]),
             "pcuda_hist_bank_workspace_size": ("size_t", ["r", "rh", "rw", "c", "is_u8"]),
             "pcuda_hist_bank_build": ("int", ["refs", "is_u8", "r", "rh", "rw", "c", "bank", "bank_bytes", "flag", "workspace",
                                               "workspace_bytes", "s"]),
             "pcuda_match_hist_bank_workspace_size": ("size_t", ["b", "h", "w", "c", "is_u8"]),
             "pcuda_match_hist_bank": ("int", ["in", "out", "is_u8", "b", "h", "w", "c", "bank", "r", "rh", "rw", "ref_index",
                                               "workspace", "workspace_bytes", "s"])}
    src = open(os.path.join(ROOT, "pointcloududa_amd", "csrc", "histmatch_bank.hip")).read()
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
    assert "histmatch_bank.hip" in mk.split("SRCS")[1].splitlines()[0]
    lib = _lib.lib()
    assert lib.pcuda_hist_bank_size(3, 10, 7, 2, 0) == (3 * 2 * 70 * 4 + 15) // 16 * 16 == lib.pcuda_hist_bank_workspace_size(3, 10, 7, 2, 0)
    assert lib.pcuda_hist_bank_size(3, 10, 7, 2, 1) == 3 * 2 * 256 * 4 and lib.pcuda_hist_bank_workspace_size(3, 10, 7, 2, 1) == 0
    assert lib.pcuda_hist_bank_size(0, 10, 7, 2, 0) == 0 and lib.pcuda_match_hist_bank_workspace_size(2, 5, 5, 3, 1) == 0
    assert lib.pcuda_match_hist_bank_workspace_size(2, 5, 5, 3, 0) == lib.pcuda_match_hist_workspace_size(2, 5, 5, 3, 0) == 1200
    # the argument checks that need no device
    assert lib.pcuda_match_hist_bank(None, None, 0, 2, 5, 5, 5, None, 1, 4, 4, None, None, 0, None) == -1
    assert lib.pcuda_hist_bank_build(None, 0, 1, 4, 4, 3, None, 0, None, None, 0, None) == -1 and b"null" in lib.pcuda_last_error()
    assert lib.pcuda_hist_bank_build(None, 0, 0, 4, 4, 3, None, 0, None, None, 0, None) == 0, "an empty set is a no-op"
