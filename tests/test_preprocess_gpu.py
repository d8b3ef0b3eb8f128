"""GPU checks of the device-side slice preparation (csrc/preprocess.hip, pointcloududa_amd/utils/preprocess.py; DESIGN.md
section 6, f11) against the committed fixture tests/golden/preprocess.npz: the device equals the two restatements of
scripts/make_preprocess_golden.py BIT FOR BIT, with no tolerance."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_preprocess_golden", os.path.join(ROOT, "scripts", "make_preprocess_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
CLAHE_CASES, RESCALE_CASES = G.load_cases(np.load(os.path.join(GOLD, "preprocess.npz")))
BY = {c["name"]: c for c in CLAHE_CASES}


def _diff(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    return "%d of %d values differ, first at %s: got %s, want %s" % (
        len(bad), want.size, np.unravel_index(bad[0], want.shape) if len(bad) else None,
        got.ravel()[bad[:4]].tolist(), want.ravel()[bad[:4]].tolist()) if len(bad) else ""


@pytest.mark.parametrize("case", CLAHE_CASES, ids=[c["name"] for c in CLAHE_CASES])
def test_clahe_equals_the_golden_bit_for_bit(dev, case):
    from pointcloududa_amd.utils.preprocess import clahe
    x = torch.from_numpy(case["images"]).to(dev)
    out = clahe(x, case["clip_limit"], case["grid"])
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert not _diff(out, case["expected"]), _diff(out, case["expected"])
    assert np.array_equal(x.cpu().numpy(), case["images"]), "the input is never written"


@pytest.mark.parametrize("name", ["224x224_g4x4_clip2_n3", "17x13_g4x4_clip2", "n5_20x28_g2x2_clip3", "30x18_g3x5_clip2.5",
                                  "all0_all255_16x16_g4x4_clip2"])
def test_clahe_to_float_is_u8_over_255_in_three_channels(dev, name):
    """both store paths: dword / float4 where the width is a multiple of four, scalar elsewhere"""
    from pointcloududa_amd.utils.preprocess import clahe
    case = BY[name]
    out = clahe(torch.from_numpy(case["images"]).to(dev), case["clip_limit"], case["grid"], to_float=True)
    want = G.to_float3(case["expected"])
    assert out.dtype == torch.float32 and tuple(out.shape) == (case["images"].shape[0], 3) + case["images"].shape[1:]
    assert not _diff(out, want), _diff(out, want)


def test_clahe_takes_one_slice_a_batch_of_one_and_a_batch_of_five(dev):
    from pointcloududa_amd.utils.preprocess import clahe, preprocess_volume
    case = BY["n5_20x28_g2x2_clip3"]
    x = torch.from_numpy(case["images"]).to(dev)
    one = clahe(x[2], case["clip_limit"], case["grid"])                       # a 2-D input
    assert one.shape == (20, 28) and not _diff(one, case["expected"][2])
    assert not _diff(clahe(x[4:5], case["clip_limit"], case["grid"]), case["expected"][4:5])
    assert not _diff(clahe(x, case["clip_limit"], case["grid"]), case["expected"])
    f = clahe(x[1], case["clip_limit"], case["grid"], to_float=True)
    assert tuple(f.shape) == (1, 3, 20, 28) and not _diff(f, G.to_float3(case["expected"][1:2]))
    # a non-contiguous view is gathered first
    wide = torch.zeros((5, 20, 40), dtype=torch.uint8, device=dev)
    wide[:, :, 3:31] = x
    assert not _diff(clahe(wide[:, :, 3:31], case["clip_limit"], case["grid"]), case["expected"])
    # the reference's name and fixed parameters
    ref = BY["224x224_g4x4_clip2_n3"]
    assert not _diff(preprocess_volume(torch.from_numpy(ref["images"]).to(dev)), ref["expected"])
    empty = clahe(torch.zeros((0, 16, 16), dtype=torch.uint8, device=dev))
    assert tuple(empty.shape) == (0, 16, 16)


def test_clahe_on_misaligned_slices_takes_the_scalar_path_with_the_same_bits(dev):
    """w % 4 == 0 but the batch starts one byte into an allocation: no dword loads there"""
    from pointcloududa_amd import kernels as K
    case = BY["64x64_g2x2_clip2"]
    buf = torch.zeros(64 * 64 + 8, dtype=torch.uint8, device=dev)
    x = buf[1:1 + 64 * 64].view(1, 64, 64)
    x.copy_(torch.from_numpy(case["images"]).to(dev))
    assert x.data_ptr() % 4 == 1
    assert not _diff(K.clahe(x, case["clip_limit"], 2, 2), case["expected"])
    assert not _diff(K.clahe(x, case["clip_limit"], 2, 2, True), G.to_float3(case["expected"]))


@pytest.mark.parametrize("case", RESCALE_CASES, ids=[c["name"] for c in RESCALE_CASES])
def test_rescale_resize_crop_equals_the_golden_bit_for_bit(dev, case):
    from pointcloududa_amd import kernels as K
    x = torch.from_numpy(case["volume"]).to(dev)
    out = K.rescale_resize_crop_u8(x, case["resize_h"], case["resize_w"], case["crop"])
    assert not _diff(out, case["expected"]), _diff(out, case["expected"])
    assert np.array_equal(x.cpu().numpy(), case["volume"]), "the input is never written"


@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.uint8], ids=["f32", "i16", "u8"])
def test_rescale_finds_the_extremes_in_wide_loads_tails_and_misaligned_volumes(dev, dtype):
    """the reduce reads 16 bytes per lane where the volume starts on a 16-byte boundary and the rest value by value; the map
    kernel stores dwords where the row pitch and the pointer allow it"""
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(60)
    for shape, at_lo, at_hi in (((1, 5, 7), 34, 0), ((1, 5, 7), 0, 34), ((2, 9, 23), 413, 400), ((1, 16, 16), 100, 255), ((3, 8, 24), 7, 570)):
        vol = rng.integers(60, 120, shape).astype(dtype)
        vol.ravel()[at_lo], vol.ravel()[at_hi] = 3, 250
        want = G.rescale_numpy(vol, 12, 16, 0)
        assert not _diff(K.rescale_resize_crop_u8(torch.from_numpy(vol).to(dev), 12, 16), want), shape
        # the same volume one element into an allocation, into an output one byte into another
        buf = torch.zeros(vol.size + 8, dtype=torch.from_numpy(vol).dtype, device=dev)
        x = buf[1:1 + vol.size].view(shape)
        x.copy_(torch.from_numpy(vol).to(dev))
        obuf = torch.zeros(want.size + 8, dtype=torch.uint8, device=dev)
        out = obuf[1:1 + want.size].view(want.shape)
        assert x.data_ptr() % 16 != 0 and out.data_ptr() % 4 == 1
        K.rescale_resize_crop_u8(x, 12, 16, out=out)
        assert not _diff(out, want), shape
        assert obuf[0] == 0 and not obuf[1 + want.size:].any(), "nothing is written outside the output"


def test_the_thin_views_of_the_second_entry_point(dev):
    from pointcloududa_amd.utils import preprocess as P
    by = {c["name"]: c for c in RESCALE_CASES}
    for tag in ("f32", "i16", "u8"):
        vol = by["%s_3x20x28_to16_crop0" % tag]["volume"]
        u8 = P.rescale_intensity_u8(torch.from_numpy(vol).to(dev))
        assert not _diff(u8, G.rescale_numpy(vol))
        resized = P.resize_volume(u8, w=16, h=16)
        assert not _diff(resized, by["%s_3x20x28_to16_crop0" % tag]["expected"]), "nearest resize of the rescaled volume, values kept"
        assert not _diff(P.crop_volume(resized, crop_size=6), by["%s_3x20x28_to16_crop12" % tag]["expected"])
    # resize_volume / crop_volume keep the values of a uint8 volume that does not span 0 .. 255
    raw = G.random_u8((2, 9, 11), 31, 40, 90)
    ys, xs = np.minimum(np.floor(np.arange(14) * (1.0 / (14.0 / 9.0))).astype(int), 8), np.minimum(
        np.floor(np.arange(5) * (1.0 / (5.0 / 11.0))).astype(int), 10)
    assert not _diff(P.resize_volume(torch.from_numpy(raw).to(dev), w=5, h=14), np.ascontiguousarray(raw[:, ys[:, None], xs[None, :]]))
    assert not _diff(P.crop_volume(torch.from_numpy(raw).to(dev), crop_size=3), np.ascontiguousarray(raw[:, 1:7, 2:8]))
    assert tuple(P.resize_volume(torch.from_numpy(raw).to(dev)).shape) == (2, 256, 256)


def test_prepare_mscmrseg_slices_equals_the_composition_of_the_parts(dev):
    from pointcloududa_amd.utils import preprocess as P
    rng = np.random.default_rng(40)
    y, x = np.mgrid[0:40, 0:36]
    raw = (np.exp(-((y - 20) ** 2 + (x - 17) ** 2) / 150.0)[None] * rng.uniform(500, 900, (3, 1, 1))
           + rng.standard_normal((3, 40, 36)) * 20.0).astype(np.int16)
    t = torch.from_numpy(raw).to(dev)
    u8 = G.rescale_numpy(raw, 32, 32, 24)
    want = G.clahe_numpy(u8, 2.0, (4, 4))
    assert u8.shape == (3, 24, 24) and G.bit_equal(want, G.clahe_loops(u8, 2.0, (4, 4)))
    got = P.prepare_mscmrseg_slices(t, size=32, crop_size=24)
    assert tuple(got.shape) == (3, 3, 24, 24) and not _diff(got, G.to_float3(want))
    assert not _diff(P.prepare_mscmrseg_slices(t, size=32, crop_size=24, to_float=False), want)
    assert not _diff(P.prepare_mscmrseg_slices(t, size=32, crop_size=24, clahe=False, to_float=False), u8)
    # and of the package's own parts
    parts = P.preprocess_volume(P.crop_volume(P.resize_volume(P.rescale_intensity_u8(t), w=32, h=32), crop_size=12))
    assert torch.equal(parts, P.prepare_mscmrseg_slices(t, size=32, crop_size=24, to_float=False))
    # the reference's sizes: 256 -> 224, fp32 in (one slice; the restatement's loops are not run at this size)
    vol = (G.slices_u8((1, 256, 256), 41).astype(np.float32) * 3.5 - 100.0)
    got = P.prepare_mscmrseg_slices(torch.from_numpy(vol).to(dev))
    want = G.to_float3(G.clahe_numpy(G.rescale_numpy(vol, 256, 256, 224), 2.0, (4, 4)))
    assert tuple(got.shape) == (1, 3, 224, 224) and not _diff(got, want)


def test_in_place_calls_and_wrong_dtypes_raise(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import preprocess as P
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.zeros((2, 16, 16), dtype=torch.uint8, device=dev)
    o = torch.empty_like(x)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    need = lib.pcuda_clahe_workspace_size(2, 4, 4)
    assert need == 2 * 16 * 256 and lib.pcuda_clahe_workspace_size(0, 4, 4) == 0 and lib.pcuda_clahe_workspace_size(2, 17, 4) == 0
    big = torch.empty(need, dtype=torch.uint8, device=dev)

    def call(inp, outp, n=2, h=16, w=16, clip=2.0, tx=4, ty=4, mode=0, wsp=big.data_ptr(), nbytes=need):
        return lib.pcuda_clahe(inp, outp, n, h, w, clip, tx, ty, mode, wsp, nbytes, stream)
    assert call(x.data_ptr(), o.data_ptr()) == 0
    assert call(x.data_ptr(), x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(None, None, n=0) == 0, "an empty batch is a no-op"
    assert call(x.data_ptr(), o.data_ptr(), wsp=ws.data_ptr(), nbytes=4096) == -4
    assert call(x.data_ptr(), o.data_ptr(), wsp=big.data_ptr() + 1) == -4
    for kw in (dict(tx=0), dict(ty=17), dict(h=1), dict(w=1), dict(mode=2), dict(clip=float("nan")), dict(h=2, w=3, tx=2, ty=2),
               dict(n=-1), dict(h=32768, w=32768, tx=1, ty=1)):
        assert call(x.data_ptr(), o.data_ptr(), **kw) == -1, kw
    assert call(None, o.data_ptr()) == -1
    with pytest.raises(ValueError, match="out does not match"):
        K.clahe(x, out=torch.empty((2, 16, 8), dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError):
        K.clahe(x, to_float=True, out=o)
    with pytest.raises(TypeError):
        K.clahe(x.float())
    with pytest.raises(TypeError):
        K.clahe(x[0])
    with pytest.raises(RuntimeError, match="in == out"):
        K.clahe(x, out=x)
    with pytest.raises(TypeError, match="uint8"):
        P.clahe(x.to(torch.int16))

    v = torch.zeros((2, 8, 8), dtype=torch.int16, device=dev)
    vo = torch.empty((2, 8, 8), dtype=torch.uint8, device=dev)
    rneed = lib.pcuda_rescale_resize_crop_u8_workspace_size()
    assert 8 <= rneed <= 4096

    def rcall(inp, outp, dt=1, n=2, sh=8, sw=8, rh=8, rw=8, crop=0, wsp=ws.data_ptr(), nbytes=4096):
        return lib.pcuda_rescale_resize_crop_u8(inp, dt, n, sh, sw, rh, rw, crop, outp, wsp, nbytes, stream)
    assert rcall(v.data_ptr(), vo.data_ptr()) == 0
    u = torch.zeros((2, 8, 8), dtype=torch.uint8, device=dev)
    assert rcall(u.data_ptr(), u.data_ptr(), dt=2) == -1 and b"in == out" in lib.pcuda_last_error()
    assert rcall(None, None, n=0) == 0
    assert rcall(v.data_ptr(), vo.data_ptr(), wsp=None) == -4 and rcall(v.data_ptr(), vo.data_ptr(), nbytes=4) == -4
    for kw in (dict(dt=4), dict(dt=-1), dict(sh=0), dict(rw=0), dict(crop=-2), dict(crop=10), dict(crop=1), dict(n=-1)):
        assert rcall(v.data_ptr(), vo.data_ptr(), **kw) == -1, kw
    with pytest.raises(TypeError, match="fp32, int16 or uint8"):
        K.rescale_resize_crop_u8(v.to(torch.int32))
    with pytest.raises(TypeError, match="raw"):
        K.rescale_resize_crop_u8(v, raw=True)
    with pytest.raises(ValueError, match="leaves"):
        K.rescale_resize_crop_u8(v, 8, 8, 10)
    with pytest.raises(RuntimeError, match="in == out"):
        K.rescale_resize_crop_u8(u, out=u)
    with pytest.raises(TypeError):
        P.rescale_intensity_u8(v.double())
    torch.cuda.synchronize()


def test_two_runs_give_identical_bytes(dev):
    from pointcloududa_amd.utils import preprocess as P
    case = BY["224x224_g4x4_clip2_n3"]
    x = torch.from_numpy(case["images"]).to(dev)
    vol = torch.from_numpy((G.slices_u8((4, 96, 80), 50).astype(np.float32) - 30.0) * 7.25).to(dev)
    for _ in range(3):
        a, b = P.clahe(x), P.clahe(x)
        assert torch.equal(a, b)
        fa, fb = P.clahe(x, to_float=True), P.clahe(x, to_float=True)
        assert torch.equal(fa, fb)
        pa, pb = P.prepare_mscmrseg_slices(vol, size=64, crop_size=48), P.prepare_mscmrseg_slices(vol, size=64, crop_size=48)
        assert torch.equal(pa, pb)


def test_the_preparation_adds_no_host_synchronisation(dev):
    from pointcloududa_amd.utils import preprocess as P
    vol = torch.from_numpy(G.slices_u8((2, 40, 40), 51).astype(np.int16) * 5 - 300).to(dev)
    want = P.prepare_mscmrseg_slices(vol, size=32, crop_size=24)                   # (warm: allocator, library load)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = P.prepare_mscmrseg_slices(vol, size=32, crop_size=24)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, want)
