"""Device-side photometric augmentation on the GPU, through the public surface
(utils/augment.py, utils/photometric.py) and the C ABI, against the committed fixture tests/golden/photometric.npz
(scripts/make_photometric_golden.py: a scipy restatement pinned by a plain-numpy one) and, at the production size, against
the plain-numpy restatement itself.  Inputs are rebuilt from the cases' seeds; scipy is not needed here.

Rule: the images equal the restatement's except at EXCUSED pixels (a float64 operator's pre-rounding value within 1e-9 of
a rounding boundary, or such a pixel in the dependency window), which may differ by one grey level.  The integer operators
and the chains of the fixture have no excused pixel: they are bit-exact."""
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
    _spec = importlib.util.spec_from_file_location("make_photometric_golden", os.path.join(ROOT, "scripts", "make_photometric_golden.py"))
    G = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(G)
finally:
    sys.path.remove(os.path.join(ROOT, "scripts"))
CASES = G.load_cases(np.load(os.path.join(GOLD, "photometric.npz")))
NAMES = [c["name"] for c in CASES]
PRESET = "mscmrseg_aug2_photometric"


def _case(name):
    return [c for c in CASES if c["name"] == name][0]


def _program(case, rows=None, slots=None):
    from pointcloududa_amd.utils.photometric import PhotoProgram
    rows = slice(None) if rows is None else rows
    slots = slice(None) if slots is None else slots
    return PhotoProgram(*(np.ascontiguousarray(case[k][rows][:, slots]) for k in ("opcode", "iarg", "farg", "seed_arr")))


def _run(dev, images, program):
    from pointcloududa_amd.utils.photometric import photometric_aug
    x = torch.from_numpy(images).to(dev)
    keep = x.clone()
    out = photometric_aug(x, program)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x, keep), "the input is never written"
    return out.cpu().numpy()


def _check(got, want, exc, name):
    bad = (got != want) & ~exc
    print("%s: %d pixels, %d differ, %d of them outside the excused set (%d excused)" % (
        name, got.size, int((got != want).sum()), int(bad.sum()), int(exc.sum())))
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, name


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(dev, name):
    case = _case(name)
    exc = np.zeros(case["u8"].shape, dtype=bool)
    exc[tuple(case["exc"].T)] = True
    if case["chain"] or np.all(np.isin(case["opcode"], G.INTEGER_OPS)):
        assert not exc.any()                       # bit-exact
    _check(_run(dev, G.case_inputs(case), _program(case)), case["u8"], exc, name)


def test_fixture_excused_pixels_are_rare():
    assert sum(len(c["exc"]) for c in CASES) <= 1e-5 * sum(c["u8"].size for c in CASES)


# ---------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("shape", [(3, 64, 48, 3), (2, 37, 29, 1), (2, 50, 21, 3), (1, 16, 16, 4), (2, 33, 40, 2)])
def test_identity_programs_and_zero_slots_reproduce_the_input(dev, shape):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.photometric import PhotoProgram, upload_program
    x = np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)
    b, h, w, c = shape
    for slots in (0, 1, 2, 5, 8):
        prog = PhotoProgram.identity(b, slots)
        assert prog.is_identity()
        assert np.array_equal(_run(dev, x, prog), x), slots
    # an unknown opcode on the device behaves as NOP (the host validates programs: this goes below it)
    op, ia, fa, sd = upload_program(PhotoProgram.identity(b, 3), b, h, w, c, dev)
    op = op.clone()
    op[:, 1] = 99
    op[:, 2] = -7
    tx = torch.from_numpy(x).to(dev)
    assert torch.equal(K.photometric(tx, op, ia, fa, sd), tx)


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["chain"]])
def test_a_chain_equals_one_slot_calls(dev, name):
    case = _case(name)
    x = G.case_inputs(case)
    whole = _run(dev, x, _program(case))
    step = x
    for s in range(case["opcode"].shape[1]):
        step = _run(dev, step, _program(case, slots=slice(s, s + 1)))
    assert np.array_equal(whole, step)
    assert np.array_equal(whole, case["u8"])


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("per_channel", [False, True])
def test_random_operators_do_not_depend_on_the_launch_geometry(dev, c, per_channel):
    """noise and the dropouts: one sample alone against the same sample and slots at index 19 of a batch of 32"""
    from pointcloududa_amd.utils.photometric import PhotoProgram
    h, w = 96, 80
    rng = np.random.default_rng(31 + c)
    big = rng.integers(0, 256, (32, h, w, c), dtype=np.uint8)
    prog = PhotoProgram.identity(32, 3)
    for i in range(32):
        prog.set_gaussian_noise(i, 0, rng.uniform(2, 12), per_channel, int(rng.integers(0, 2 ** 63)))
        prog.set_dropout(i, 1, rng.uniform(0.02, 0.1), per_channel, int(rng.integers(0, 2 ** 63)))
        prog.set_coarse_dropout(i, 2, rng.uniform(0.05, 0.15), rng.uniform(0.03, 0.05), per_channel, int(rng.integers(0, 2 ** 63)))
    one = PhotoProgram(*(np.ascontiguousarray(a[19:20]) for a in (prog.opcode, prog.iarg, prog.farg, prog.seed)))
    got_big, got_one = _run(dev, big, prog), _run(dev, big[19:20], one)
    assert np.array_equal(got_big[19], got_one[0])
    assert not np.array_equal(got_big[19], got_big[18]) and (got_one == 0).mean() > 0.03
    want, _ = G.run_program(big[19:20], one.opcode, one.iarg, one.farg, one.seed, backend="numpy")
    assert (got_one != want).mean() <= 1e-5 and np.abs(got_one.astype(int) - want).max() <= 1


def test_production_size_sampled_program_matches_the_numpy_restatement(dev):
    """B = 32, 256 x 256 x 3, a sampled "mscmrseg_aug2_photometric" program: mismatches only where the restatement's
    pre-rounding value is inside the band"""
    from pointcloududa_amd.utils.augment import sample_program
    b, h, w, c = 32, 256, 256, 3
    x = np.concatenate([G.make_images("grey3", 16, h, w, c, 71), G.make_images("smooth", 8, h, w, c, 72),
                        G.make_images("random", 8, h, w, c, 73)])
    prog = sample_program(b, PRESET, np.random.default_rng(2026))
    assert set(np.unique(prog.opcode)) >= {1, 2, 3, 4, 5, 6, 7, 9, 10, 11} and (prog.opcode != 0).sum() > 60
    got = _run(dev, x, prog)
    want, exc = G.run_program(x, prog.opcode, prog.iarg, prog.farg, prog.seed, backend="numpy")
    assert exc.sum() <= 1e-5 * exc.size
    _check(got, want, exc, "production size")
    changed = [i for i in range(b) if not np.array_equal(got[i], x[i])]
    assert len(changed) >= 20


# ---------------------------------------------------------------------------------------------- the loader path
def _loader_inputs(dev, b=4, seed=5):
    from oracle.synth import synth_batch
    q = G.make_images("grey3", b, 256, 256, 3, seed)
    lab = np.argmax(synth_batch(b, 1, 5, 256, seed=seed)[1], axis=1).astype(np.int64)
    return q, lab, torch.from_numpy(q).to(dev), torch.from_numpy(lab).to(dev)


@pytest.mark.parametrize("rescale", ["div255", None])
def test_augment_batch_with_a_program_equals_the_two_calls(dev, rescale):
    from pointcloududa_amd.utils.augment import augment_batch, photometric_aug, sample_params, sample_program
    q, lab, tq, tl = _loader_inputs(dev)
    params = sample_params(4, "mscmrseg_simple", np.random.default_rng(3))
    params.affine_on[:2] = True
    prog = sample_program(4, PRESET, np.random.default_rng(4))
    assert not prog.is_identity()
    for crop, resample in ((224, True), (0, False)):
        one = augment_batch(tq, tl, params, 5, crop, rescale=rescale, resample_verts=resample, photometric=prog)
        two = augment_batch(photometric_aug(tq, prog), tl, params, 5, crop, rescale=rescale, resample_verts=resample)
        plain = augment_batch(tq, tl, params, 5, crop, rescale=rescale, resample_verts=resample)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
        assert torch.equal(one[1], plain[1]) and not torch.equal(one[0], plain[0]), "masks are untouched, images are not"
        if resample:
            assert torch.equal(one[2], two[2]) and torch.equal(one[2], plain[2])
    with pytest.raises(TypeError, match="uint8"):
        augment_batch(tq.float(), tl, params, 5, 0, rescale="minmax", photometric=prog)
    with pytest.raises(TypeError, match="uint8"):
        augment_batch(tq.float(), tl, params, 5, 0, rescale=None, photometric=prog)


def test_no_program_is_bit_identical_to_the_call_without_the_argument(dev):
    from pointcloududa_amd.utils.augment import augment_batch, sample_params
    q, lab, tq, tl = _loader_inputs(dev)
    params = sample_params(4, "mmwhs_light", np.random.default_rng(6))
    params.affine_on[:2] = True
    tx = torch.from_numpy(G.smooth_images(4, 256, 256, 3, 9)).to(dev)
    for img, rescale in ((tq, "div255"), (tq, None), (tx, "minmax"), (tx, None)):
        a = augment_batch(img, tl, params, 5, 224, rescale=rescale, resample_verts=True)
        b = augment_batch(img, tl, params, 5, 224, rescale=rescale, resample_verts=True, photometric=None)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_augmented_batches_with_a_photometric_preset_feed_train_epoch_shapes(dev):
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import AugmentedBatches, augment_batch, sample_params, sample_program
    raw = []
    for i in range(3):
        lab = np.argmax(synth_batch(4, 1, 5, 256, seed=40 + i)[1], axis=1).astype(np.int64)[..., None]
        raw.append((G.make_images("grey3", 4, 256, 256, 3, 50 + i), lab))
    it = AugmentedBatches(iter(raw), dev, "mscmrseg_simple", np.random.default_rng(77), num_classes=5, crop_size=224,
                          rescale="div255", photometric_preset=PRESET)
    assert it.last_program is None
    twin = np.random.default_rng(77)
    n = 0
    for (x, y, z), (img, lab) in zip(it, raw):
        assert x.dtype == torch.float32 and x.shape == (4, 3, 224, 224) and x.device.type == "cuda"
        assert y.dtype == torch.uint8 and y.shape == (4, 5, 224, 224) and z.dtype == torch.float32 and z.shape == (4, 300, 3)
        assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
        want_params = sample_params(4, "mscmrseg_simple", twin)
        want = sample_program(4, PRESET, twin)
        for k in ("opcode", "iarg", "farg", "seed"):
            assert np.array_equal(getattr(want, k), getattr(it.last_program, k)), k
        rx, ry, rz = augment_batch(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), want_params, 5, 224, "div255",
                                   resample_verts=True, photometric=want)
        assert torch.equal(x, rx) and torch.equal(y, ry) and torch.equal(z, rz)
        n += 1
    assert n == 3
    # without the preset the wrapper is what it was
    it = AugmentedBatches(iter(raw), dev, "mscmrseg_simple", np.random.default_rng(77), num_classes=5, crop_size=224, rescale="div255")
    x, y, z = next(it)
    rx, ry, rz = augment_batch(torch.from_numpy(raw[0][0]).to(dev), torch.from_numpy(raw[0][1]).to(dev),
                               sample_params(4, "mscmrseg_simple", np.random.default_rng(77)), 5, 224, "div255", resample_verts=True)
    assert it.last_program is None and torch.equal(x, rx) and torch.equal(y, ry) and torch.equal(z, rz)


def test_the_photometric_path_adds_no_host_synchronisation(dev):
    """photometric_aug and augment_batch(.., photometric=..) (resample_verts=False) under
    torch.cuda.set_sync_debug_mode("error"); the mode is first shown to be enforced (a ``.item()`` raises under it)"""
    from pointcloududa_amd.utils.augment import augment_batch, photometric_aug, sample_params, sample_program
    q, lab, tq, tl = _loader_inputs(dev)
    params = sample_params(4, "mscmrseg_simple", np.random.default_rng(3))
    prog = sample_program(4, PRESET, np.random.default_rng(4))
    ref_p = photometric_aug(tq, prog)                                                 # (warm: allocator, library load)
    ref = augment_batch(tq, tl, params, 5, 224, rescale="div255", photometric=prog)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        a = photometric_aug(tq, prog)
        b = augment_batch(tq, tl, params, 5, 224, rescale="div255", photometric=prog)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, ref_p) and torch.equal(b[0], ref[0]) and torch.equal(b[1], ref[1])


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_returns_status_codes(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd.utils.photometric import PhotoProgram, upload_program
    lib = _lib.lib()
    b, h, w, c = 2, 32, 48, 3
    x = torch.zeros((b, h, w, c), dtype=torch.uint8, device=dev)
    out = torch.full_like(x, 7)
    op, ia, fa, sd = upload_program(PhotoProgram.identity(b, 8), b, h, w, c, dev)
    need = lib.pcuda_photometric_workspace_size(b, h, w, c)
    assert need >= b * h * w * c and need % 16 == 0 and lib.pcuda_photometric_workspace_size(0, h, w, c) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(inp=x.data_ptr(), outp=out.data_ptr(), b=b, h=h, w=w, c=c, slots=8, op=op.data_ptr(), wsp=ws.data_ptr(), nbytes=need):
        return lib.pcuda_photometric(inp, outp, b, h, w, c, slots, op, ia.data_ptr(), fa.data_ptr(), sd.data_ptr(), wsp, nbytes, stream)
    assert call(outp=x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(slots=9) == -1 and b"slots" in lib.pcuda_last_error()
    assert call(slots=-1) == -1
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(wsp=None) == -4
    for kw in (dict(inp=None), dict(outp=None), dict(b=0), dict(h=0), dict(w=-1), dict(c=0), dict(c=5), dict(op=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "a rejected call launches nothing"
    assert call() == 0 and call(slots=1, wsp=None, nbytes=0) == 0 and call(slots=0, op=None, wsp=None, nbytes=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
