"""Device-side geometric augmentation on the GPU, through the public surface (utils/augment.py,
utils/geometric.py) and the C ABI, against the committed fixture tests/golden/geometric.npz
(scripts/make_geometric_golden.py: a scipy map_coordinates restatement pinned by a plain-numpy one) and, at the production
size, against the plain-numpy restatement itself.  scipy is not needed here.

Rule: images and labels equal the restatement's except at EXCUSED pixels (order 1: the pre-rounding value within 1e-9 of
k + 1/2, one grey level; order 0 and labels: a source coordinate within 1e-9 of a half-integer).  The chains of the fixture
have no excused pixel in any slot: they are bit-exact.  Nothing here provokes a fault: wrong programs are finite, in-range
matrices that point far outside the image."""
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
    _spec = importlib.util.spec_from_file_location("make_geometric_golden", os.path.join(ROOT, "scripts", "make_geometric_golden.py"))
    G = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(G)
finally:
    sys.path.remove(os.path.join(ROOT, "scripts"))
CASES = G.load_cases(np.load(os.path.join(GOLD, "geometric.npz")))
NAMES = [c["name"] for c in CASES]


def _case(name):
    return [c for c in CASES if c["name"] == name][0]


def _program(case, rows=None, slots=None):
    from pointcloududa_amd.utils.geometric import GeoProgram
    rows = slice(None) if rows is None else rows
    slots = slice(None) if slots is None else slots
    return GeoProgram(*(np.ascontiguousarray(case[k][rows][:, slots]) for k in ("opcode", "iarg", "farg", "seed_arr")))


def _run(dev, images, labels, program):
    from pointcloududa_amd.utils.geometric import geometric_aug
    x, l = torch.from_numpy(images).to(dev), torch.from_numpy(labels).to(dev)
    kx, kl = x.clone(), l.clone()
    out, lab = geometric_aug(x, l, program)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert lab.dtype == l.dtype and lab.shape == l.shape and lab.data_ptr() != l.data_ptr()
    assert torch.equal(x, kx) and torch.equal(l, kl), "the inputs are never written"
    return out.cpu().numpy(), lab.cpu().numpy()


def _check(got, want, exc, name, step=1):
    bad = (got != want) & ~exc
    print("%s: %d values, %d differ, %d of them outside the excused set (%d excused)" % (
        name, got.size, int((got != want).sum()), int(bad.sum()), int(exc.sum())))
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    if step:
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= step, name


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(dev, name):
    case = _case(name)
    exc, exc_lab = G.exc_masks(case)
    if case["chain"]:
        assert not exc.any() and not exc_lab.any()                       # bit-exact
    got, lab = _run(dev, case["images"], case["labels"], _program(case))
    # (an excused order-0 pixel may take the neighbouring texel: any value; an excused order-1 pixel differs by one level)
    _check(got, case["u8"], exc, name, step=1 if np.all(case["iarg"][..., 0][case["opcode"] != 0] == 1) else 0)
    _check(lab, case["lab"], exc_lab, name + " labels", step=0)


def test_fixture_excused_pixels_are_rare():
    g = np.load(os.path.join(GOLD, "geometric.npz"))
    tot, exc = (int(v) for v in g["counts"])
    assert exc == sum(len(c["exc"]) + len(c["exc_lab"]) for c in CASES) and exc <= 1e-5 * tot


# ---------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("shape", [(3, 64, 48, 3), (2, 37, 29, 1), (2, 50, 21, 3), (1, 16, 16, 4), (2, 33, 40, 2), (2, 2, 2, 1), (1, 5, 131, 3)])
def test_identity_programs_and_zero_slots_reproduce_the_input(dev, shape):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.geometric import GeoProgram, upload_geo_program
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    b, h, w, c = shape
    lab = rng.integers(0, 5, (b, h, w)).astype(np.int64)
    for slots in (0, 1, 2, 5, 8):
        prog = GeoProgram.identity(b, slots)
        assert prog.is_identity()
        got, gl = _run(dev, x, lab, prog)
        assert np.array_equal(got, x) and np.array_equal(gl, lab), slots
    # the identity as a homography, in every order and mode, and the flips applied twice
    prog = GeoProgram.identity(b, 5)
    for i in range(b):
        prog.set_homography(i, 0, np.eye(3), order=i % 2, mode=(i + 1) % 5, cval=9)
        prog.set_flip_lr(i, 1, w); prog.set_flip_ud(i, 2, h); prog.set_flip_lr(i, 3, w); prog.set_flip_ud(i, 4, h)
    got, gl = _run(dev, x, lab, prog)
    assert np.array_equal(got, x) and np.array_equal(gl, lab)
    # without labels
    tx = torch.from_numpy(x).to(dev)
    from pointcloududa_amd.utils.geometric import geometric_aug
    out, none = geometric_aug(tx, None, prog)
    assert none is None and torch.equal(out, tx)
    # an unknown opcode on the device behaves as NOP (the host validates programs: this goes below it)
    op, ia, fa, sd = upload_geo_program(GeoProgram.identity(b, 3), b, h, w, dev)
    op = op.clone()
    op[:, 1] = 99
    op[:, 2] = -7
    out, _ = K.geometric(tx, None, op, ia, fa, sd)
    assert torch.equal(out, tx)


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["chain"]])
def test_a_chain_equals_one_slot_calls(dev, name):
    case = _case(name)
    whole, whole_lab = _run(dev, case["images"], case["labels"], _program(case))
    step, step_lab = case["images"], case["labels"]
    for s in range(case["opcode"].shape[1]):
        step, step_lab = _run(dev, step, step_lab, _program(case, slots=slice(s, s + 1)))
    assert np.array_equal(whole, step) and np.array_equal(whole_lab, step_lab)
    assert np.array_equal(whole, case["u8"]) and np.array_equal(whole_lab, case["lab"])


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("sigma", [0.25, 1.0])
def test_elastic_does_not_depend_on_the_launch_geometry(dev, c, sigma):
    """one sample alone against the same sample and slot at index 19 of a batch of 32"""
    from pointcloududa_amd.utils.geometric import GeoProgram
    h, w = 96, 80
    rng = np.random.default_rng(31 + c)
    big = rng.integers(0, 256, (32, h, w, c), dtype=np.uint8)
    lab = rng.integers(0, 5, (32, h, w)).astype(np.int64)
    prog = GeoProgram.identity(32, 1)
    for i in range(32):
        prog.set_elastic(i, 0, rng.uniform(0.5, 3.5) / sigma, sigma, int(rng.integers(0, 2 ** 63)), mode=int(rng.integers(0, 5)))
    one = GeoProgram(*(np.ascontiguousarray(a[19:20]) for a in (prog.opcode, prog.iarg, prog.farg, prog.seed)))
    (got_big, lab_big), (got_one, lab_one) = _run(dev, big, lab, prog), _run(dev, big[19:20], lab[19:20], one)
    assert np.array_equal(got_big[19], got_one[0]) and np.array_equal(lab_big[19], lab_one[0])
    assert not np.array_equal(got_one[0], big[19]) and not np.array_equal(lab_one[0], lab[19])
    want, want_lab, exc, exc_lab, _ = G.run_program(big[19:20], lab[19:20], one.opcode, one.iarg, one.farg, one.seed, backend="numpy")
    _check(got_one, want, exc, "elastic alone")
    _check(lab_one, want_lab, exc_lab, "elastic alone labels", step=0)


def test_production_size_sampled_plan_matches_the_numpy_restatement(dev):
    """B = 32, 256 x 256 x 3, a sampled "heavy_device" plan: every geometric stage against the plain-numpy restatement
    (its input is the device's output of the stage before, so the photometric stages, f7's ground, are not restated)"""
    from pointcloududa_amd.utils.augment import sample_heavy_plan
    from pointcloududa_amd.utils.geometric import GeoProgram, geometric_aug, photometric_aug
    from oracle.synth import synth_batch
    import make_photometric_golden as PG  # noqa: F401  (imported by the generator; f7's inputs)
    b, h, w, c = 32, 256, 256, 3
    x = np.concatenate([PG.make_images("grey3", 16, h, w, c, 81), PG.make_images("smooth", 8, h, w, c, 82),
                        PG.make_images("random", 8, h, w, c, 83)])
    lab = np.argmax(synth_batch(b, 1, 5, 256, seed=8)[1], axis=1).astype(np.int64)
    plan = sample_heavy_plan(b, "heavy_device", np.random.default_rng(2027), h, w)
    geo = [st for st in plan.stages if isinstance(st, GeoProgram)]
    assert len(geo) >= 2 and len(geo) < len(plan.stages)
    assert set(np.concatenate([st.opcode.ravel() for st in geo])) >= {1, 2, 3}
    tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    values = excused = 0
    for k, st in enumerate(plan.stages):
        if not isinstance(st, GeoProgram):
            tx = photometric_aug(tx, st)
            continue
        before, before_lab = tx.cpu().numpy(), tl.cpu().numpy()
        tx, tl = geometric_aug(tx, tl, st)
        want, want_lab, exc, exc_lab, earlier = G.run_program(before, before_lab, st.opcode, st.iarg, st.farg, st.seed, backend="numpy")
        got, got_lab = tx.cpu().numpy(), tl.cpu().numpy()
        if st.slots == 1:          # (in a stage of several slots an excused pixel of an earlier slot spreads: compare the rest)
            _check(got, want, exc, "stage %d" % k, step=0)
            _check(got_lab, want_lab, exc_lab, "stage %d labels" % k, step=0)
        else:
            clean = earlier == 0
            print("stage %d: %d slots, %d excused in earlier slots" % (k, st.slots, earlier))
            if clean:
                _check(got, want, exc, "stage %d" % k, step=0)
                _check(got_lab, want_lab, exc_lab, "stage %d labels" % k, step=0)
            else:      # one slot at a time from the device's own intermediate values
                cur, cur_lab = before, before_lab
                for s in range(st.slots):
                    one = GeoProgram(*(np.ascontiguousarray(a[:, s:s + 1]) for a in (st.opcode, st.iarg, st.farg, st.seed)))
                    w1, wl1, e1, el1, _ = G.run_program(cur, cur_lab, one.opcode, one.iarg, one.farg, one.seed, backend="numpy")
                    cur, cur_lab = _run(dev, cur, cur_lab, one)
                    _check(cur, w1, e1, "stage %d slot %d" % (k, s), step=0)
                    _check(cur_lab, wl1, el1, "stage %d slot %d labels" % (k, s), step=0)
                assert np.array_equal(cur, got) and np.array_equal(cur_lab, got_lab)
        values += exc.size + exc_lab.size
        excused += int(exc.sum()) + int(exc_lab.sum())
    print("production size: %d values, %d excused" % (values, excused))
    assert not np.array_equal(tl.cpu().numpy(), lab)


def test_wrong_but_finite_programs_read_inside_the_image(dev):
    """the garbage-program guarantee through finite, in-range matrices that point far outside the image (and one whose
    denominator crosses zero inside the frame): every mode folds the indices, the result is the restatement's"""
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.geometric import GeoProgram
    b, h, w, c = 10, 40, 36, 3
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)
    lab = rng.integers(0, 5, (b, h, w)).astype(np.int64)
    prog = GeoProgram.identity(b, 1)
    for i in range(b):
        m = np.array([[1e3 * (i + 1) + 0.3717, 37.3129, -2e5], [-11.2931, 3e3 + 0.7193, 1e6 * (i - 4.5)], [0.0, 0.0, 1.0]])
        if i >= 8:
            m = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0], [-1.0 / 17.3, 0.0, 1.0]])      # d = 0 between two pixel columns
        prog.set_homography(i, 0, m, order=i % 2, mode=(i // 2) % 5, cval=100 + i)
    arrays = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (prog.opcode, prog.iarg, prog.farg, prog.seed.view(np.int64))]
    out, gl = K.geometric(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev).to(torch.int32), *arrays)
    want, want_lab, exc, exc_lab, _ = G.run_program(x, lab, prog.opcode, prog.iarg, prog.farg, prog.seed, backend="numpy")
    _check(out.cpu().numpy(), want, exc, "far outside", step=0)
    _check(gl.cpu().numpy().astype(np.int64), want_lab, exc_lab, "far outside labels", step=0)


# ---------------------------------------------------------------------------------------------- the loader path
def _loader_inputs(dev, b=4, seed=5):
    from oracle.synth import synth_batch
    import make_photometric_golden as PG
    q = PG.make_images("grey3", b, 256, 256, 3, seed)
    lab = np.argmax(synth_batch(b, 1, 5, 256, seed=seed)[1], axis=1).astype(np.int64)
    return q, lab, torch.from_numpy(q).to(dev), torch.from_numpy(lab).to(dev)


def _busy_plan(b, preset, seed, h=256, w=256):
    """a sampled plan that warps something"""
    from pointcloududa_amd.utils.augment import GeoProgram, sample_heavy_plan
    rng = np.random.default_rng(seed)
    while True:
        plan = sample_heavy_plan(b, preset, rng, h, w)
        if any(isinstance(st, GeoProgram) and not st.is_identity() for st in plan.stages):
            return plan


@pytest.mark.parametrize("rescale", ["div255", None])
def test_augment_batch_with_a_plan_equals_heavy_aug_then_augment_batch(dev, rescale):
    from pointcloududa_amd.utils.augment import augment_batch, heavy_aug, sample_params
    q, lab, tq, tl = _loader_inputs(dev)
    params = sample_params(4, "mscmrseg_simple", np.random.default_rng(3))
    plan = _busy_plan(4, "heavy_device", 4)
    for crop, resample in ((224, True), (0, False)):
        one = augment_batch(tq, tl, params, 5, crop, rescale=rescale, resample_verts=resample, heavy=plan)
        hx, hl = heavy_aug(tq, tl, plan)
        assert hx.dtype == torch.uint8 and hl.dtype == tl.dtype and hl.shape == tl.shape
        two = augment_batch(hx, hl, params, 5, crop, rescale=rescale, resample_verts=resample)
        plain = augment_batch(tq, tl, params, 5, crop, rescale=rescale, resample_verts=resample)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
        assert not torch.equal(one[0], plain[0]) and not torch.equal(one[1], plain[1]), "images and masks both move"
        if resample:
            assert torch.equal(one[2], two[2]) and not torch.equal(one[2], plain[2])
    with pytest.raises(TypeError, match="uint8"):
        augment_batch(tq.float(), tl, params, 5, 0, rescale="minmax", heavy=plan)
    with pytest.raises(TypeError, match="uint8"):
        augment_batch(tq.float(), tl, params, 5, 0, rescale=None, heavy=plan)
    with pytest.raises(TypeError, match="plan is required"):
        heavy_aug(tq, tl)


def test_no_plan_is_bit_identical_to_the_call_without_the_argument(dev):
    from pointcloududa_amd.utils.augment import augment_batch, sample_params
    q, lab, tq, tl = _loader_inputs(dev)
    params = sample_params(4, "mmwhs_light", np.random.default_rng(6))
    params.affine_on[:2] = True
    tx = tq.float() / 3.0 - 20.0
    for img, rescale in ((tq, "div255"), (tq, None), (tx, "minmax"), (tx, None)):
        a = augment_batch(img, tl, params, 5, 224, rescale=rescale, resample_verts=True)
        b = augment_batch(img, tl, params, 5, 224, rescale=rescale, resample_verts=True, heavy=None)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("preset", ["heavy_device", "mscmrseg_aug2_device"])
def test_augmented_batches_with_a_heavy_preset_feed_train_epoch_shapes(dev, preset):
    from oracle.synth import synth_batch
    import make_photometric_golden as PG
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.augment import AugmentedBatches, AugmentParams, heavy_aug, sample_heavy_plan, upload_params
    from pointcloududa_amd.utils.npy2point import masks_to_pointclouds
    raw = []
    for i in range(3):
        lab = np.argmax(synth_batch(4, 1, 5, 256, seed=40 + i)[1], axis=1).astype(np.int64)[..., None]
        raw.append((PG.make_images("grey3", 4, 256, 256, 3, 50 + i), lab))
    it = AugmentedBatches(iter(raw), dev, None, np.random.default_rng(77), num_classes=5, crop_size=224, rescale="div255",
                          heavy_preset=preset)
    assert it.last_plan is None
    twin = np.random.default_rng(77)
    n = 0
    for (x, y, z), (img, lab) in zip(it, raw):
        assert x.dtype == torch.float32 and x.shape == (4, 3, 224, 224) and x.device.type == "cuda"
        assert y.dtype == torch.uint8 and y.shape == (4, 5, 224, 224) and z.dtype == torch.float32 and z.shape == (4, 300, 3)
        assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
        want = sample_heavy_plan(4, preset, twin, 256, 256)
        assert len(want.stages) == len(it.last_plan.stages) and it.last_params.is_identity()
        for a, b in zip(want.stages, it.last_plan.stages):
            assert type(a) is type(b)
            for k in ("opcode", "iarg", "farg", "seed"):
                assert np.array_equal(getattr(a, k), getattr(b, k)), k
        # the vertices are those of the warped full-size mask
        hx, hl = heavy_aug(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), want)
        assert hl.shape == (4, 256, 256, 1)
        full = (hl[..., 0] > 0).to(torch.uint8)
        verts = masks_to_pointclouds(full, torch.zeros(4, dtype=torch.int32, device=dev))
        # (a device tensor as divisor, as augment_batch divides: a Python scalar becomes a multiplication by 1 / 255)
        assert torch.equal(z, verts.to(torch.float32) / torch.full((), 255.0, dtype=torch.float32, device=dev))
        inv, order, cval = upload_params(AugmentParams.identity(4), 4, 256, 256, dev)
        ref = K.augment_assemble(hx, hl[..., 0].to(torch.int32), inv, order, cval, 5, 224, K.AUG_DIV255)
        assert torch.equal(x, ref["images"]) and torch.equal(y, ref["onehot"])
        n += 1
    assert n == 3


def test_the_heavy_path_adds_no_host_synchronisation(dev):
    """geometric_aug, heavy_aug and augment_batch(.., heavy=..) (resample_verts=False) under
    torch.cuda.set_sync_debug_mode("error"); the mode is first shown to be enforced (a ``.item()`` raises under it)"""
    from pointcloududa_amd.utils.augment import augment_batch, geometric_aug, heavy_aug, sample_geo_program
    q, lab, tq, tl = _loader_inputs(dev)
    plan = _busy_plan(4, "heavy_device", 4)
    prog = sample_geo_program(4, "heavy_device", np.random.default_rng(9), 256, 256)
    ref_g = geometric_aug(tq, tl, prog)                                                # (warm: allocator, library load)
    ref_h = heavy_aug(tq, tl, plan)
    ref = augment_batch(tq, tl, None, 5, 224, rescale="div255", heavy=plan)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        a = geometric_aug(tq, tl, prog)
        b = heavy_aug(tq, tl, plan)
        c = augment_batch(tq, tl, None, 5, 224, rescale="div255", heavy=plan)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a[0], ref_g[0]) and torch.equal(a[1], ref_g[1])
    assert torch.equal(b[0], ref_h[0]) and torch.equal(b[1], ref_h[1])
    assert torch.equal(c[0], ref[0]) and torch.equal(c[1], ref[1])


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_returns_status_codes(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd.utils.geometric import GeoProgram, upload_geo_program
    lib = _lib.lib()
    b, h, w, c = 2, 32, 48, 3
    x = torch.zeros((b, h, w, c), dtype=torch.uint8, device=dev)
    out = torch.full_like(x, 7)
    lab = torch.zeros((b, h, w), dtype=torch.int32, device=dev)
    lab_out = torch.full_like(lab, 7)
    op, ia, fa, sd = upload_geo_program(GeoProgram.identity(b, 8), b, h, w, dev)
    need = lib.pcuda_geometric_workspace_size(b, h, w, c, 1)
    assert need >= b * h * w * (c + 4) and need % 16 == 0 and lib.pcuda_geometric_workspace_size(0, h, w, c, 1) == 0
    assert b * h * w * c <= lib.pcuda_geometric_workspace_size(b, h, w, c, 0) < need
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(inp=x.data_ptr(), outp=out.data_ptr(), li=lab.data_ptr(), lo=lab_out.data_ptr(), b=b, h=h, w=w, c=c, slots=8,
             op=op.data_ptr(), wsp=ws.data_ptr(), nbytes=need):
        return lib.pcuda_geometric(inp, outp, li, lo, b, h, w, c, slots, op, ia.data_ptr(), fa.data_ptr(), sd.data_ptr(), wsp, nbytes,
                                   stream)
    assert call(outp=x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(lo=lab.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(slots=9) == -1 and b"slots" in lib.pcuda_last_error()
    assert call(slots=-1) == -1
    assert call(c=5) == -1 and b"channels" in lib.pcuda_last_error()
    assert call(h=1) == -1 and b"at least 2" in lib.pcuda_last_error()
    assert call(w=1) == -1 and b"at least 2" in lib.pcuda_last_error()
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(wsp=None) == -4
    for kw in (dict(inp=None), dict(outp=None), dict(b=0), dict(h=0), dict(w=-1), dict(c=0), dict(op=None), dict(li=None), dict(lo=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((lab_out == 7).all()), "a rejected call launches nothing"
    assert call() == 0 and call(slots=1, wsp=None, nbytes=0) == 0 and call(slots=0, op=None, wsp=None, nbytes=0) == 0
    assert call(li=None, lo=None, nbytes=lib.pcuda_geometric_workspace_size(b, h, w, c, 0)) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((lab_out == 0).all())
