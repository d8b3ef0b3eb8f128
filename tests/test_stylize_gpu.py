"""Device-side stylize augmentation on the GPU, through the public surface (utils/augment.py,
utils/stylize.py) and the C ABI, against the committed fixture tests/golden/stylize.npz (scripts/make_stylize_golden.py: a
vectorised numpy restatement pinned by an independent one) and, at the production size, against the numpy restatements of
f7, f8 and f9 stage by stage.  scipy is not needed here.

Rule: HUE_SATURATION and SUPERPIXELS are integer operators and bit-identical.  NOISE_ALPHA_CONV3X3 equals the restatement
except at EXCUSED pixels (the 3x3 correlation's or the blend's pre-rounding value within 1e-9 of a rounding boundary, or such
a pixel in the dependency window), which may differ by one grey level; the excused set is the restatement's, never the
device's.  The fixture has no excused pixel at all."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


def _load(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return m


G = _load("make_stylize_golden")
CASES = G.load_cases(np.load(os.path.join(GOLD, "stylize.npz")))
NAMES = [c["name"] for c in CASES]
KEYS = ("opcode", "iarg", "farg", "table", "seed_arr")


def _case(name):
    return [c for c in CASES if c["name"] == name][0]


def _program(case, rows=None, slots=None):
    from pointcloududa_amd.utils.stylize import StyleProgram
    rows = slice(None) if rows is None else rows
    slots = slice(None) if slots is None else slots
    return StyleProgram(*(np.ascontiguousarray(case[k][rows][:, slots]) for k in KEYS))


def _run(dev, images, program):
    from pointcloududa_amd.utils.stylize import stylize_aug
    x = torch.from_numpy(images).to(dev)
    keep = x.clone()
    out = stylize_aug(x, program)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x, keep), "the input is never written"
    return out.cpu().numpy()


def _check(got, want, exc, name, step=1):
    bad = (got != want) & ~exc
    print("%s: %d values, %d differ, %d of them outside the excused set (%d excused)" % (
        name, got.size, int((got != want).sum()), int(bad.sum()), int(exc.sum())))
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    if step:
        assert np.abs(got.astype(int) - want.astype(int)).max() <= step, name


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
    from pointcloududa_amd.utils.stylize import StyleProgram, upload_style_program
    x = np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)
    b, h, w, c = shape
    for slots in (0, 1, 2, 5, 8):
        prog = StyleProgram.identity(b, slots)
        assert prog.is_identity()
        assert np.array_equal(_run(dev, x, prog), x), slots
    # an unknown opcode on the device behaves as NOP (the host validates programs: this goes below it)
    arrays = upload_style_program(StyleProgram.identity(b, 3), b, h, w, c, dev)
    op = arrays[0].clone()
    op[:, 1] = 99
    op[:, 2] = -7
    tx = torch.from_numpy(x).to(dev)
    assert torch.equal(K.stylize(tx, op, *arrays[1:]), tx)


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


def test_the_result_does_not_depend_on_the_batch_position(dev):
    """one sample alone against the same sample and slots at index 19 of a batch of 32 (every sample its own program)"""
    from pointcloududa_amd.utils.stylize import (StyleProgram, directed_edge_weights, edge_detect_weights, simplex_grid)
    h, w, c = 96, 80, 3
    rng = np.random.default_rng(33)
    big = rng.integers(0, 256, (32, h, w, c), dtype=np.uint8)
    big[16:] = G.make_images("smooth", 16, h, w, c, 7)
    prog = StyleProgram.identity(32, 3)
    for i in range(32):
        order = rng.permutation(3)
        sd = lambda: int(rng.integers(0, 2 ** 63))
        prog.set_superpixels(i, order[0], int(rng.integers(1, 13)), int(rng.integers(1, 13)), rng.uniform(0.3, 1), sd())
        wts = edge_detect_weights(rng.uniform(0.5, 1)) if i % 2 else directed_edge_weights(rng.uniform(0.5, 1), rng.uniform(0, 1))
        grids = [simplex_grid(int(rng.integers(2, 17)), int(rng.integers(2, 17)), sd()) for _ in range(1 + i % 3)]
        prog.set_noise_alpha(i, order[1], wts, grids, i % 2, i % 3, bool((i // 2) % 2), rng.normal(0, 5))
        prog.set_hue_saturation(i, order[2], int(rng.integers(-14, 15)), int(rng.integers(-20, 21)))
    arrays = (prog.opcode, prog.iarg, prog.farg, prog.table, prog.seed)
    one = StyleProgram(*(np.ascontiguousarray(a[19:20]) for a in arrays))
    got_big, got_one = _run(dev, big, prog), _run(dev, big[19:20], one)
    assert np.array_equal(got_big[19], got_one[0])
    assert not np.array_equal(got_big[19], got_big[18]) and not np.array_equal(got_one[0], big[19])
    want, exc = G.run_program(big, *arrays, backend="numpy")
    _check(got_big, want, exc, "batch of 32")


def test_production_size_sampled_full_plan_matches_the_restatements(dev):
    """B = 32, 256 x 256 x 3 with labels, a sampled "heavy_full_device" plan through heavy_aug's stages: every stage against its
    numpy restatement (f7's, f8's, f9's) on the device's output of the stage before; then the same plan through heavy_aug and
    augment_batch(.., heavy=plan)"""
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import (GeoProgram, PhotoProgram, StyleProgram, augment_batch, geometric_aug, heavy_aug,
                                                 photometric_aug, sample_heavy_plan, sample_params, stylize_aug)
    PG, GG = _load("make_photometric_golden"), _load("make_geometric_golden")
    b, h, w, c = 32, 256, 256, 3
    x = np.concatenate([G.make_images("grey3", 16, h, w, c, 91), G.make_images("smooth", 8, h, w, c, 92),
                        G.make_images("random", 8, h, w, c, 93)])
    lab = np.argmax(synth_batch(b, 1, 5, 256, seed=9)[1], axis=1).astype(np.int64)
    plan = sample_heavy_plan(b, "heavy_full_device", np.random.default_rng(2029), h, w)
    style = [st for st in plan.stages if isinstance(st, StyleProgram)]
    assert set(np.concatenate([st.opcode.ravel() for st in style])) >= {1, 2, 3}
    assert any(isinstance(st, GeoProgram) for st in plan.stages) and any(isinstance(st, PhotoProgram) for st in plan.stages)
    tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    for k, st in enumerate(plan.stages):
        before, before_lab = tx.cpu().numpy(), tl.cpu().numpy()
        if isinstance(st, StyleProgram):
            tx = stylize_aug(tx, st)
            want, exc = G.run_program(before, st.opcode, st.iarg, st.farg, st.table, st.seed, backend="numpy")
            _check(tx.cpu().numpy(), want, exc, "stage %d (stylize, %d slots)" % (k, st.slots))
            assert exc.sum() <= 1e-5 * exc.size
        elif isinstance(st, PhotoProgram):
            tx = photometric_aug(tx, st)
            want, exc = PG.run_program(before, st.opcode, st.iarg, st.farg, st.seed, backend="numpy")
            _check(tx.cpu().numpy(), want, exc, "stage %d (photometric, %d slots)" % (k, st.slots))
        else:
            tx, tl = geometric_aug(tx, tl, st)
            cur, cur_lab = before, before_lab
            for s in range(st.slots):      # one slot at a time from the device's own intermediate values (f8's rule)
                one = GeoProgram(*(np.ascontiguousarray(a[:, s:s + 1]) for a in (st.opcode, st.iarg, st.farg, st.seed)))
                w1, wl1, e1, el1, _ = GG.run_program(cur, cur_lab, one.opcode, one.iarg, one.farg, one.seed, backend="numpy")
                gx, gl = geometric_aug(torch.from_numpy(cur).to(dev), torch.from_numpy(cur_lab).to(dev), one)
                cur, cur_lab = gx.cpu().numpy(), gl.cpu().numpy()
                _check(cur, w1, e1, "stage %d slot %d (geometric)" % (k, s), step=0)
                _check(cur_lab, wl1, el1, "stage %d slot %d labels" % (k, s), step=0)
            assert np.array_equal(cur, tx.cpu().numpy()) and np.array_equal(cur_lab, tl.cpu().numpy())
    hx, hl = heavy_aug(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), plan)
    assert torch.equal(hx, tx) and torch.equal(hl, tl)
    assert not torch.equal(hl.cpu(), torch.from_numpy(lab))
    params = sample_params(b, "mscmrseg_simple", np.random.default_rng(3))
    one = augment_batch(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), params, 5, 224, rescale="div255", heavy=plan)
    two = augment_batch(hx, hl, params, 5, 224, rescale="div255")
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


def test_augmented_batches_take_the_full_presets(dev):
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import AugmentedBatches, StyleProgram, sample_heavy_plan
    raw = []
    for i in range(4):
        lab = np.argmax(synth_batch(4, 1, 5, 256, seed=40 + i)[1], axis=1).astype(np.int64)[..., None]
        raw.append((G.make_images("grey3", 4, 256, 256, 3, 50 + i), lab))
    for preset in ("heavy_full_device", "mscmrseg_aug2_full_device"):
        it = AugmentedBatches(iter(raw), dev, None, np.random.default_rng(78), num_classes=5, crop_size=224, rescale="div255",
                              heavy_preset=preset)
        twin = np.random.default_rng(78)
        seen = 0
        for x, y, z in it:
            assert x.dtype == torch.float32 and x.shape == (4, 3, 224, 224) and y.shape == (4, 5, 224, 224) and z.shape == (4, 300, 3)
            want = sample_heavy_plan(4, preset, twin, 256, 256)
            assert [type(s) for s in want.stages] == [type(s) for s in it.last_plan.stages]
            for a, b2 in zip(want.stages, it.last_plan.stages):
                assert np.array_equal(a.opcode, b2.opcode) and np.array_equal(a.farg, b2.farg)
            seen += sum(isinstance(s, StyleProgram) for s in want.stages)
        assert seen > 0, preset


def test_the_stylize_path_adds_no_host_synchronisation(dev):
    """stylize_aug, heavy_aug and augment_batch(.., heavy=plan) (resample_verts=False) under
    torch.cuda.set_sync_debug_mode("error"); the mode is first shown to be enforced (a ``.item()`` raises under it)"""
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import StyleProgram, augment_batch, heavy_aug, sample_heavy_plan, sample_params, stylize_aug
    q = G.make_images("grey3", 4, 256, 256, 3, 5)
    lab = np.argmax(synth_batch(4, 1, 5, 256, seed=5)[1], axis=1).astype(np.int64)
    tq, tl = torch.from_numpy(q).to(dev), torch.from_numpy(lab).to(dev)
    rng = np.random.default_rng(11)
    while True:
        plan = sample_heavy_plan(4, "heavy_full_device", rng, 256, 256)
        style = [st for st in plan.stages if isinstance(st, StyleProgram)]
        if style and len(set(np.concatenate([st.opcode.ravel() for st in style])) - {0}) >= 2:
            break
    params = sample_params(4, "mscmrseg_simple", np.random.default_rng(3))
    ref_s = stylize_aug(tq, style[0])                                              # (warm: allocator, library load)
    ref_h = heavy_aug(tq, tl, plan)
    ref = augment_batch(tq, tl, params, 5, 224, rescale="div255", heavy=plan)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        a = stylize_aug(tq, style[0])
        hx, hl = heavy_aug(tq, tl, plan)
        b = augment_batch(tq, tl, params, 5, 224, rescale="div255", heavy=plan)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, ref_s) and torch.equal(hx, ref_h[0]) and torch.equal(hl, ref_h[1])
    assert torch.equal(b[0], ref[0]) and torch.equal(b[1], ref[1])


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_returns_status_codes(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd.utils.stylize import StyleProgram, upload_style_program
    lib = _lib.lib()
    b, h, w, c = 2, 32, 48, 3
    x = torch.zeros((b, h, w, c), dtype=torch.uint8, device=dev)
    out = torch.full_like(x, 7)
    op, ia, fa, tb, sd = upload_style_program(StyleProgram.identity(b, 8), b, h, w, c, dev)
    need = lib.pcuda_stylize_workspace_size(b, h, w, c)
    assert need >= b * h * w * (c + 1) and need % 16 == 0 and lib.pcuda_stylize_workspace_size(0, h, w, c) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(inp=x.data_ptr(), outp=out.data_ptr(), b=b, h=h, w=w, c=c, slots=8, op=op.data_ptr(), tbp=tb.data_ptr(), wsp=ws.data_ptr(),
             nbytes=need):
        return lib.pcuda_stylize(inp, outp, b, h, w, c, slots, op, ia.data_ptr(), fa.data_ptr(), tbp, sd.data_ptr(), wsp, nbytes, stream)
    assert call(outp=x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(slots=9) == -1 and b"slots" in lib.pcuda_last_error()
    assert call(slots=-1) == -1
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(wsp=None) == -4 and call(slots=1, wsp=None, nbytes=0) == -4
    for kw in (dict(inp=None), dict(outp=None), dict(b=0), dict(h=0), dict(w=-1), dict(c=0), dict(c=5), dict(op=None), dict(tbp=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "a rejected call launches nothing"
    assert call() == 0 and call(slots=1) == 0 and call(slots=0, op=None, tbp=None, wsp=None, nbytes=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
