"""Connected superpixels (csrc/spx_connect.hip) on the GPU, through the public surface
(utils/stylize.py, utils/augment.py) and the C ABI (pcuda_stylize_connect), against the committed fixture
tests/golden/spx_connect.npz and the digests tests/golden/spx_connect_digests.json (scripts/make_spx_connect_golden.py: a
vectorised restatement pinned by a sequential one).

Rule: the pass is integers only and the device equals the restatement bit for bit, with no excused pixel.  (In a program that
also holds NOISE_ALPHA_CONV3X3 slots those slots keep f9's excused set, which is the restatement's and empty in every case
here unless a test says otherwise.)"""
import hashlib
import importlib.util
import json
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


G = _load("make_spx_connect_golden")
CASES = G.load_cases(np.load(os.path.join(GOLD, "spx_connect.npz")))
NAMES = [c["name"] for c in CASES]
KEYS = ("opcode", "iarg", "farg", "table", "seed_arr")


def _case(name):
    return [c for c in CASES if c["name"] == name][0]


def _program(case, rows=None):
    from pointcloududa_amd.utils.stylize import StyleProgram
    rows = slice(None) if rows is None else rows
    return StyleProgram(*(np.ascontiguousarray(case[k][rows]) for k in KEYS))


def _arrays(prog, rows=slice(None), slots=slice(None)):
    return tuple(np.array(a[rows][:, slots], order="C", copy=True) for a in (prog.opcode, prog.iarg, prog.farg, prog.table, prog.seed))


def _run(dev, images, program):
    from pointcloududa_amd.utils.stylize import stylize_aug
    x = torch.from_numpy(images).to(dev)
    keep = x.clone()
    out = stylize_aug(x, program)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x, keep), "the input is never written"
    return out.cpu().numpy()


def _same(got, want, name):
    bad = got != want
    print("%s: %d values, %d differ" % (name, got.size, int(bad.sum())))
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(dev, name):
    """nine samples per shape: min_size in {1, superpixel_min_size, H W} x p_replace in {0, between, 1}"""
    case = _case(name)
    x = G.case_inputs(case)
    prog = _program(case)
    assert prog.needs_connect()
    got = _run(dev, x, prog)
    _same(got, case["u8"], name)
    h, w = case["h"], case["w"]
    mean = G.rdiv(x[8].astype(np.int64).reshape(h * w, -1).sum(0), h * w)
    assert np.all(got[8].reshape(h * w, -1) == mean), "min_size = H W with p_replace = 1 is the image's rdiv mean everywhere"
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[3], x[3]) and np.array_equal(got[6], x[6])


@pytest.mark.parametrize("name", ["production_n20", "production_n200"])
def test_production_size_by_digest(dev, name):
    """256 x 256 x 3, B = 2 (smooth with noise, uniform noise: chains of several hundred targets), 5 updates"""
    want = json.load(open(os.path.join(GOLD, "spx_connect_digests.json")))[name]
    case = [c for c in G.production_cases() if c["name"] == name][0]
    assert [case[k] for k in ("b", "h", "w", "c", "seed")] == want["dims"] and max(want["longest_chain"]) > 256
    p = case["prog"]
    from pointcloududa_amd.utils.stylize import StyleProgram
    got = _run(dev, G.case_inputs(case), StyleProgram(p.opcode, p.iarg, p.farg, p.table, p.seed))
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == want["sha256"]


# ---------------------------------------------------------------------------------------------- structure
def _mixed(rng, h, w):
    """B = 5, one slot: connected superpixels, unconnected superpixels, hue, NOP, connected superpixels with min_size 1"""
    from pointcloududa_amd.utils.stylize import StyleProgram, superpixel_min_size
    prog = StyleProgram.identity(5, 1)
    sd = lambda: int(rng.integers(0, 2 ** 63))
    prog.set_superpixels(0, 0, 6, 7, 0.8, sd(), min_size=superpixel_min_size(6, 7, h, w))
    prog.set_superpixels(1, 0, 6, 7, 0.8, sd())
    prog.set_hue_saturation(2, 0, 11, -17)
    prog.set_superpixels(4, 0, 5, 4, 0.6, sd(), iters=2, min_size=1)
    return prog


def test_a_mixed_batch_and_the_batch_position(dev):
    from pointcloududa_amd.utils.stylize import StyleProgram
    h, w, c = 50, 46, 3
    rng = np.random.default_rng(41)
    x = np.stack([G._noisy("smooth", h, w, c, 60 + i) for i in range(5)])
    prog = _mixed(rng, h, w)
    got = _run(dev, x, prog)
    want, exc = G.run_program(x, *_arrays(prog), backend="numpy", check=True)
    assert not exc.any()
    _same(got, want, "mixed batch")
    assert np.array_equal(got[3], x[3]) and not np.array_equal(got[0], x[0]) and not np.array_equal(got[4], x[4])
    # the unconnected sample is pcuda_stylize's, bit for bit, and the connected one differs from its unconnected run
    plain = StyleProgram(*_arrays(prog))
    plain.iarg[..., 5] = 0
    assert not plain.needs_connect()
    got_plain = _run(dev, x, plain)
    assert np.array_equal(got_plain[1:4], got[1:4]) and not np.array_equal(got_plain[0], got[0])
    for i in range(5):      # every sample alone, and at another position of a batch turned round
        one = _run(dev, x[i:i + 1], StyleProgram(*_arrays(prog, slice(i, i + 1))))
        assert np.array_equal(one[0], got[i]), i
    rev = _run(dev, np.ascontiguousarray(x[::-1]), StyleProgram(*_arrays(prog, slice(None, None, -1))))
    assert np.array_equal(rev[::-1], got)


def test_a_two_slot_chain_equals_two_one_slot_calls(dev):
    """connected superpixels, then noise-alpha (and the other way round in the second sample): the slots ping-pong between
    the output and the workspace, and the pass has to follow them"""
    from pointcloududa_amd.utils.stylize import StyleProgram, edge_detect_weights, simplex_grid, superpixel_min_size
    h, w, c = 64, 48, 3
    x = np.stack([G._noisy("smooth", h, w, c, 71), G._noisy("smooth", h, w, c, 72), G._noisy("random", h, w, c, 73)])
    prog = StyleProgram.identity(3, 2)
    for i, order in enumerate(((0, 1), (1, 0), (0, 1))):
        prog.set_superpixels(i, order[0], 5, 4, 0.9, 1000 + i, min_size=superpixel_min_size(5, 4, h, w) if i < 2 else h * w)
        prog.set_noise_alpha(i, order[1], edge_detect_weights(0.7137), [simplex_grid(5, 7, 90 + i)], 1, 2, True, 0.5)
    whole = _run(dev, x, prog)
    step = x
    for s in range(2):
        step = _run(dev, step, StyleProgram(*_arrays(prog, slots=slice(s, s + 1))))
    assert np.array_equal(whole, step)
    want, exc = G.run_program(x, *_arrays(prog), backend="numpy", check=True)
    assert not exc.any()      # (alpha is no round value: no pre-rounding value of the blend sits on a rounding boundary)
    _same(whole, want, "two slots")
    three = StyleProgram.identity(3, 3)      # an odd number of slots: the connected slot writes the workspace image
    for i in range(3):
        three.set_superpixels(i, 1, 5, 4, 1.0, 2000 + i, min_size=40)
        three.set_hue_saturation(i, 2, 9, 12)
    got3 = _run(dev, x, three)
    want3, exc3 = G.run_program(x, *_arrays(three), backend="numpy", check=True)
    assert not exc3.any()
    _same(got3, want3, "three slots")


def test_two_runs_give_the_same_bits(dev):
    case = _case("fragments_64x48x3")
    x, prog = G.case_inputs(case), _program(case)
    a, b = _run(dev, x, prog), _run(dev, x, prog)
    assert np.array_equal(a, b) and np.array_equal(a, case["u8"])


def test_the_connected_path_adds_no_host_synchronisation(dev):
    """stylize_aug on a connected program and heavy_aug on a connected plan under torch.cuda.set_sync_debug_mode("error"); the
    mode is first shown to be enforced (a ``.item()`` raises under it)"""
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import StyleProgram, heavy_aug, sample_heavy_plan, stylize_aug
    q = np.stack([G._noisy("smooth", 64, 64, 3, 80 + i) for i in range(4)])
    lab = np.argmax(synth_batch(4, 1, 5, 64, seed=5)[1], axis=1).astype(np.int64)
    tq, tl = torch.from_numpy(q).to(dev), torch.from_numpy(lab).to(dev)
    rng = np.random.default_rng(11)
    while True:
        plan = sample_heavy_plan(4, "heavy_connected_device", rng, 64, 64)
        style = [st for st in plan.stages if isinstance(st, StyleProgram) and st.needs_connect()]
        if style:
            break
    ref_s = stylize_aug(tq, style[0])                                              # (warm: allocator, library load)
    ref_h = heavy_aug(tq, tl, plan)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        a = stylize_aug(tq, style[0])
        hx, hl = heavy_aug(tq, tl, plan)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, ref_s) and torch.equal(hx, ref_h[0]) and torch.equal(hl, ref_h[1])


# ---------------------------------------------------------------------------------------------- presets
def test_a_sampled_connected_plan_matches_the_restatements(dev):
    """64 x 64 x 3, B = 8: sampled "heavy_connected_device" and "mscmrseg_aug2_connected_device" plans through heavy_aug's
    stages; every stylize stage against the restatement on the device's output of the stage before"""
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import (CropPadProgram, GeoProgram, PhotoProgram, StyleProgram, crop_pad_aug, geometric_aug,
                                                 heavy_aug, photometric_aug, sample_heavy_plan, stylize_aug)
    b, h, w, c = 8, 64, 64, 3
    x = np.stack([G._noisy("smooth", h, w, c, 90 + i) for i in range(b)])
    lab = np.argmax(synth_batch(b, 1, 5, 64, seed=9)[1], axis=1).astype(np.int64)
    for preset, seed in (("heavy_connected_device", 2031), ("mscmrseg_aug2_connected_device", 2032)):
        rng = np.random.default_rng(seed)
        while True:
            plan = sample_heavy_plan(b, preset, rng, h, w)
            if any(isinstance(st, StyleProgram) and st.needs_connect() for st in plan.stages):
                break
        tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
        connected = 0
        for k, st in enumerate(plan.stages):
            before = tx.cpu().numpy()
            if isinstance(st, StyleProgram):
                tx = stylize_aug(tx, st)
                want, exc = G.run_program(before, st.opcode, st.iarg, st.farg, st.table, st.seed, backend="numpy", check=True)
                got = tx.cpu().numpy()
                bad = (got != want) & ~exc
                print("%s stage %d: %d values, %d differ, %d excused" % (preset, k, got.size, int((got != want).sum()), int(exc.sum())))
                assert not bad.any() and exc.sum() <= 1e-5 * exc.size
                spx = (st.opcode == 3) & (st.iarg[..., 5] > 0)
                connected += int(spx.sum())
                for i in np.nonzero(spx.any(1))[0]:      # a sample with a connected slot has no excused pixel at all
                    if not (st.opcode[i] == 2).any():
                        assert np.array_equal(got[i], want[i])
            elif isinstance(st, PhotoProgram):
                tx = photometric_aug(tx, st)
            elif isinstance(st, GeoProgram):
                tx, tl = geometric_aug(tx, tl, st)
            else:
                assert isinstance(st, CropPadProgram)
                tx, tl = crop_pad_aug(tx, tl, st)
        assert connected > 0, preset
        hx, hl = heavy_aug(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), plan)
        assert torch.equal(hx, tx) and torch.equal(hl, tl)


def test_augmented_batches_take_the_connected_presets(dev):
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import AugmentedBatches, StyleProgram, sample_heavy_plan
    raw = []
    for i in range(3):
        lab = np.argmax(synth_batch(4, 1, 5, 64, seed=40 + i)[1], axis=1).astype(np.int64)[..., None]
        raw.append((np.stack([G._noisy("smooth", 64, 64, 3, 50 + 4 * i + j) for j in range(4)]), lab))
    for preset in ("heavy_connected_device", "mscmrseg_aug2_connected_device"):
        it = AugmentedBatches(iter(raw), dev, None, np.random.default_rng(72), num_classes=5, crop_size=56, rescale="div255",
                              heavy_preset=preset)
        twin = np.random.default_rng(72)
        seen = 0
        for x, y, z in it:
            assert x.dtype == torch.float32 and x.shape == (4, 3, 56, 56) and y.shape == (4, 5, 56, 56)
            want = sample_heavy_plan(4, preset, twin, 64, 64)
            assert [type(s) for s in want.stages] == [type(s) for s in it.last_plan.stages]
            for a, b2 in zip(want.stages, it.last_plan.stages):
                assert np.array_equal(a.opcode, b2.opcode) and np.array_equal(a.iarg, b2.iarg)
            seen += sum(isinstance(s, StyleProgram) and s.needs_connect() for s in want.stages)
        assert seen > 0, preset


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_returns_status_codes(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd.utils.stylize import StyleProgram, upload_style_program
    lib = _lib.lib()
    b, h, w, c = 2, 32, 48, 3
    x = torch.zeros((b, h, w, c), dtype=torch.uint8, device=dev)
    out = torch.full_like(x, 7)
    prog = StyleProgram.identity(b, 8)
    prog.set_superpixels(1, 3, 4, 5, 1.0, 5, min_size=20)
    up = upload_style_program(prog, b, h, w, c, dev)
    assert len(up) == 5
    op, ia, fa, tb, sd = up
    need, base = lib.pcuda_stylize_connect_workspace_size(b, h, w, c), lib.pcuda_stylize_workspace_size(b, h, w, c)
    assert need >= base + 4 * b * h * w and need % 16 == 0 and lib.pcuda_stylize_connect_workspace_size(0, h, w, c) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(inp=x.data_ptr(), outp=out.data_ptr(), b=b, h=h, w=w, c=c, slots=8, op=op.data_ptr(), tbp=tb.data_ptr(), wsp=ws.data_ptr(),
             nbytes=need):
        return lib.pcuda_stylize_connect(inp, outp, b, h, w, c, slots, op, ia.data_ptr(), fa.data_ptr(), tbp, sd.data_ptr(), wsp, nbytes,
                                         stream)
    assert call(outp=x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(slots=9) == -1 and b"slots" in lib.pcuda_last_error()
    assert call(slots=-1) == -1
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(nbytes=base) == -4, "pcuda_stylize's workspace is not enough"
    assert call(wsp=None) == -4 and call(slots=1, wsp=None, nbytes=0) == -4
    for kw in (dict(inp=None), dict(outp=None), dict(b=0), dict(h=0), dict(w=-1), dict(c=0), dict(c=5), dict(op=None), dict(tbp=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "a rejected call launches nothing"
    assert call() == 0 and call(slots=1) == 0 and call(slots=0, op=None, tbp=None, wsp=None, nbytes=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    # pcuda_stylize itself never reads iarg[5]: the same program through it is the unconnected result
    x2 = torch.from_numpy(np.stack([G._noisy("smooth", h, w, c, 3), G._noisy("smooth", h, w, c, 4)])).to(dev)
    o1, o2 = torch.empty_like(x2), torch.empty_like(x2)
    plain = StyleProgram(prog.opcode.copy(), prog.iarg.copy(), prog.farg, prog.table, prog.seed)
    plain.iarg[..., 5] = 0
    ia0 = upload_style_program(plain, b, h, w, c, dev)[1]
    args = lambda o, i: (x2.data_ptr(), o.data_ptr(), b, h, w, c, 8, op.data_ptr(), i.data_ptr(), fa.data_ptr(), tb.data_ptr(),
                         sd.data_ptr(), ws.data_ptr(), need, stream)
    assert lib.pcuda_stylize(*args(o1, ia)) == 0 and lib.pcuda_stylize(*args(o2, ia0)) == 0
    assert torch.equal(o1, o2)
    assert lib.pcuda_stylize_connect(*args(o2, ia)) == 0
    assert torch.equal(o1[0], o2[0]) and not torch.equal(o1[1], o2[1])
