"""Superpixels at a working size (csrc/spx_scale.hip) on the GPU, through the public surface
(utils/stylize.py, utils/augment.py, kernels.stylize_scaled) and the C ABI (pcuda_stylize_scaled), against the committed fixture
tests/golden/spx_scaled.npz and the digests tests/golden/spx_scaled_edges.json (scripts/make_spx_scaled_golden.py: a vectorised
restatement pinned by a sequential one).

Rule: the scaled slot is integers only and the device equals the restatement bit for bit, with no excused pixel.  The rule is
this build's own (imgaug, cv2 and skimage are not installed: parity with imgaug's max_size = 128 path is unpinned)."""
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


G = _load("make_spx_scaled_golden")
CASES = G.load_cases(np.load(os.path.join(GOLD, "spx_scaled.npz")))
NAMES = [c["name"] for c in CASES]
KEYS = ("opcode", "iarg", "farg", "table", "seed_arr")
noisy = G.F9B._noisy


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


def _want(images, prog, info=None):
    want, exc = G.run_program(images, *_arrays(prog), backend="numpy", info=info)
    assert not exc.any()
    return want


def _same(got, want, name):
    bad = got != want
    print("%s: %d values, %d differ" % (name, got.size, int(bad.sum())))
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(dev, name):
    """six samples per shape: p_replace in {0, between, 1} x two min_size (0 and superpixel_min_size, or superpixel_min_size and
    1 in the connected case): non-integer factors on both axes with w' = m exactly and odd working rows (40 x 56 x 3 -> 11 x
    16), a tall C = 1 image, odd sizes at C = 4 (no aligned store), the exact 2x case"""
    from pointcloududa_amd.utils.stylize import StyleProgram
    case = [c for c in CASES if c["name"] == name][0]
    x = G.case_inputs(case)
    prog = StyleProgram(*(np.ascontiguousarray(case[k]) for k in KEYS))
    assert prog.needs_scale(case["h"], case["w"]) and prog.needs_connect()
    got = _run(dev, x, prog)
    _same(got, case["u8"], name)
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[3], x[3]), "p_replace = 0: the input, not the blurred round trip"
    assert not np.array_equal(got[2], x[2]) and not np.array_equal(got[5], x[5])
    # p_replace = 1 replaces every segment: the output is the upscale of an image with at most gy gx (unconnected) colours
    # and differs from the same slot at full resolution
    full = StyleProgram(*_arrays(prog))
    full.iarg[..., 6] = 0
    full.iarg[..., 5] = np.minimum(full.iarg[..., 5], 1)      # (valid at either size)
    assert not full.needs_scale(case["h"], case["w"])
    got_full = _run(dev, x, full)
    assert not np.array_equal(got_full[2], got[2]) and not np.array_equal(got_full[5], got[5])
    assert np.array_equal(got_full[0], x[0])


@pytest.mark.parametrize("name", ["production_n20", "production_n200"])
def test_the_workloads_shape_by_digest(dev, name):
    """B = 2, 256 x 256 x 3, max_size 128, n_segments 20 and 200, connected"""
    from pointcloududa_amd.utils.stylize import StyleProgram
    want = json.load(open(os.path.join(GOLD, "spx_scaled_edges.json")))[name]
    case = [c for c in G.edge_cases() if c["name"] == name][0]
    assert [case[k] for k in ("b", "h", "w", "c", "seed")] == want["dims"] and want["working"] == [128, 128]
    p = case["prog"]
    prog = StyleProgram(p.opcode, p.iarg, p.farg, p.table, p.seed)
    assert prog.needs_scale(256, 256) and prog.needs_connect() and int(p.iarg[0, 0, 6]) == 128
    got = _run(dev, G.case_inputs(case), prog)
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == want["sha256"]


# ---------------------------------------------------------------------------------------------- unscaled programs
def test_programs_that_scale_nothing_equal_todays_entry_points(dev):
    """max_size = 0 and max_size >= max(H, W) through pcuda_stylize_scaled: kernels.stylize(.., connect=..) on the same program,
    bit for bit, for unconnected and connected slots, hue and noise-alpha"""
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.stylize import (StyleProgram, edge_detect_weights, simplex_grid, superpixel_min_size,
                                                 upload_style_program)
    h, w, c = 50, 46, 3
    x = torch.from_numpy(np.stack([noisy("smooth", h, w, c, 300 + i) for i in range(4)])).to(dev)
    for m in (0, 50, 51, 4000):
        prog = StyleProgram.identity(4, 2)
        prog.set_superpixels(0, 0, 6, 7, 0.8, 11, max_size=m)
        prog.set_superpixels(1, 1, 6, 7, 0.8, 12, min_size=superpixel_min_size(6, 7, h, w), max_size=m)
        prog.set_hue_saturation(2, 0, 11, -17)
        prog.set_noise_alpha(3, 1, edge_detect_weights(0.7137), [simplex_grid(5, 7, 90)], 1, 2, True, 0.5)
        prog.set_superpixels(3, 0, 5, 4, 0.6, 13, iters=2, min_size=1, max_size=m)
        assert not prog.needs_scale(h, w)
        up = upload_style_program(prog, 4, h, w, c, dev)
        got = K.stylize_scaled(x, *up)
        assert torch.equal(got, K.stylize(x, *up, connect=True)), m
        plain = StyleProgram(*_arrays(prog))
        plain.iarg[..., 5][plain.opcode == 3] = 0
        up0 = upload_style_program(plain, 4, h, w, c, dev)
        assert torch.equal(K.stylize_scaled(x, *up0), K.stylize(x, *up0)), m
        assert torch.equal(K.stylize(x, *up), K.stylize(x, *up0)), "pcuda_stylize reads neither iarg[5] nor iarg[6]"
    # ... and the two existing entry points never read iarg[6]
    prog = StyleProgram.identity(4, 1)
    for i in range(4):
        prog.set_superpixels(i, 0, 6, 7, 0.8, 20 + i, min_size=(0, 30)[i % 2], max_size=(16, 0)[i // 2])
    up = upload_style_program(prog, 4, h, w, c, dev)
    zero = StyleProgram(*_arrays(prog))
    zero.iarg[..., 6] = 0
    up0 = upload_style_program(zero, 4, h, w, c, dev)
    for connect in (False, True):
        assert torch.equal(K.stylize(x, *up, connect=connect), K.stylize(x, *up0, connect=connect))
    assert not torch.equal(K.stylize_scaled(x, *up)[:2], K.stylize(x, *up0, connect=True)[:2])


# ---------------------------------------------------------------------------------------------- structure
def _mixed(rng, h, w, m):
    """B = 5, one slot: scaled, unscaled superpixels, connected unscaled superpixels, hue, NOP"""
    from pointcloududa_amd.utils.stylize import StyleProgram, superpixel_min_size
    prog = StyleProgram.identity(5, 1)
    sd = lambda: int(rng.integers(0, 2 ** 63))
    prog.set_superpixels(0, 0, 3, 4, 0.8, sd(), max_size=m)
    prog.set_superpixels(1, 0, 6, 7, 0.8, sd())
    prog.set_superpixels(2, 0, 6, 7, 0.8, sd(), min_size=superpixel_min_size(6, 7, h, w))
    prog.set_hue_saturation(3, 0, 11, -17)
    return prog


def test_a_mixed_batch_and_the_batch_position(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.stylize import StyleProgram, upload_style_program
    h, w, c, m = 50, 46, 3, 20
    x = np.stack([noisy("smooth", h, w, c, 60 + i) for i in range(5)])
    prog = _mixed(np.random.default_rng(41), h, w, m)
    assert prog.needs_scale(h, w)
    info = []
    want = _want(x, prog, info)
    assert [d["sample"] for d in info] == [0] and info[0]["working"] == [20, 18] and info[0]["replaced"]
    got = _run(dev, x, prog)
    _same(got, want, "mixed batch")
    assert np.array_equal(got[4], x[4]) and all(not np.array_equal(got[i], x[i]) for i in range(4))
    # every sample takes its own path: the four that are not scaled are pcuda_stylize_connect's, bit for bit
    zero = StyleProgram(*_arrays(prog))
    zero.iarg[..., 6] = 0
    tx = torch.from_numpy(x).to(dev)
    today = K.stylize(tx, *upload_style_program(zero, 5, h, w, c, dev), connect=True).cpu().numpy()
    assert np.array_equal(today[1:], got[1:]) and not np.array_equal(today[0], got[0])
    for i in range(5):      # every sample alone, and at another position of a batch turned round
        one = _run(dev, x[i:i + 1], StyleProgram(*_arrays(prog, slice(i, i + 1))))
        assert np.array_equal(one[0], got[i]), i
    rev = _run(dev, np.ascontiguousarray(x[::-1]), StyleProgram(*_arrays(prog, slice(None, None, -1))))
    assert np.array_equal(rev[::-1], got)


@pytest.mark.parametrize("slots", [3, 4])
def test_two_scaled_slots_with_hue_between(dev, slots):
    """Superpixels, hue, Superpixels in the last three of 3 / 4 slots: the slots ping-pong between the output and the
    workspace (an odd and an even count), and the scaled slot has to follow them; the second sample is connected"""
    from pointcloududa_amd.utils.stylize import StyleProgram
    h, w, c, m = 40, 56, 3, 16
    x = np.stack([noisy("smooth", h, w, c, 71), noisy("smooth", h, w, c, 72), noisy("random", h, w, c, 73)])
    prog = StyleProgram.identity(3, slots)
    for i in range(3):
        prog.set_superpixels(i, slots - 3, 3, 4, 0.9, 1000 + i, min_size=(0, 7, 0)[i], max_size=m)
        prog.set_hue_saturation(i, slots - 2, 9, 12)
        prog.set_superpixels(i, slots - 1, 2, 5, (1.0, 0.7, 0.0)[i], 2000 + i, min_size=(0, 5, 1)[i], max_size=(m, m, 24)[i])
    whole = _run(dev, x, prog)
    _same(whole, _want(x, prog), "%d slots" % slots)
    step = x
    for s in range(slots):
        step = _run(dev, step, StyleProgram(*_arrays(prog, slots=slice(s, s + 1))))
    assert np.array_equal(whole, step)


def test_p_replace_zero_is_the_input_and_one_replaces_every_segment(dev):
    from pointcloududa_amd.utils.stylize import StyleProgram
    h, w, c, m = 40, 56, 3, 16
    x = np.stack([noisy("smooth", h, w, c, 81 + i) for i in range(4)])
    prog = StyleProgram.identity(4, 1)
    for i in range(4):
        prog.set_superpixels(i, 0, 3, 4, (0.0, 1.0)[i % 2], 500 + i, min_size=(0, 7)[i // 2], max_size=m)
    got = _run(dev, x, prog)
    _same(got, _want(x, prog), "p_replace 0 / 1")
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[2], x[2])
    for i in (1, 3):      # every segment replaced: the image is R(painted), and painted has at most gy gx colours
        small = G.resize_numpy(x[i], 11, 16).astype(np.uint8)
        lab = G.F9.slic_numpy(small, 3, 4, 5, 100)[0]
        if i == 3:
            painted = G.F9B.connect_numpy(small, lab, 7, 2 ** 32 - 1, 500 + i)[0]
        else:
            painted = G.F9.superpixels_numpy(small, 3, 4, 5, 100, 2 ** 32 - 1, 500 + i)[0]
        if i == 1:
            assert len(np.unique(painted.reshape(-1, c), axis=0)) <= 12
        assert np.array_equal(got[i], G.resize_numpy(painted.astype(np.uint8), h, w))
    full = StyleProgram(*_arrays(prog))
    full.iarg[..., 6] = 0
    got_full = _run(dev, x, full)
    assert not np.array_equal(got_full[1], got[1]) and not np.array_equal(got_full[3], got[3])


def test_views_offset_by_one_byte(dev):
    """``in`` and ``out`` one byte behind a 16-byte boundary: no aligned vector load or store applies"""
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.stylize import StyleProgram, upload_style_program
    b, h, w, c, m = 3, 33, 47, 4, 20
    x = np.stack([noisy("smooth", h, w, c, 91 + i) for i in range(b)])
    prog = StyleProgram.identity(b, 2)
    prog.set_superpixels(0, 0, 4, 5, 0.8, 31, max_size=m)
    prog.set_superpixels(1, 1, 4, 5, 0.8, 32, min_size=7, max_size=m)
    prog.set_superpixels(2, 0, 4, 5, 0.8, 33, min_size=9)
    n = x.size
    src, dst = torch.zeros(n + 32, dtype=torch.uint8, device=dev), torch.full((n + 32,), 201, dtype=torch.uint8, device=dev)
    xin, out = src[17:17 + n].view(b, h, w, c), dst[1:1 + n].view(b, h, w, c)
    assert xin.data_ptr() % 16 == 1 and out.data_ptr() % 16 == 1
    xin.copy_(torch.from_numpy(x))
    got = K.stylize_scaled(xin, *upload_style_program(prog, b, h, w, c, dev), out=out)
    assert got.data_ptr() == out.data_ptr()
    _same(got.cpu().numpy(), _want(x, prog), "offset views")
    assert bool((dst[:1] == 201).all()) and bool((dst[1 + n:] == 201).all()), "nothing outside the view is written"
    assert np.array_equal(xin.cpu().numpy(), x)


def test_two_runs_give_the_same_bits(dev):
    from pointcloududa_amd.utils.stylize import StyleProgram
    case = CASES[2]
    x, prog = G.case_inputs(case), StyleProgram(*(np.ascontiguousarray(case[k]) for k in KEYS))
    a, b = _run(dev, x, prog), _run(dev, x, prog)
    assert np.array_equal(a, b) and np.array_equal(a, case["u8"])


# ---------------------------------------------------------------------------------------------- presets
def test_a_sampled_scaled_plan_matches_the_restatements(dev):
    """64 x 64 x 3, B = 4: a sampled "heavy_scaled_device" plan through heavy_aug's stages; every stylize stage against the
    restatement on the device's output of the stage before.  (At 64 x 64 max_size = 128 scales nothing: the plan runs the
    connected path; the same plan with max_size lowered to 32 runs the scaled one.)"""
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import (CropPadProgram, GeoProgram, PhotoProgram, StyleProgram, crop_pad_aug, geometric_aug,
                                                 heavy_aug, photometric_aug, sample_heavy_plan, stylize_aug)
    from pointcloududa_amd.utils.stylize import superpixel_grid, superpixel_min_size
    b, h, w, c = 4, 64, 64, 3
    x = np.stack([noisy("smooth", h, w, c, 90 + i) for i in range(b)])
    lab = np.argmax(synth_batch(b, 1, 5, 64, seed=9)[1], axis=1).astype(np.int64)
    rng = np.random.default_rng(2041)
    while True:
        plan = sample_heavy_plan(b, "heavy_scaled_device", rng, h, w)
        if any(isinstance(st, StyleProgram) and (st.opcode == 3).any() for st in plan.stages):
            break
    for lowered in (False, True):
        if lowered:      # the same draws at max_size = 32: the grid and min_size re-encoded for the 32 x 32 working size
            for st in plan.stages:
                if isinstance(st, StyleProgram):
                    for i, s in zip(*np.nonzero(st.opcode == 3)):
                        gy, gx = superpixel_grid(int(st.iarg[i, s, 0]) * int(st.iarg[i, s, 1]), 32, 32)
                        st.iarg[i, s, 0:2], st.iarg[i, s, 5], st.iarg[i, s, 6] = (gy, gx), superpixel_min_size(gy, gx, 32, 32), 32
        tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
        spx = 0
        for k, st in enumerate(plan.stages):
            before = tx.cpu().numpy()
            if isinstance(st, StyleProgram):
                assert st.needs_scale(h, w) == (lowered and bool((st.opcode == 3).any()))
                assert np.all(st.iarg[st.opcode == 3][:, 6] == (32 if lowered else 128))
                tx = stylize_aug(tx, st)
                want, exc = G.run_program(before, st.opcode, st.iarg, st.farg, st.table, st.seed, backend="numpy")
                got = tx.cpu().numpy()
                bad = (got != want) & ~exc
                print("stage %d: %d values, %d differ, %d excused" % (k, got.size, int((got != want).sum()), int(exc.sum())))
                assert not bad.any() and exc.sum() <= 1e-5 * exc.size
                spx += int((st.opcode == 3).sum())
            elif isinstance(st, PhotoProgram):
                tx = photometric_aug(tx, st)
            elif isinstance(st, GeoProgram):
                tx, tl = geometric_aug(tx, tl, st)
            else:
                assert isinstance(st, CropPadProgram)
                tx, tl = crop_pad_aug(tx, tl, st)
        assert spx > 0
        hx, hl = heavy_aug(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), plan)
        assert torch.equal(hx, tx) and torch.equal(hl, tl)


def test_augmented_batches_take_the_scaled_presets(dev):
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import AugmentedBatches, StyleProgram, sample_heavy_plan
    raw = []
    for i in range(2):
        lab = np.argmax(synth_batch(2, 1, 5, 160, seed=40 + i)[1], axis=1).astype(np.int64)[..., None]
        raw.append((np.stack([noisy("smooth", 160, 160, 3, 50 + 2 * i + j) for j in range(2)]), lab))
    for preset, seed in (("heavy_scaled_device", 63), ("mscmrseg_aug2_scaled_device", 60)):
        it = AugmentedBatches(iter(raw), dev, None, np.random.default_rng(seed), num_classes=5, crop_size=144, rescale="div255",
                              heavy_preset=preset)
        twin = np.random.default_rng(seed)
        seen = 0
        for x, y, z in it:
            assert x.dtype == torch.float32 and x.shape == (2, 3, 144, 144) and y.shape == (2, 5, 144, 144)
            want = sample_heavy_plan(2, preset, twin, 160, 160)
            assert [type(s) for s in want.stages] == [type(s) for s in it.last_plan.stages]
            for a, b2 in zip(want.stages, it.last_plan.stages):
                assert np.array_equal(a.opcode, b2.opcode) and np.array_equal(a.iarg, b2.iarg)
                if isinstance(a, StyleProgram):
                    assert np.all(a.iarg[a.opcode == 3][:, 6] == 128)
                    seen += int(a.needs_scale(160, 160))
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
    prog.set_superpixels(1, 3, 4, 5, 1.0, 5, min_size=20, max_size=24)
    op, ia, fa, tb, sd = upload_style_program(prog, b, h, w, c, dev)
    need, conn = lib.pcuda_stylize_scaled_workspace_size(b, h, w, c), lib.pcuda_stylize_connect_workspace_size(b, h, w, c)
    assert need >= conn + 2 * b * h * w * c + 4 * b and need % 16 == 0 and lib.pcuda_stylize_scaled_workspace_size(b, 0, w, c) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(inp=x.data_ptr(), outp=out.data_ptr(), b=b, h=h, w=w, c=c, slots=8, op=op.data_ptr(), tbp=tb.data_ptr(), wsp=ws.data_ptr(),
             nbytes=need):
        return lib.pcuda_stylize_scaled(inp, outp, b, h, w, c, slots, op, ia.data_ptr(), fa.data_ptr(), tbp, sd.data_ptr(), wsp, nbytes,
                                        stream)
    assert call(outp=x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(slots=9) == -1 and b"slots" in lib.pcuda_last_error()
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(nbytes=conn) == -4, "pcuda_stylize_connect's workspace is not enough"
    assert call(wsp=None) == -4 and call(slots=1, wsp=None, nbytes=0) == -4
    for kw in (dict(inp=None), dict(outp=None), dict(b=0), dict(h=0), dict(w=-1), dict(c=0), dict(c=5), dict(op=None), dict(tbp=None)):
        assert call(**kw) == -1, kw
    assert call(h=4097, w=4096) == -1 and b"2^24" in lib.pcuda_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "a rejected call launches nothing"
    assert call() == 0 and call(slots=1) == 0 and call(slots=0, op=None, tbp=None, wsp=None, nbytes=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
