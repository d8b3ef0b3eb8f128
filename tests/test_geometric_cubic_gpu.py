"""Order 3 of the device-side geometric augmentation on the GPU, through the public surface and
``K.geometric(.., cubic=..)``, against the NUMPY restatement of scripts/make_geometric_cubic_golden.py.

Rule: bit for bit at every value, with no excused value -- both sides execute the same IEEE float64 operations in the same
order.  (The fixture's own excusable set, where the numpy restatement could leave the exact one, is empty.)  Nothing here
provokes a fault: every program is a valid one."""
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


C = _load("make_geometric_cubic_golden")
CASES = C.load_cases(np.load(os.path.join(GOLD, "geometric_cubic.npz")))
NAMES = [c["name"] for c in CASES]


def _case(name):
    return [c for c in CASES if c["name"] == name][0]


def _program(arrays, slots=None):
    from pointcloududa_amd.utils.geometric import GeoProgram
    slots = slice(None) if slots is None else slots
    return GeoProgram(*(np.ascontiguousarray(a[:, slots]) for a in arrays))


def _arrays(case):
    return case["opcode"], case["iarg"], case["farg"], case["seed_arr"]


def _run(dev, images, labels, program):
    from pointcloududa_amd.utils.geometric import geometric_aug
    x, l = torch.from_numpy(images).to(dev), torch.from_numpy(labels).to(dev)
    kx, kl = x.clone(), l.clone()
    out, lab = geometric_aug(x, l, program)
    assert out.dtype == torch.uint8 and out.shape == x.shape and lab.dtype == l.dtype and lab.shape == l.shape
    assert torch.equal(x, kx) and torch.equal(l, kl), "the inputs are never written"
    return out.cpu().numpy(), lab.cpu().numpy()


def _same(got, want, name):
    diff = got != want
    print("%s: %d values, %d differ" % (name, got.size, int(diff.sum())))
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[diff][:5].tolist(), want[diff][:5].tolist())


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(dev, name):
    case = _case(name)
    assert len(case["exc"]) == 0
    prog = _program(_arrays(case))
    assert prog.uses_cubic()
    got, lab = _run(dev, case["images"], case["labels"], prog)
    _same(got, case["u8"], name)
    _same(lab, case["lab"], name + " labels")
    if case["chain"]:      # slot by slot, from the device's own intermediate values
        cur, cur_lab = case["images"], case["labels"]
        for s in range(case["opcode"].shape[1]):
            one = tuple(np.ascontiguousarray(a[:, s:s + 1]) for a in _arrays(case))
            want, want_lab, _, _ = C.run_program(cur, cur_lab, *one, backend="numpy")
            cur, cur_lab = _run(dev, cur, cur_lab, _program(one))
            _same(cur, want, "%s slot %d" % (name, s))
            _same(cur_lab, want_lab, "%s slot %d labels" % (name, s))
        assert np.array_equal(cur, got) and np.array_equal(cur_lab, lab)
    if case["kind"] == "stripes":
        assert (got == 0).any() and (got == 255).any()


# ---------------------------------------------------------------------------------------------- small shapes
def _mixed_program(b, h, w, rng, order=3):
    """one slot per sample, the opcodes and the five modes in turn, parameters from the reference's ranges"""
    prog = C.Prog(b)
    for i in range(b):
        mode, cval = i % 5, int(rng.integers(1, 256))
        kind = (i // 5) % 4
        if kind == 0:
            m = C.G.affine_inverse(h, w, rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2),
                                   rng.uniform(-45, 45), rng.uniform(-16, 16))
            prog.homography(i, 0, m, order, mode, cval)
        elif kind == 1:
            prog.elastic(i, 0, float(rng.uniform(0.5, 3.5)), (0.25, 1.0, 0.1)[i % 3], int(rng.integers(0, 2 ** 63)), order, mode, cval)
        elif kind == 2:
            g = 2 + i % 3
            prog.piecewise(i, 0, h, w, rng.normal(0, 0.05 * w, (g, g)), rng.normal(0, 0.05 * h, (g, g)), order, mode, cval)
        else:
            prog.homography(i, 0, C.G.perspective(h, w, rng.normal(0, 0.08, (4, 2)).clip(-0.45, 0.45)), order, mode, cval)
    return prog


def _k_run(dev, x, lab, prog, cubic, shift_in=0, shift_out=0):
    """K.geometric on tensors whose first byte sits ``shift`` bytes behind an aligned address"""
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.geometric import upload_geo_program
    b, h, w, c = x.shape
    up = upload_geo_program(_program((prog.opcode, prog.iarg, prog.farg, prog.seed)), b, h, w, dev)
    n = x.size
    buf_in = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    buf_out = torch.full((n + 16,), 0xAB, dtype=torch.uint8, device=dev)
    tx = buf_in[shift_in:shift_in + n].view(b, h, w, c)
    tx.copy_(torch.from_numpy(x).to(dev))
    to = buf_out[shift_out:shift_out + n].view(b, h, w, c)
    assert tx.data_ptr() % 16 == shift_in and to.data_ptr() % 16 == shift_out
    tl = torch.from_numpy(lab.astype(np.int32)).to(dev)
    out, lab_out = K.geometric(tx, tl, *up, out=to, cubic=cubic)
    assert out.data_ptr() == to.data_ptr()
    guard = torch.cat([buf_out[:shift_out], buf_out[shift_out + n:]])
    assert bool((guard == 0xAB).all()), "bytes outside the output were written"
    return out.cpu().numpy(), lab_out.cpu().numpy().astype(np.int64)


# 18x65: two x tiles, a ragged last lane group, the scalar store path; 20x68: the 32-bit-word store path; 2x2, 2x5, 3x3: the
# 4 x 4 footprint is larger than the image, every fold mode wraps more than once
@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", [(18, 65), (20, 68), (2, 2), (2, 5), (3, 3)])
def test_small_shapes_match_the_numpy_restatement(dev, hw, c):
    h, w = hw
    b = 20
    rng = np.random.default_rng(100 * h + w + c)
    x = rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)
    lab = rng.integers(0, 5, (b, h, w)).astype(np.int64)
    prog = _mixed_program(b, h, w, rng)
    want, want_lab, _, _ = C.run_program(x, lab, prog.opcode, prog.iarg, prog.farg, prog.seed, backend="numpy")
    assert not np.array_equal(want, x)
    for shift_in, shift_out in ((0, 0), (1, 0), (0, 1), (1, 1)):
        got, got_lab = _k_run(dev, x, lab, prog, True, shift_in, shift_out)
        _same(got, want, "%dx%dx%d in+%d out+%d" % (h, w, c, shift_in, shift_out))
        _same(got_lab, want_lab, "%dx%dx%d labels" % (h, w, c))


def test_stripes_reach_both_clips(dev):
    h, w = 18, 65
    x = np.repeat(C.stripes_image(h, w, 3), 3, axis=0)
    lab = np.random.default_rng(0).integers(0, 5, (3, h, w)).astype(np.int64)
    prog = C.Prog(3)
    prog.homography(0, 0, np.array([[1.0, 0.0, 0.37], [0.0, 1.0, 0.21], [0.0, 0.0, 1.0]]), 3, C.EDGE, 0)
    prog.homography(1, 0, C.G.affine_inverse(h, w, 1.1, 0.9, 0.02, -0.03, 11.0, 4.0), 3, C.SYMMETRIC, 0)
    prog.elastic(2, 0, 3.5, 0.25, 99, 3, C.WRAP, 0)
    want = np.empty_like(x)
    lo, hi = 0.0, 255.0
    for i in range(3):
        sx, sy = C.G.source_coords(int(prog.opcode[i, 0]), prog.iarg[i, 0], prog.farg[i, 0], int(prog.seed[i, 0]), h, w)
        v, _ = C.sample_cubic_numpy(x[i], lab[i], sx, sy, int(prog.iarg[i, 0, 1]), 0)
        lo, hi, want[i] = min(lo, v.min()), max(hi, v.max()), C.G.to_u8(v)
    assert lo < -0.5 and hi >= 255.5, "the restatement reaches both clips before it rounds"
    got, _ = _run(dev, x, lab, _program((prog.opcode, prog.iarg, prog.farg, prog.seed)))
    _same(got, want, "stripes")


# ---------------------------------------------------------------------------------------------- anchors, the two entries
@pytest.mark.parametrize("shape", [(2, 18, 65, 3), (2, 3, 3, 1), (1, 20, 68, 4)])
def test_anchors_hold_on_the_device(dev, shape):
    from pointcloududa_amd.utils.geometric import GeoProgram
    b, h, w, c = shape
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    lab = rng.integers(0, 5, (b, h, w)).astype(np.int64)
    for mode in range(5):
        prog = GeoProgram.identity(b, 1)
        for i in range(b):
            prog.set_homography(i, 0, np.eye(3), order=3, mode=mode, cval=9)
        got, gl = _run(dev, x, lab, prog)
        assert np.array_equal(got, x) and np.array_equal(gl, lab), "identity, mode %d" % mode
        for m in (C.G.flip_lr(w), C.G.flip_ud(h)):
            p3, p0 = GeoProgram.identity(b, 1), GeoProgram.identity(b, 1)
            for i in range(b):
                p3.set_homography(i, 0, m, order=3, mode=mode, cval=9)
                p0.set_homography(i, 0, m, order=0, mode=mode, cval=9)
            a, z = _run(dev, x, lab, p3), _run(dev, x, lab, p0)
            assert np.array_equal(a[0], z[0]) and np.array_equal(a[1], z[1]) and not np.array_equal(a[0], x)
    for ty, tx in ((1, 2), (-3, 5), (h + 1, -2 * w - 1)):
        prog = GeoProgram.identity(b, 1)
        for i in range(b):
            prog.set_homography(i, 0, [[1.0, 0.0, -tx], [0.0, 1.0, -ty], [0.0, 0.0, 1.0]], order=3, mode=4)
        got, _ = _run(dev, x, lab, prog)
        assert np.array_equal(got, np.roll(x, (ty, tx), axis=(1, 2)))


def test_a_program_without_order_3_gives_the_same_bytes_through_both_entries(dev):
    b, h, w, c = 20, 18, 65, 3
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)
    lab = rng.integers(0, 5, (b, h, w)).astype(np.int64)
    prog = _mixed_program(b, h, w, rng, order=1)
    prog.iarg[::2, 0, 0] = 0
    a, al = _k_run(dev, x, lab, prog, False)
    z, zl = _k_run(dev, x, lab, prog, True)
    assert np.array_equal(a, z) and np.array_equal(al, zl) and not np.array_equal(a, x)
    # and the old entry keeps sampling order 3 as order 1, exactly as before
    p3 = _mixed_program(b, h, w, np.random.default_rng(12), order=3)
    p1 = _mixed_program(b, h, w, np.random.default_rng(12), order=1)
    a, _ = _k_run(dev, x, lab, p3, False)
    z, _ = _k_run(dev, x, lab, p1, False)
    q, _ = _k_run(dev, x, lab, p3, True)
    assert np.array_equal(a, z) and not np.array_equal(a, q)


# ---------------------------------------------------------------------------------------------- the loader
def _raw(b, h, w):
    rng = np.random.default_rng(21)
    PG = _load("make_photometric_golden")
    x = PG.make_images("grey3", b, h, w, 3, 31)
    lab = C.G.ellipse_labels(b, h, w, 5, 32).astype(np.int64)
    return x, lab, rng


def _cubic_plan(b, h, w, seed):
    """a sampled cubic plan with an order-3 elastic slot and a cubic noise upscale"""
    from pointcloududa_amd.utils.augment import GeoProgram, StyleProgram, sample_heavy_plan
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        state = rng.bit_generator.state
        plan = sample_heavy_plan(b, "heavy_refpad_device", rng, h, w, interp="cubic")
        geo = any(isinstance(s, GeoProgram) and s.uses_cubic() for s in plan.stages)
        sty = any(isinstance(s, StyleProgram) and np.any((s.opcode == 2) & (s.iarg[..., 1] == 3)) for s in plan.stages)
        if geo and sty:
            return state, plan
    raise AssertionError("no plan with both cubic paths")


def test_augmented_batches_with_cubic_interp_equal_the_restatements_stage_by_stage(dev):
    from pointcloududa_amd.utils.augment import (AugmentedBatches, AugmentParams, CropPadProgram, GeoProgram, PhotoProgram, StyleProgram,
                                                 augment_batch, crop_pad_aug, geometric_aug, heavy_aug, photometric_aug, stylize_aug)
    PG, SC, CP = _load("make_photometric_golden"), _load("make_stylize_cubic_golden"), _load("make_croppad_golden")
    b, h, w = 4, 64, 48
    x, lab, _ = _raw(b, h, w)
    state, plan = _cubic_plan(b, h, w, 5)
    rng = np.random.default_rng(0)
    rng.bit_generator.state = state
    it = AugmentedBatches(iter([(x, lab[..., None])]), dev, None, rng, num_classes=5, crop_size=0, rescale="div255",
                          heavy_preset="heavy_refpad_device", heavy_interp="cubic", resample_verts=False)
    batches = list(it)
    assert len(batches) == 1 and [type(s) for s in it.last_plan.stages] == [type(s) for s in plan.stages]
    for p, q in zip(plan.stages, it.last_plan.stages):
        assert np.array_equal(p.opcode, q.opcode) and np.array_equal(p.iarg, q.iarg)
    tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    for k, st in enumerate(it.last_plan.stages):
        before, before_lab = tx.cpu().numpy(), tl.cpu().numpy()
        if isinstance(st, PhotoProgram):
            tx = photometric_aug(tx, st)
            want, exc = PG.run_program(before, st.opcode, st.iarg, st.farg, st.seed, backend="numpy")
            assert not ((tx.cpu().numpy() != want) & ~exc).any(), "stage %d (photometric)" % k
        elif isinstance(st, StyleProgram):
            tx = stylize_aug(tx, st)
            want, exc = SC.run_any_program(before, st.opcode, st.iarg, st.farg, st.table, st.seed)
            assert not ((tx.cpu().numpy() != want) & ~exc).any(), "stage %d (stylize)" % k
        elif isinstance(st, CropPadProgram):
            tx, tl = crop_pad_aug(tx, tl, st)
            for i in range(b):
                if st.opcode[i]:
                    t, r, bt, l, mode, cval = (int(v) for v in st.iarg[i])
                    _same(tx[i].cpu().numpy(), CP.crop_pad_restated(before[i], t, r, bt, l, mode, cval)[1], "stage %d sample %d (crop-pad)" % (k, i))
                    _same(tl[i].cpu().numpy(), CP.labels_restated(before_lab[i], t, r, bt, l), "stage %d sample %d labels" % (k, i))
                else:
                    assert np.array_equal(tx[i].cpu().numpy(), before[i]) and np.array_equal(tl[i].cpu().numpy(), before_lab[i])
        else:
            assert isinstance(st, GeoProgram)
            tx, tl = geometric_aug(tx, tl, st)
            cur, cur_lab = before, before_lab
            for s in range(st.slots):      # one slot at a time from the device's own intermediate values
                one = tuple(np.ascontiguousarray(a[:, s:s + 1]) for a in (st.opcode, st.iarg, st.farg, st.seed))
                want, want_lab, _, _ = C.run_program(cur, cur_lab, *one, backend="numpy")
                # (orders 0 and 1 are f8's ground: its excused set, a coordinate or a value within 1e-9 of a tie)
                as_f8 = one[1].copy()
                as_f8[..., 0] = np.minimum(as_f8[..., 0], 1)
                _, _, exc, exc_lab, _ = C.G.run_program(cur, cur_lab, one[0], as_f8, one[2], one[3], backend="numpy")
                cubic = (one[0][:, 0] != 0) & (one[1][:, 0, 0] == 3)
                cur, cur_lab = _run(dev, cur, cur_lab, _program(one))
                _same(cur[cubic], want[cubic], "stage %d slot %d (order 3)" % (k, s))
                _same(cur_lab[cubic], want_lab[cubic], "stage %d slot %d (order 3) labels" % (k, s))
                assert not ((cur != want) & ~exc)[~cubic].any() and not ((cur_lab != want_lab) & ~exc_lab)[~cubic].any(), (k, s)
            assert np.array_equal(cur, tx.cpu().numpy()) and np.array_equal(cur_lab, tl.cpu().numpy())
    hx, hl = heavy_aug(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), it.last_plan)
    assert torch.equal(hx, tx) and torch.equal(hl, tl) and not torch.equal(hx.cpu(), torch.from_numpy(x))
    ref = augment_batch(hx, hl, AugmentParams.identity(b), 5, 0, "div255", resample_verts=False)
    assert torch.equal(batches[0][0], ref[0]) and torch.equal(batches[0][1], ref[1])


def test_the_cubic_path_adds_no_host_synchronisation(dev):
    """geometric_aug on a cubic program, heavy_aug and augment_batch(.., heavy=..) on a cubic plan under
    torch.cuda.set_sync_debug_mode("error"); the mode is first shown to be enforced (a ``.item()`` raises under it)"""
    from pointcloududa_amd.utils.augment import augment_batch, geometric_aug, heavy_aug, sample_geo_program
    b, h, w = 4, 64, 48
    x, lab, _ = _raw(b, h, w)
    tq, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    _, plan = _cubic_plan(b, h, w, 5)
    rng = np.random.default_rng(9)
    prog = sample_geo_program(b, "heavy_device", rng, h, w, interp="cubic")
    while not prog.uses_cubic():
        prog = sample_geo_program(b, "heavy_device", rng, h, w, interp="cubic")
    ref_g = geometric_aug(tq, tl, prog)                                                # (warm: allocator, library load)
    ref_h = heavy_aug(tq, tl, plan)
    ref = augment_batch(tq, tl, None, 5, 0, rescale="div255", heavy=plan, resample_verts=False)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        a = geometric_aug(tq, tl, prog)
        z = heavy_aug(tq, tl, plan)
        c = augment_batch(tq, tl, None, 5, 0, rescale="div255", heavy=plan, resample_verts=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a[0], ref_g[0]) and torch.equal(a[1], ref_g[1])
    assert torch.equal(z[0], ref_h[0]) and torch.equal(z[1], ref_h[1])
    assert torch.equal(c[0], ref[0]) and torch.equal(c[1], ref[1])


def test_entry_point_returns_status_codes(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd.utils.geometric import GeoProgram, upload_geo_program
    lib = _lib.lib()
    b, h, w, c = 2, 18, 20, 3
    x = torch.zeros((b, h, w, c), dtype=torch.uint8, device=dev)
    out = torch.full_like(x, 7)
    op, ia, fa, sd = upload_geo_program(GeoProgram.identity(b, 2), b, h, w, dev)
    need = lib.pcuda_geometric_workspace_size(b, h, w, c, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(outp=out.data_ptr(), slots=2, nbytes=need, hh=h):
        return lib.pcuda_geometric_cubic(x.data_ptr(), outp, None, None, b, hh, w, c, slots, op.data_ptr(), ia.data_ptr(), fa.data_ptr(),
                                         sd.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert call(outp=x.data_ptr()) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(slots=9) == -1 and call(hh=1) == -1
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "a rejected call launches nothing"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
