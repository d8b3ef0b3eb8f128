"""Device-side CropAndPad with numpy's pad modes on the GPU, through the public surface
(utils/augment.py, utils/croppad.py) and the C ABI, against the committed fixture tests/golden/croppad.npz: the padded arrays
are numpy.pad's own output (scripts/make_croppad_golden.py), the resized outputs a restatement pinned by a second one.
Everything is integer-valued or a float64 sequence that the restatement performs in the same order: every comparison is bit
for bit.  The fixture is read alone (no numpy.pad here)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD

pytestmark = pytest.mark.gpu

F = np.load(os.path.join(GOLD, "croppad.npz"))
SHAPES = ((9, 7), (12, 10), (33, 18), (64, 48))


def _program(args, copies=()):
    """CropPadProgram from rows of (top, right, bottom, left, mode, cval); rows named in `copies` stay copies"""
    from pointcloududa_amd.utils.augment import CropPadProgram
    p = CropPadProgram.identity(len(args))
    for i, a in enumerate(args):
        if i not in copies:
            p.set_crop_and_pad(i, *(int(v) for v in a))
    return p


def _run(dev, images, program, masks=None):
    from pointcloududa_amd.utils.augment import crop_pad_aug
    x = torch.from_numpy(np.ascontiguousarray(images)).to(dev)
    m = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks)).to(dev)
    keep = x.clone()
    out, mo = crop_pad_aug(x, m, program)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x, keep), "the input is never written"
    if masks is None:
        assert mo is None
        return out.cpu().numpy()
    assert mo.dtype == m.dtype and mo.shape == m.shape
    return out.cpu().numpy(), mo.cpu().numpy()


def _same(got, want, what):
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_mode_equals_the_fixture(dev, shape, c):
    """one batch of ten samples per shape, sample k in mode k with its own sides and cval; then every sample alone"""
    h, w = shape
    img = F["img_%dx%dx%d" % (h, w, c)]
    keys = ["%dx%dx%d_m%d" % (h, w, c, m) for m in range(10)]
    args = [F["arg_" + k] for k in keys]
    assert [int(a[4]) for a in args] == list(range(10))
    got = _run(dev, np.repeat(img[None], 10, axis=0), _program(args))
    for m, k in enumerate(keys):
        _same(got[m], F["out_" + k], (k, args[m].tolist()))
    for m, k in enumerate(keys):
        _same(_run(dev, img[None], _program(args[m:m + 1]))[0], F["out_" + k], ("alone", k))


def test_net_zero_geometries_return_numpy_pads_array(dev):
    keys = ["zero%s_m%d" % (t, m) for t in "ab" for m in range(10)]
    args = [F["arg_" + k] for k in keys]
    assert all(a[0] + a[2] == 0 and a[1] + a[3] == 0 for a in args) and tuple(args[0][:4]) == (10, -10, -10, 10)
    got = _run(dev, np.repeat(F["img_22x22x3"][None], len(keys), axis=0), _program(args))
    for i, k in enumerate(keys):
        assert F["pad_" + k].shape == (22, 22, 3)
        _same(got[i], F["pad_" + k], k)


def test_both_forms_of_the_ramp(dev):
    """width 10, end 0, edge 90: 63 at k = 7 -- and 62 once another edge value of the same side equals the end value"""
    for tag, at7 in (("a", 63), ("b", 62)):
        got = _run(dev, F["img_ramp_" + tag][None], _program([F["arg_ramp_" + tag]]))[0]
        _same(got, F["pad_ramp_" + tag], "ramp_" + tag)
        assert got[0, 7, 0] == at7 and got[0, 10, 0] == 90
    both = _run(dev, np.stack([F["img_ramp_a"], F["img_ramp_b"]]), _program([F["arg_ramp_a"], F["arg_ramp_b"]]))
    _same(both[0], F["pad_ramp_a"], "ramp_a in a batch")
    _same(both[1], F["pad_ramp_b"], "ramp_b in a batch")


@pytest.mark.parametrize("mode", (4, 5))
def test_statistics_of_k_and_a_half_round_to_even(dev, mode):
    """columns whose mean and median are k + 0.5 for even and odd k; a median over an even (6) and an odd (5) count"""
    for tag in ("even", "odd"):
        k = "half_%s_m%d" % (tag, mode)
        got = _run(dev, F["img_half"][None], _program([F["arg_" + k]]))[0]
        _same(got, F["out_" + k], k)
    assert F["pad_half_even_m%d" % mode][0, 2:10, 0].tolist() == [0, 2, 2, 4, 4, 6, 6, 8]


def test_a_batch_mixes_all_ten_modes_with_copies(dev):
    h, w, c = 33, 18, 3
    img = F["img_%dx%dx%d" % (h, w, c)]
    order = [7, 0, 5, -1, 2, 9, 4, 3, -1, 6, 1, 8, 5]
    x = np.stack([np.roll(img, i, axis=1) if m < 0 else img for i, m in enumerate(order)])
    args = [np.array([9, 9, 9, 9, 3, 77], dtype=np.int32) if m < 0 else F["arg_%dx%dx%d_m%d" % (h, w, c, m)] for m in order]
    lab = np.random.default_rng(3).integers(0, 5, (len(order), h, w)).astype(np.int64)
    got, glab = _run(dev, x, _program(args, copies=[i for i, m in enumerate(order) if m < 0]), lab)
    for i, m in enumerate(order):
        if m < 0:
            _same(got[i], x[i], "copy %d" % i)
            _same(glab[i], lab[i], "copied mask %d" % i)
        else:
            _same(got[i], F["out_%dx%dx%d_m%d" % (h, w, c, m)], "sample %d mode %d" % (i, m))


@pytest.mark.parametrize("shape", ((12, 10), (33, 18)), ids=lambda s: "%dx%d" % s)
def test_masks_are_nearest_with_constant_zero_under_every_image_mode(dev, shape):
    h, w = shape
    lab = F["lab_%dx%d" % (h, w)]
    img = F["img_%dx%dx1" % (h, w)]
    k = 0
    while "labarg_%dx%d_s%d" % (h, w, k) in F.files:
        sides = F["labarg_%dx%d_s%d" % (h, w, k)]
        want = F["labout_%dx%d_s%d" % (h, w, k)]
        args = [np.concatenate([sides, [m, 200]]).astype(np.int32) for m in range(10)]
        for masks in (np.repeat(lab[None], 10, axis=0), np.repeat(lab[None], 10, axis=0).astype(np.int64)[..., None]):
            _, got = _run(dev, np.repeat(img[None], 10, axis=0), _program(args), masks)
            for m in range(10):
                _same(got[m].reshape(h, w), want, ("mask", shape, sides.tolist(), m))
        k += 1
    assert k >= 4


def test_out_and_aliasing(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.augment import crop_pad_aug
    from pointcloududa_amd.utils.croppad import upload_crop_pad_program
    key = "12x10x3_m5"
    x = torch.from_numpy(F["img_12x10x3"][None].copy()).to(dev)
    prog = _program([F["arg_" + key]])
    out = torch.full_like(x, 9)
    res, none = crop_pad_aug(x, None, prog, out=out)
    assert none is None and res.data_ptr() == out.data_ptr()
    _same(out.cpu().numpy()[0], F["out_" + key], "out=")
    keep = x.clone()
    with pytest.raises(RuntimeError, match="in == out"):
        crop_pad_aug(x, None, prog, out=x)
    lab = torch.zeros((1, 12, 10), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="in == out"):
        K.crop_pad(x, lab, *upload_crop_pad_program(prog, 1, 12, 10, dev), labels_out=lab)
    with pytest.raises(ValueError, match="out must be"):
        crop_pad_aug(x, None, prog, out=torch.empty((1, 12, 10, 4), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(x, keep), "a refused call launches nothing"


def test_entry_point_returns_status_codes(dev):
    from pointcloududa_amd import _lib
    from pointcloududa_amd.utils.croppad import upload_crop_pad_program
    lib = _lib.lib()
    key = "33x18x3_m4"
    b, h, w, c = 2, 33, 18, 3
    x = torch.from_numpy(np.repeat(F["img_33x18x3"][None], b, axis=0)).to(dev)
    out = torch.full_like(x, 7)
    op, ia = upload_crop_pad_program(_program([F["arg_" + key]] * b), b, h, w, dev)
    need = lib.pcuda_crop_pad_workspace_size(b, h, w, c)
    assert need % 16 == 0 and need >= b * c * (w + h + 128) + 4 * b
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(outp=out.data_ptr(), nbytes=need, wsp=ws.data_ptr(), **kw):
        d = dict(b=b, h=h, w=w, c=c)
        d.update(kw)
        return lib.pcuda_crop_pad(x.data_ptr(), outp, None, None, d["b"], d["h"], d["w"], d["c"], op.data_ptr(), ia.data_ptr(), wsp,
                                  nbytes, stream)
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()      # one byte short
    assert call(wsp=None) == -4 and call(outp=x.data_ptr()) == -1 and call(c=5) == -1 and call(h=1) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "a rejected call launches nothing"
    assert call() == 0
    torch.cuda.synchronize()
    for i in range(b):
        _same(out[i].cpu().numpy(), F["out_" + key], "C ABI")


def _raw_batches(n, b):
    from oracle.synth import synth_batch
    raw = []
    for i in range(n):
        lab = np.argmax(synth_batch(b, 1, 5, 256, seed=40 + i)[1], axis=1).astype(np.int64)[..., None]
        img = np.random.default_rng(50 + i).integers(0, 256, (b, 256, 256, 3), dtype=np.uint8)
        raw.append((img, lab))
    return raw


def _plan_with_crop(preset, b, h, w, seed):
    from pointcloududa_amd.utils.augment import CropPadProgram, sample_heavy_plan
    rng = np.random.default_rng(seed)
    while True:
        plan = sample_heavy_plan(b, preset, rng, h, w)
        crop = [s for s in plan.stages if isinstance(s, CropPadProgram)]
        if crop and len(set(crop[0].iarg[crop[0].opcode == 1][:, 4])) >= 3:
            return plan


def _one_by_one(images, masks, plan):
    from pointcloududa_amd.utils.augment import (CropPadProgram, GeoProgram, PhotoProgram, StyleProgram, crop_pad_aug, geometric_aug,
                                                 photometric_aug, stylize_aug)
    for st in plan.stages:
        if isinstance(st, PhotoProgram):
            images = photometric_aug(images, st)
        elif isinstance(st, StyleProgram):
            images = stylize_aug(images, st)
        elif isinstance(st, GeoProgram):
            images, masks = geometric_aug(images, masks, st)
        else:
            assert isinstance(st, CropPadProgram)
            images, masks = crop_pad_aug(images, masks, st)
    return images, masks


@pytest.mark.parametrize("preset", ("heavy_refpad_device", "mscmrseg_aug2_refpad_device"))
def test_heavy_aug_runs_the_new_presets_stage_by_stage(dev, preset):
    b, h, w = 8, 64, 48
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (b, h, w, 3), dtype=np.uint8)).to(dev)
    m = torch.from_numpy(np.random.default_rng(2).integers(0, 5, (b, h, w)).astype(np.int64)).to(dev)
    from pointcloududa_amd.utils.augment import heavy_aug
    plan = _plan_with_crop(preset, b, h, w, 21)
    gx, gm = heavy_aug(x, m, plan)
    wx, wm = _one_by_one(x, m, plan)
    assert torch.equal(gx, wx) and torch.equal(gm, wm) and gm.dtype == m.dtype and gm.shape == m.shape
    assert not torch.equal(gx, x)


@pytest.mark.parametrize("preset", ("heavy_refpad_device", "mscmrseg_aug2_refpad_device"))
def test_augmented_batches_take_the_new_presets(dev, preset):
    from pointcloududa_amd.utils.augment import (AugmentedBatches, AugmentParams, CropPadProgram, augment_batch, sample_heavy_plan)
    raw = _raw_batches(2, 4)
    it = AugmentedBatches(iter(raw), dev, None, np.random.default_rng(78), num_classes=5, crop_size=224, rescale="div255",
                          heavy_preset=preset, resample_verts=False)
    twin = np.random.default_rng(78)
    seen = 0
    for k, (x, y, z) in enumerate(it):
        assert x.dtype == torch.float32 and x.shape == (4, 3, 224, 224) and y.shape == (4, 5, 224, 224)
        want = sample_heavy_plan(4, preset, twin, 256, 256)
        assert [type(s) for s in want.stages] == [type(s) for s in it.last_plan.stages]
        for a, b2 in zip(want.stages, it.last_plan.stages):
            assert np.array_equal(a.opcode, b2.opcode) and np.array_equal(a.iarg, b2.iarg)
        seen += sum(isinstance(s, CropPadProgram) for s in want.stages)
        tx, tm = torch.from_numpy(raw[k][0]).to(dev), torch.from_numpy(raw[k][1]).to(dev)
        hx, hm = _one_by_one(tx, tm, want)
        ref = augment_batch(hx, hm, AugmentParams.identity(4), 5, 224, "div255", resample_verts=False)
        assert torch.equal(x, ref[0]) and torch.equal(y, ref[1])
    assert seen > 0, preset


def test_the_crop_pad_path_adds_no_host_synchronisation(dev):
    """crop_pad_aug and heavy_aug under torch.cuda.set_sync_debug_mode("error"); the mode is first shown to be enforced"""
    from pointcloududa_amd.utils.augment import crop_pad_aug, heavy_aug
    b, h, w = 10, 33, 18
    args = [F["arg_33x18x3_m%d" % m] for m in range(10)]
    x = torch.from_numpy(np.repeat(F["img_33x18x3"][None], b, axis=0)).to(dev)
    lab = torch.from_numpy(np.random.default_rng(5).integers(0, 5, (b, h, w)).astype(np.int32)).to(dev)
    prog = _program(args)
    plan = _plan_with_crop("heavy_refpad_device", b, h, w, 4)
    ref = crop_pad_aug(x, lab, prog)                                   # (warm: allocator, library load)
    ref_h = heavy_aug(x, lab, plan)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        got = crop_pad_aug(x, lab, prog)
        got_h = heavy_aug(x, lab, plan)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(got_h[0], ref_h[0]) and torch.equal(got_h[1], ref_h[1])
    for m in range(10):
        _same(got[0][m].cpu().numpy(), F["out_33x18x3_m%d" % m], m)
