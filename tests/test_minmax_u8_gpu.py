"""The fp32 -> uint8 -> fp32 joint of the MM-WHS heavy path (``data_generator_mmwhs.py:245-263``) on
the GPU: ``kernels.quantize_u8`` against numpy's ``quantise`` (scripts/make_augment_golden.py), the dequantising assemble
against ``dequantise``, ``augment_batch(.., rescale="minmax_u8")`` against the fused ``"minmax"`` launch and against the uint8
path on the numpy-quantised upload, ``AugmentedBatches`` against the manual composition.  Everything bit for bit, no excused
pixels: both sides run the same device warp, only the joint differs."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_augment_golden", os.path.join(ROOT, "scripts", "make_augment_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
CASES = [c for c in G.load_cases(np.load(os.path.join(GOLD, "augment.npz"))) if "minmax_f32" in c]

QUANT_BLOCK = 256 * 16       # elements per workgroup of quantize_u8_kernel's wide path (csrc/augment.hip)
B, H, W, C, K5 = 4, 64, 48, 3, 5
PLAN_SEED = 3                # heavy_full_device: photometric, stylize, photometric, geometric stages; refpad adds CropAndPad


def _quantize(dev, x, offset_in=0, offset_out=0):
    """kernels.quantize_u8 on a flat copy of x that starts ``offset_in`` floats into its buffer, written ``offset_out`` bytes
    into the result's buffer -> (q as numpy in x's shape, the (min, max) the device found)"""
    from pointcloududa_amd import kernels as K
    n = x.size
    buf = torch.zeros(n + offset_in, dtype=torch.float32, device=dev)
    buf[offset_in:] = torch.from_numpy(x.reshape(-1)).to(dev)
    src = buf[offset_in:]
    mm = K.minmax(src)
    obuf = torch.full((n + offset_out + 16,), 77, dtype=torch.uint8, device=dev)
    out = obuf[offset_out:offset_out + n]
    assert src.data_ptr() % 16 == (4 * offset_in) % 16 and out.data_ptr() % 16 == offset_out % 16
    got = K.quantize_u8(src, mm, out=out)
    assert got.data_ptr() == out.data_ptr()
    o = obuf.cpu().numpy()
    assert np.all(o[:offset_out] == 77) and np.all(o[offset_out + n:] == 77), "the kernel wrote outside its result"
    return o[offset_out:offset_out + n].reshape(x.shape), mm.cpu().numpy()


def _check_quantiser(dev, x, **kw):
    exp, mn, mx = G.quantise(x)
    got, mm = _quantize(dev, x, **kw)
    assert mm[0] == mn and mm[1] == mx
    assert got.dtype == np.uint8 and np.array_equal(got, exp), int((got != exp).sum())
    return got


# ---------------------------------------------------------------------------------------------- 1. the quantiser
def test_quantiser_tail_only(dev):
    x = np.random.default_rng(1).normal(0, 1, (1, 5, 7, 3)).astype(np.float32)
    assert x.size == 105 and x.size % 16 != 0
    _check_quantiser(dev, x)


def test_quantiser_several_workgroups(dev):
    x = np.random.default_rng(2).normal(0, 1, (2, 64, 72, 3)).astype(np.float32)
    assert x.size >= 3 * QUANT_BLOCK and x.size % QUANT_BLOCK != 0
    q = _check_quantiser(dev, x)
    assert q.min() == 0 and q.max() == 255


@pytest.mark.parametrize("lo,hi", [(-1.7, 2.9), (-3.0, 3.0), (-0.37, 4.11)])
def test_quantiser_on_the_grid_levels(dev, lo, hi):
    """the 256 values min + k (max - min) / 255 sit on truncation boundaries: a quantiser that multiplies by 1 / range gets
    38, 8 and 4 of them wrong (numpy, on the CPU; asserted here so that the case keeps its teeth)"""
    mn, mx = np.float32(lo), np.float32(hi)
    x = (mn + np.arange(256, dtype=np.float32) * (mx - mn) / np.float32(255.)).astype(np.float32)
    x[0], x[-1] = mn, mx
    x = x.reshape(1, 16, 16, 1)
    exp, emn, emx = G.quantise(x)
    assert emn == mn and emx == mx
    short = np.array((x - mn) * np.float32(255.) * (np.float32(1.) / (mx - mn)), dtype=np.uint8)
    assert int((short != exp).sum()) == {-1.7: 38, -3.0: 8, -0.37: 4}[lo]
    _check_quantiser(dev, x)
    _check_quantiser(dev, x, offset_in=1, offset_out=1)


@pytest.mark.parametrize("offset_in,offset_out", [(1, 0), (0, 1), (1, 1), (3, 5)])
def test_quantiser_misaligned_views(dev, offset_in, offset_out):
    x = np.random.default_rng(4).normal(0, 1, (2, 37, 41, 3)).astype(np.float32)
    assert x.size > QUANT_BLOCK
    aligned = _check_quantiser(dev, x)
    assert np.array_equal(_check_quantiser(dev, x, offset_in=offset_in, offset_out=offset_out), aligned)


def test_quantiser_constant_batch(dev):
    """max == min: q = 0 everywhere (the reference computes 0 / 0), and the dequantised images all equal min"""
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.augment import AugmentParams, augment_batch, quantize_minmax, upload_params
    x = torch.full((2, 16, 20, 2), 3.25, dtype=torch.float32, device=dev)
    q, mm = quantize_minmax(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and not q.any() and mm.tolist() == [3.25, 3.25]
    inv, order, cval = upload_params(AugmentParams.identity(2), 2, 16, 20, dev)
    out = K.augment_assemble_dequant(q, None, inv, order, cval, mm)["images"]
    assert out.shape == (2, 2, 16, 20) and bool((out == 3.25).all())
    lab = torch.zeros((2, 16, 20), dtype=torch.int64, device=dev)
    gi, _, _ = augment_batch(x, lab, None, 2, 0, rescale="minmax_u8")
    assert bool((gi == 3.25).all())


def test_quantiser_nan_element(dev):
    from pointcloududa_amd import kernels as K
    x = np.random.default_rng(6).normal(0, 1, (1, 33, 35, 3)).astype(np.float32)
    exp, mn, mx = G.quantise(x)
    for at in (7, x.size - 2):          # one in the wide path, one in the tail
        y = x.reshape(-1).copy()
        assert y[at] != mn and y[at] != mx
        y[at] = np.nan
        t = torch.from_numpy(y).to(dev)
        mm = K.minmax(t)
        assert mm.tolist() == [float(mn), float(mx)]
        got = K.quantize_u8(t, mm).cpu().numpy()
        want = exp.reshape(-1).copy()
        want[at] = 0
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- 2. the fused path
def _case_params(case):
    from pointcloududa_amd.utils.augment import AugmentParams
    return AugmentParams(op_order=case["op_order"], **{k: np.array(v) for k, v in case["params"].items()})


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_minmax_u8_equals_the_fused_minmax_launch(dev, name):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.augment import augment_batch, quantize_minmax, upload_params
    case = [c for c in CASES if c["name"] == name][0]
    x, q, mn, mx, lab = G.case_inputs(case)
    params = _case_params(case)
    tx, tl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    tq, mm = quantize_minmax(tx)
    assert np.array_equal(tq.cpu().numpy(), q) and mm.tolist() == [float(mn), float(mx)]
    inv, order, cval = upload_params(params, case["b"], case["h"], case["w"], dev)
    for crop, verts in ((0, False), (40, False), (40, True)):
        ri, ro, rv = augment_batch(tx, tl, params, case["k"], crop, rescale="minmax", resample_verts=verts)
        gi, go, gv = augment_batch(tx, tl, params, case["k"], crop, rescale="minmax_u8", resample_verts=verts)
        assert gi.dtype == torch.float32 and torch.equal(gi, ri) and torch.equal(go, ro)
        assert (gv is None and rv is None) if not verts else torch.equal(gv, rv)
        # and the two-launch form of the same thing: quantise, then the dequantising assemble
        out = K.augment_assemble_dequant(tq, tl.to(torch.int32), inv, order, cval, mm, case["k"], crop, want_full_mask=verts)
        assert torch.equal(out["images"], ri) and torch.equal(out["onehot"], ro)
    with pytest.raises(TypeError, match="fp32"):
        augment_batch(tq, tl, params, case["k"], 0, rescale="minmax_u8")


# ---------------------------------------------------------------------------------------------- 3. / 4. uint8 stages
def _inputs(dev, seed=11):
    x = G.smooth_images(B, H, W, C, seed)
    lab = G.ellipse_labels(B, H, W, K5, seed + 1)
    q, mn, mx = G.quantise(x)
    return x, lab, q, mn, mx, torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(q).to(dev)


def _live(plan):
    live = np.zeros(plan.batch, dtype=bool)
    for st in plan.stages:
        live |= (st.opcode.reshape(plan.batch, -1) != 0).any(1)
    return live


def _check_against_the_u8_path(dev, params, **stages):
    """rescale="minmax_u8" on fp32 against rescale=None on the numpy-quantised upload with the same stages: one-hot and
    vertices equal, images = dequantise(q') of that path's uint8 result; and the stages act"""
    from pointcloududa_amd.utils.augment import augment_batch
    x, lab, q, mn, mx, tx, tl, tq = _inputs(dev)
    gi, go, gv = augment_batch(tx, tl, params, K5, 0, rescale="minmax_u8", resample_verts=True, **stages)
    ri, ro, rv = augment_batch(tq, tl, params, K5, 0, rescale=None, resample_verts=True, **stages)
    assert gi.dtype == torch.float32 and gi.shape == (B, C, H, W) and go.shape == (B, K5, H, W) and gv.shape == (B, 300, 3)
    assert torch.equal(go, ro) and torch.equal(gv, rv)
    qp = ri.cpu().numpy()
    assert np.array_equal(qp, np.floor(qp)) and qp.min() >= 0 and qp.max() <= 255
    assert np.array_equal(gi.cpu().numpy(), G.dequantise(qp.astype(np.uint8), mn, mx))
    pi, _, _ = augment_batch(tx, tl, params, K5, 0, rescale="minmax_u8", resample_verts=True)
    differs = (gi != pi).flatten(1).any(1).cpu().numpy()
    return differs


@pytest.mark.parametrize("preset", ["heavy_full_device", "heavy_refpad_device"])
def test_heavy_plan_between_quantiser_and_assemble(dev, preset):
    from pointcloududa_amd.utils.augment import AugmentParams, sample_heavy_plan
    plan = sample_heavy_plan(B, preset, np.random.default_rng(PLAN_SEED), H, W)
    assert _live(plan).all() and len({type(s) for s in plan.stages}) >= 3
    differs = _check_against_the_u8_path(dev, AugmentParams.identity(B), heavy=plan)
    assert differs.any()


def test_photometric_program_between_quantiser_and_assemble(dev):
    from pointcloududa_amd.utils.augment import sample_params, sample_program
    rng = np.random.default_rng(9)
    prog = sample_program(B, "mscmrseg_aug2_photometric", rng)
    assert ((prog.opcode != 0).sum(1) > 0).all()
    params = sample_params(B, "mmwhs_light", rng)
    params.affine_on[:] = True
    params.flip_lr[:] = [True, False, False, True]
    params.order[:] = [0, 1, 1, 0]
    differs = _check_against_the_u8_path(dev, params, photometric=prog)
    assert differs.any()


# ---------------------------------------------------------------------------------------------- 5. the loader wrapper
def test_augmented_batches_minmax_u8_heavy_end_to_end(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.augment import (AugmentParams, AugmentedBatches, as_labels, heavy_aug, quantize_minmax,
                                                 sample_heavy_plan, upload_params)
    from pointcloududa_amd.utils.npy2point import masks_to_pointclouds
    raw = [(G.smooth_images(B, H, W, C, 60 + i), G.ellipse_labels(B, H, W, K5, 70 + i)[..., None]) for i in range(2)]
    it = AugmentedBatches(iter(raw), dev, None, np.random.default_rng(123), num_classes=K5, crop_size=40, rescale="minmax_u8",
                          heavy_preset="heavy_refpad_device")
    twin = np.random.default_rng(123)
    inv, order, cval = upload_params(AugmentParams.identity(B), B, H, W, dev)
    n = 0
    for (gx, gy, gz), (img, lab) in zip(it, raw):
        plan = sample_heavy_plan(B, "heavy_refpad_device", twin, H, W)
        assert it.last_plan is not None and len(it.last_plan.stages) == len(plan.stages)
        for a, b in zip(it.last_plan.stages, plan.stages):
            assert type(a) is type(b) and np.array_equal(a.opcode, b.opcode)
        q, mm = quantize_minmax(torch.from_numpy(img).to(dev))
        q, m = heavy_aug(q, torch.from_numpy(lab).to(dev), plan)
        out = K.augment_assemble_dequant(q, as_labels(m), inv, order, cval, mm, K5, 40, want_full_mask=True)
        z = masks_to_pointclouds(out["full_mask"], torch.zeros(B, dtype=torch.int32, device=dev)).cpu().numpy()
        z = z.astype(np.float32) / np.float32(255.0)          # (a true division, as the generator's; not torch's scalar reciprocal)
        assert gx.shape == (B, C, 40, 40) and gx.dtype == torch.float32 and gy.dtype == torch.uint8
        assert torch.equal(gx, out["images"]) and torch.equal(gy, out["onehot"]) and np.array_equal(gz.cpu().numpy(), z)
        n += 1
    assert n == 2
    # a photometric preset and a plain preset take the value too, draw for draw as "div255" does
    for kw in (dict(photometric_preset="mscmrseg_aug2_photometric"), {}):
        a = AugmentedBatches(iter(raw), dev, "mmwhs_light", np.random.default_rng(5), num_classes=K5, rescale="minmax_u8", **kw)
        u8 = [(G.quantise(img)[0], lab) for img, lab in raw]
        b = AugmentedBatches(iter(u8), dev, "mmwhs_light", np.random.default_rng(5), num_classes=K5, rescale="div255", **kw)
        for (ax, ay, az), (bx, by, bz) in zip(a, b):
            assert torch.equal(ay, by) and torch.equal(az, bz) and ax.shape == bx.shape
        assert a.rng.bit_generator.state == b.rng.bit_generator.state


# ---------------------------------------------------------------------------------------------- 6. match_hist in front
def test_match_hist_runs_on_fp32_in_front_of_the_quantiser(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.augment import (AugmentParams, HistReference, augment_batch, match_histograms,
                                                 sample_heavy_plan)
    x, lab, q, mn, mx, tx, tl, tq = _inputs(dev)
    ref = HistReference(G.smooth_images(1, H, W, C, 99)[0] * np.float32(1.7) - np.float32(0.4), dev)
    plan = sample_heavy_plan(B, "heavy_refpad_device", np.random.default_rng(PLAN_SEED), H, W)
    ident = AugmentParams.identity(B)
    matched = match_histograms(tx, ref)
    mmn, mmx = K.minmax(matched).tolist()
    assert (mmn, mmx) != (float(mn), float(mx))
    gi, go, gv = augment_batch(tx, tl, ident, K5, 0, rescale="minmax_u8", resample_verts=True, heavy=plan, match_hist=ref)
    ri, ro, rv = augment_batch(matched, tl, ident, K5, 0, rescale="minmax_u8", resample_verts=True, heavy=plan)
    assert torch.equal(gi, ri) and torch.equal(go, ro) and torch.equal(gv, rv)
    # min and max are those of the matched images: the uint8 path on the numpy-quantised matched batch, dequantised with them
    mq, qmn, qmx = G.quantise(matched.cpu().numpy())
    assert (float(qmn), float(qmx)) == (mmn, mmx)
    ui, _, _ = augment_batch(torch.from_numpy(mq).to(dev), tl, ident, K5, 0, rescale=None, heavy=plan)
    assert np.array_equal(gi.cpu().numpy(), G.dequantise(ui.cpu().numpy().astype(np.uint8), qmn, qmx))
