"""Device-side light augmentation (flips + affine + rescale + batch assembly) on the GPU against
the committed fixture tests/golden/augment.npz (scripts/make_augment_golden.py: scipy.ndimage.affine_transform on float64,
pinned by a plain-numpy restatement).  Inputs are rebuilt from the cases' seeds; scipy is not needed here.

Rule for the warped cases: the uint8 warp equals the helper's except at EXCUSED pixels -- order 1: the helper's
pre-rounding value lies within 1e-9 of a rounding boundary, the pixel may differ by one grey level; order 0 (and every
mask): a source coordinate lies within 1e-9 of a half-integer, the pixel must equal one of the four neighbouring source
texels or the fill value.  Excused pixels are at most 1e-5 of all pixels of the case set (asserted on the fixture)."""
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
CASES = G.load_cases(np.load(os.path.join(GOLD, "augment.npz")))
NAMES = [c["name"] for c in CASES]


def _case(name):
    return [c for c in CASES if c["name"] == name][0]


def _params(case, **override):
    from pointcloududa_amd.utils.augment import AugmentParams
    d = {k: np.array(v) for k, v in case["params"].items()}
    d.update(override)
    return AugmentParams(op_order=case["op_order"], **d)


def _excused_masks(case):
    b, h, w, c = case["u8"].shape
    ei, em = np.zeros((b, h, w, c), dtype=bool), np.zeros((b, h, w), dtype=bool)
    ei[tuple(case["exc_img"].T)] = True
    em[tuple(case["exc_mask"].T)] = True
    return ei, em


def _neighbour_values(src2d, inv, y, x, fill):
    """the four source texels around the source coordinate of output pixel (x, y), fill where outside"""
    h, w = src2d.shape
    sx = inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]
    sy = inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]
    vals = {int(fill)}
    for yy in (int(np.floor(sy)), int(np.floor(sy)) + 1):
        for xx in (int(np.floor(sx)), int(np.floor(sx)) + 1):
            if 0 <= yy < h and 0 <= xx < w:
                vals.add(int(src2d[yy, xx]))
    return vals


def _check_images(case, got_u8, q):
    """got_u8 [B,H,W,C] against the helper's warp under the excused-pixel rule"""
    exp = case["u8"]
    assert got_u8.shape == exp.shape and got_u8.dtype == np.uint8
    ei, _ = _excused_masks(case)
    order, cval = G.effective(case["params"])
    assert np.array_equal(got_u8[~ei], exp[~ei]), (case["name"], int((got_u8 != exp)[~ei].sum()))
    for b, y, x, ch in case["exc_img"]:
        if order[b] == 1:
            assert abs(int(got_u8[b, y, x, ch]) - int(exp[b, y, x, ch])) <= 1
        else:
            assert int(got_u8[b, y, x, ch]) in _neighbour_values(q[b, :, :, ch], case["inv"][b], y, x, cval[b])
    return got_u8 == exp


def _check_masks(case, got, lab):
    exp = case["mask"]
    assert got.shape == exp.shape
    _, em = _excused_masks(case)
    assert np.array_equal(got[~em], exp[~em]), (case["name"], int((got != exp)[~em].sum()))
    for b, y, x in case["exc_mask"]:
        assert int(got[b, y, x]) in _neighbour_values(lab[b], case["inv"][b], y, x, 0)
    return got == exp


def _to_u8_hwc(images_chw):
    a = images_chw.permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(a, np.floor(a)) and a.min() >= 0 and a.max() <= 255
    return np.ascontiguousarray(a.astype(np.uint8))


# ---------------------------------------------------------------------------------------------- identity, flips
@pytest.mark.parametrize("crop", [0, 224, 100])
def test_identity_parameters_reproduce_assemble_batch(dev, crop):
    from oracle import batch as OB
    from pointcloududa_amd.utils.augment import AugmentParams, augment_batch
    from pointcloududa_amd.utils.batch import assemble_batch
    rng = np.random.default_rng(9)
    img = rng.normal(0, 1, (3, 256, 256, 3)).astype(np.float32)
    m = rng.integers(0, 5, (3, 256, 256, 1)).astype(np.int64)
    v = rng.integers(0, 256, (3, 300, 3)).astype(np.int64)
    ti, tm, tv = torch.from_numpy(img).to(dev), torch.from_numpy(m).to(dev), torch.from_numpy(v).to(dev)
    ri, ro, rv = assemble_batch(ti, tm, 5, crop, verts=tv)
    oi, oo, ov = OB.assemble_batch(img, m, v, num_classes=5, crop_size=crop)
    ident = AugmentParams.identity(3)
    ident.order[:] = 1; ident.cval[:] = 200; ident.rotate[:] = 33.0       # affine_on is False: none of these may act
    for params in (None, AugmentParams.identity(3), ident):
        gi, go, gv = augment_batch(ti, tm, params, 5, crop, rescale=None, verts=tv)
        assert gi.dtype == torch.float32 and go.dtype == torch.uint8 and gi.shape == ri.shape and go.shape == ro.shape
        assert torch.equal(gi, ri) and torch.equal(go, ro) and torch.equal(gv, rv)
        assert np.array_equal(gi.cpu().numpy(), oi) and np.array_equal(go.cpu().numpy(), oo) and np.array_equal(gv.cpu().numpy(), ov)


@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("ud", [False, True])
def test_flips_are_bit_exact(dev, lr, ud):
    from oracle import batch as OB
    from pointcloududa_amd.utils.augment import AugmentParams, augment_batch, light_aug, simple_aug
    rng = np.random.default_rng(21)
    b, h, w, c = 2, 200, 231, 3
    img = rng.normal(0, 1, (b, h, w, c)).astype(np.float32)
    u8 = rng.integers(0, 256, (b, h, w, c)).astype(np.uint8)
    m = rng.integers(0, 5, (b, h, w)).astype(np.int64)

    def flip(a):
        a = a[:, :, ::-1] if lr else a
        return np.ascontiguousarray(a[:, ::-1] if ud else a)
    for oo in ((0, 1, 2), (2, 1, 0)):
        p = AugmentParams.identity(b)
        p.flip_lr[:] = lr; p.flip_ud[:] = ud; p.order[:] = 1; p.cval[:] = 255; p.op_order = oo
        for crop in (0, 100):
            oi, oh, _ = OB.assemble_batch(flip(img), flip(m)[..., None], np.zeros((b, 300, 3)), num_classes=5, crop_size=crop)
            gi, go, gv = augment_batch(torch.from_numpy(img).to(dev), torch.from_numpy(m).to(dev), p, 5, crop, rescale=None)
            assert gv is None and np.array_equal(gi.cpu().numpy(), oi) and np.array_equal(go.cpu().numpy(), oh)
        gu, gm = light_aug(torch.from_numpy(u8).to(dev), torch.from_numpy(m).to(dev), p)
        assert gu.dtype == torch.uint8 and gm.dtype == torch.int64
        assert np.array_equal(gu.cpu().numpy(), flip(u8)) and np.array_equal(gm.cpu().numpy(), flip(m))
        assert np.array_equal(light_aug(torch.from_numpy(u8).to(dev), None, p).cpu().numpy(), flip(u8))
    # one sample flipped, the other not; simple_aug on a single [H,W,C] image with its [H,W,1] mask
    p = AugmentParams.identity(b)
    p.flip_lr[1] = lr; p.flip_ud[1] = ud
    gu = light_aug(torch.from_numpy(u8).to(dev), None, p).cpu().numpy()
    assert np.array_equal(gu[0], u8[0]) and np.array_equal(gu[1], flip(u8)[1])
    p1 = AugmentParams.identity(1)
    p1.flip_lr[:] = lr; p1.flip_ud[:] = ud
    su, sm = simple_aug(torch.from_numpy(u8[0]).to(dev), torch.from_numpy(m[0][..., None]).to(dev), p1)
    assert su.shape == (h, w, c) and sm.shape == (h, w, 1)
    assert np.array_equal(su.cpu().numpy(), flip(u8)[0]) and np.array_equal(sm.cpu().numpy()[..., 0], flip(m)[0])


# ---------------------------------------------------------------------------------------------- affine
def test_fixture_excused_pixels_are_rare():
    pixels = sum(c["u8"].size + c["mask"].size for c in CASES)
    assert sum(len(c["exc_img"]) + len(c["exc_mask"]) for c in CASES) <= 1e-5 * pixels


@pytest.mark.parametrize("name", NAMES)
def test_affine_warp_matches_the_helper(dev, name):
    from oracle import batch as OB
    from pointcloududa_amd.utils.augment import augment_batch, light_aug
    case = _case(name)
    x, q, mn, mx, lab = G.case_inputs(case)
    params = _params(case)
    tq, tl = torch.from_numpy(q).to(dev), torch.from_numpy(lab).to(dev)
    gi, go, _ = augment_batch(tq, tl, params, case["k"], 0, rescale=None)          # uint8 in, float(q') out
    got = _to_u8_hwc(gi)
    _check_images(case, got, q)
    gu, gm = light_aug(tq, tl, params)                                              # the same warp, uint8 out, labels out
    assert np.array_equal(gu.cpu().numpy(), got)
    same = _check_masks(case, gm.cpu().numpy(), lab)
    exp_oh = OB.to_categorical(case["mask"].astype(np.int64), case["k"])
    goh = go.cpu().numpy()
    assert goh.shape == exp_oh.shape
    keep = np.broadcast_to(same[:, None], goh.shape)
    assert np.array_equal(goh[keep], exp_oh[keep])
    assert np.array_equal(goh, OB.to_categorical(gm.cpu().numpy(), case["k"]))      # and it is the one-hot of the labels it warped


@pytest.mark.parametrize("name", [c["name"] for c in CASES if "minmax_f32" in c])
@pytest.mark.parametrize("crop", [0, 40])
def test_rescale_paths_are_bit_exact(dev, name, crop):
    from oracle import batch as OB
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.augment import augment_batch
    case = _case(name)
    x, q, mn, mx, lab = G.case_inputs(case)
    params = _params(case)
    tx, tq, tl = torch.from_numpy(x).to(dev), torch.from_numpy(q).to(dev), torch.from_numpy(lab).to(dev)
    mm = K.minmax(tx).cpu().numpy()
    assert mm.dtype == np.float32 and mm[0] == mn == case["minmax"][0] and mm[1] == mx == case["minmax"][1]
    u8 = _to_u8_hwc(augment_batch(tq, tl, params, case["k"], 0, rescale=None)[0])
    same = _check_images(case, u8, q)
    verts = np.zeros((case["b"], 300, 3), dtype=np.int64)
    for mode, src, exp in (("minmax", tx, case["minmax_f32"]), ("div255", tq, case["div255_f32"])):
        ei, _, _ = OB.assemble_batch(exp, case["mask"][..., None].astype(np.int64), verts, num_classes=case["k"], crop_size=crop)
        keep, _, _ = OB.assemble_batch(same, case["mask"][..., None].astype(np.int64), verts, num_classes=case["k"], crop_size=crop)
        gi, _, _ = augment_batch(src, tl, params, case["k"], crop, rescale=mode)
        gi = gi.cpu().numpy()
        assert gi.dtype == np.float32 and gi.shape == ei.shape and keep.mean() > 0.999
        assert np.array_equal(gi[keep], ei[keep]), (mode, int((gi != ei)[keep].sum()))


def test_constant_batch_gives_min_everywhere(dev):
    """max == min: q is 0 everywhere (documented; the reference casts a NaN to uint8), so every output equals min"""
    from pointcloududa_amd.utils.augment import augment_batch
    case = _case("heavy_96x80")
    _, _, _, _, lab = G.case_inputs(case)
    x = torch.full((case["b"], case["h"], case["w"], 2), 3.25, dtype=torch.float32, device=dev)
    gi, go, _ = augment_batch(x, torch.from_numpy(lab).to(dev), _params(case), case["k"], 0, rescale="minmax")
    assert gi.shape == (case["b"], 2, case["h"], case["w"]) and bool((gi == 3.25).all())
    assert np.array_equal(go.cpu().numpy().argmax(1)[case["mask"] > 0], case["mask"][case["mask"] > 0])


@pytest.mark.parametrize("name", [c["name"] for c in CASES if "verts" in c])
@pytest.mark.parametrize("fused", [True, False])
def test_vertices_are_resampled_from_the_full_warped_mask(dev, name, fused):
    from pointcloududa_amd.utils.augment import augment_batch
    case = _case(name)
    assert len(case["exc_mask"]) == 0
    x, q, mn, mx, lab = G.case_inputs(case)
    gi, go, gv = augment_batch(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), _params(case), case["k"], 224,
                               rescale="minmax", resample_verts=True, fused_mask=fused)
    ref = case["verts"].astype(np.float32) / np.float32(255.0)
    assert gv.dtype == torch.float32 and np.array_equal(gv.cpu().numpy(), ref)
    assert gi.shape == (case["b"], case["c"], 224, 224) and go.shape == (case["b"], case["k"], 224, 224)
    if name == "out_of_frame":
        assert np.all(case["area"][:2] <= 50) and not gv[:2].any() and bool(gv[2].any())


def test_one_call_equals_flip_then_affine(dev):
    """flip-then-affine in one call against a flip-only call followed by an affine-only call"""
    from pointcloududa_amd.utils.augment import light_aug
    case = [c for c in CASES if c["op_order"] == (0, 1, 2) and c["b"] == 5 and c["name"].startswith("ops_")][0]
    assert np.any(case["params"]["flip_lr"] & case["params"]["affine_on"]) or np.any(case["params"]["flip_ud"] & case["params"]["affine_on"])
    _, q, _, _, lab = G.case_inputs(case)
    tq, tl = torch.from_numpy(q).to(dev), torch.from_numpy(lab).to(dev)
    off = np.zeros(case["b"], dtype=bool)
    one_u, one_m = light_aug(tq, tl, _params(case))
    fu, fm = light_aug(tq, tl, _params(case, affine_on=off))
    two_u, two_m = light_aug(fu, fm, _params(case, flip_lr=off, flip_ud=off))
    ei, em = _excused_masks(case)
    one_u, two_u, one_m, two_m = one_u.cpu().numpy(), two_u.cpu().numpy(), one_m.cpu().numpy(), two_m.cpu().numpy()
    assert np.array_equal(one_u[~ei], two_u[~ei]) and np.array_equal(one_m[~em], two_m[~em])
    _check_images(case, two_u, q)
    _check_masks(case, two_m, lab)


# ---------------------------------------------------------------------------------------------- the loader wrapper
def test_augmented_batches_feed_train_epoch_shapes(dev):
    from oracle.synth import synth_batch
    from pointcloududa_amd.utils.augment import AugmentParams, AugmentedBatches, augment_batch, sample_params
    raw = []
    for i in range(3):
        lab = np.argmax(synth_batch(4, 1, 5, 256, seed=40 + i)[1], axis=1).astype(np.int64)[..., None]
        raw.append((G.smooth_images(4, 256, 256, 3, 50 + i), lab))
    it = AugmentedBatches(iter(raw), dev, "mmwhs_light", np.random.default_rng(77), num_classes=5, crop_size=224)
    twin = np.random.default_rng(77)
    n = 0
    for (x, y, z), (img, lab) in zip(it, raw):
        assert x.dtype == torch.float32 and x.shape == (4, 3, 224, 224) and x.device.type == "cuda"
        assert y.dtype == torch.uint8 and y.shape == (4, 5, 224, 224) and z.dtype == torch.float32 and z.shape == (4, 300, 3)
        want = sample_params(4, "mmwhs_light", twin)
        for k in AugmentParams.__dataclass_fields__:
            assert np.array_equal(getattr(want, k), getattr(it.last_params, k)), k
        rx, ry, rz = augment_batch(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), want, 5, 224, "minmax",
                                   resample_verts=True)
        assert torch.equal(x, rx) and torch.equal(y, ry) and torch.equal(z, rz)
        n += 1
    assert n == 3
    with pytest.raises(StopIteration):
        next(it)
    with pytest.raises(NotImplementedError, match="out of scope"):
        AugmentedBatches(iter(raw), dev, "heavy", np.random.default_rng(0))


def test_augment_batch_adds_no_host_synchronisation(dev):
    """the resample_verts=False path under torch.cuda.set_sync_debug_mode("error"); the mode is first shown to be enforced
    by this torch build (a ``.item()`` raises under it)"""
    from pointcloududa_amd.utils.augment import augment_batch
    case = _case("ops_012_mmwhs_light")
    x, q, mn, mx, lab = G.case_inputs(case)
    tx, tq, tl = torch.from_numpy(x).to(dev), torch.from_numpy(q).to(dev), torch.from_numpy(lab).to(dev)
    params = _params(case)
    ref = augment_batch(tx, tl, params, case["k"], 40, rescale="minmax")             # (warm: allocator, library load)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        a = augment_batch(tx, tl, params, case["k"], 40, rescale="minmax")
        b = augment_batch(tq, tl, params, case["k"], 40, rescale="div255")
        c = augment_batch(tx, tl, None, case["k"], 0, rescale=None)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a[0], ref[0]) and torch.equal(a[1], ref[1]) and b[0].shape == a[0].shape and c[2] is None
