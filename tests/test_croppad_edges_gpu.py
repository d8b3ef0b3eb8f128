"""Device-side CropAndPad (csrc/croppad.hip) at the shapes where the kernels leave the paths that
tests/golden/croppad.npz reaches: more than one x tile, C = 2 and 4, both store paths of images and labels (and outputs that
are not aligned for them), cropped lines longer than a wave, ramp flags behind the first 256 edge values, pads of exactly 64,
and the workload's 256 x 256 x 3 and 224 x 224 x 1 (tests/croppad_edge_cases.py).

Expected arrays are the plain restatement of scripts/make_croppad_golden.py, computed here; before anything is compared with
one, its sha256 is compared with tests/golden/croppad_edges.json, which was written only after the restatement had equalled
numpy.pad on every row.  Every comparison is bit for bit."""
import json

import numpy as np
import pytest
import torch

import croppad_edge_cases as T

pytestmark = pytest.mark.gpu

G = T.G
RECORDED = json.load(open(T.JSON_PATH))["cases"]
_CHECKED = set()


def _case(name):
    """the case, its recorded digests asserted once against the restatement as this machine's numpy computes it"""
    cs = T.BY_NAME[name]
    if name not in _CHECKED:
        assert T.digests_of(cs) == RECORDED[name], "the restatement here is not the one that was checked against numpy.pad: " + name
        _CHECKED.add(name)
    return cs


def _outs(cs):
    return [o for _, o in T.expected_rows(cs)]


def _program(args, copies=()):
    from pointcloududa_amd.utils.augment import CropPadProgram
    p = CropPadProgram.identity(len(args))
    for i, a in enumerate(args):
        if i not in copies:
            p.set_crop_and_pad(i, *(int(v) for v in a))
    return p


def _run(dev, images, program, masks=None):
    from pointcloududa_amd.utils.augment import crop_pad_aug
    x = torch.from_numpy(np.array(images)).to(dev)                      # (a copy: the table's arrays are read-only)
    m = None if masks is None else torch.from_numpy(np.array(masks)).to(dev)
    keep, keep_m = x.clone(), None if m is None else m.clone()
    out, mo = crop_pad_aug(x, m, program)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x, keep), "the input is never written"
    if masks is None:
        assert mo is None
        return out.cpu().numpy()
    assert mo.dtype == m.dtype and mo.shape == m.shape and torch.equal(m, keep_m)
    return out.cpu().numpy(), mo.cpu().numpy()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())


def _rep(a, n):
    return np.repeat(a[None], n, axis=0)


MODE_CASES = [cs.name for cs in T.CASES if cs.kind == "modes"]


@pytest.mark.parametrize("name", MODE_CASES)
def test_every_mode_at_every_edge_shape(dev, name):
    """per side-set offset one batch of ten samples, sample m in mode m; then every row alone, against the same arrays"""
    cs = _case(name)
    img, want = T.image_of(cs), _outs(cs)
    for r in range(len(cs.sets)):
        rows = cs.rows[10 * r:10 * r + 10]
        got = _run(dev, _rep(img, 10), _program(rows))
        for m in range(10):
            _same(got[m], want[10 * r + m], (name, "batch", r, rows[m]))
    for i, row in enumerate(cs.rows):
        _same(_run(dev, img[None], _program([row]))[0], want[i], (name, "alone", row))


@pytest.mark.parametrize("name", ("two_tiles_full", "two_tiles_tail_c1", "two_tiles_tail_c3", "c4_tail", "c4_full", "production_256",
                                  "production_224"))
def test_masks_on_the_vector_and_scalar_label_paths(dev, name):
    """W % 4 == 0 stores labels as 16 bytes, every other width one by one; negative and large labels pass through unchanged, and
    the image's mode does not matter"""
    cs = _case(name)
    img, lab = T.image_of(cs), T.labels_of(cs)
    assert set(T.LABEL_VALUES) == set(np.unique(lab).tolist())
    for sides, want in zip(cs.sets, T.expected_labels(cs)):
        args = [tuple(sides) + (m, 200) for m in range(10)]
        for dtype in (np.int32, np.int64):
            for tail in ((), (1,)):
                masks = _rep(lab, 10).astype(dtype).reshape((10, cs.h, cs.w) + tail)
                _, got = _run(dev, _rep(img, 10), _program(args), masks)
                assert got.dtype == dtype and got.shape == masks.shape
                for m in range(10):
                    _same(got[m].reshape(cs.h, cs.w), want.astype(dtype), ("mask", name, sides, m, dtype.__name__, tail))


@pytest.mark.parametrize("name", ("two_tiles_full", "c2_vec_tail", "c4_full"))
def test_misaligned_outputs_take_the_scalar_stores_with_the_same_bytes(dev, name):
    """shapes whose aligned outputs take the 32-bit image stores (and, at W % 4 == 0, the 16-byte label stores): `out` one
    byte, `labels_out` one int32 into a larger allocation, both and each alone; nothing is written around them"""
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.croppad import upload_crop_pad_program
    cs = _case(name)
    h, w, c = cs.h, cs.w, cs.c
    assert (w * c) % 4 == 0
    want_all, lab = _outs(cs), T.labels_of(cs)
    x = torch.from_numpy(_rep(T.image_of(cs), 10)).to(dev)
    li = torch.from_numpy(_rep(lab, 10)).to(dev)
    keep, keep_l = x.clone(), li.clone()
    n_img, n_lab = x.numel(), li.numel()
    for r in (0, 3):
        rows = cs.rows[10 * r:10 * r + 10]
        want = np.stack(want_all[10 * r:10 * r + 10])
        want_lab = np.stack([T.expected_labels(cs)[(r + m) % len(cs.sets)] for m in range(10)])
        up = upload_crop_pad_program(_program(rows), 10, h, w, dev)
        ref, ref_lab = K.crop_pad(x, li, *up)
        assert ref.data_ptr() % 4 == 0 and ref_lab.data_ptr() % 16 == 0
        _same(ref.cpu().numpy(), want, (name, r, "aligned"))
        _same(ref_lab.cpu().numpy(), want_lab, (name, r, "aligned labels"))
        for off_img, off_lab in ((1, 1), (1, 4), (16, 1)):
            obuf = torch.full((n_img + 32,), 0xA5, dtype=torch.uint8, device=dev)
            lbuf = torch.full((n_lab + 8,), -1234567, dtype=torch.int32, device=dev)
            out = obuf[off_img:off_img + n_img].view(10, h, w, c)
            lout = lbuf[off_lab:off_lab + n_lab].view(10, h, w)
            assert out.is_contiguous() and lout.is_contiguous()
            assert out.data_ptr() % 4 == off_img % 4 and lout.data_ptr() % 16 == (4 * off_lab) % 16      # 1 or 0; 4 or 0
            res, res_lab = K.crop_pad(x, li, *up, out=out, labels_out=lout)
            assert res.data_ptr() == out.data_ptr() and res_lab.data_ptr() == lout.data_ptr()
            what = (name, r, off_img, off_lab)
            assert torch.equal(out, ref) and torch.equal(lout, ref_lab), what
            _same(out.cpu().numpy(), want, what)
            _same(lout.cpu().numpy(), want_lab, what)
            assert bool((obuf[:off_img] == 0xA5).all()) and bool((obuf[off_img + n_img:] == 0xA5).all()), what
            assert bool((lbuf[:off_lab] == -1234567).all()) and bool((lbuf[off_lab + n_lab:] == -1234567).all()), what
    assert torch.equal(x, keep) and torch.equal(li, keep_l), "the inputs are never written"


def test_ramp_flags_beyond_the_first_256_edge_values(dev):
    """130 x 90 x 3, pads of 55: one texel equal to the end value on one side, behind index 256 of that side's flag loop,
    turns that side (and no other) to linspace's k / width form"""
    order = ("top", "right", "bottom", "left", "none_all", "none_lr")
    cases = [_case("max_pad_ramp_" + s) for s in order]
    rows = [cs.rows[0] for cs in cases]
    assert all(r[4] == 2 and r[5] == T.RAMP_CVAL for r in rows)
    got = _run(dev, np.stack([T.image_of(cs) for cs in cases]), _program(rows))
    for i, cs in enumerate(cases):
        _same(got[i], _outs(cs)[0], cs.name)
        _same(_run(dev, T.image_of(cs)[None], _program(rows[i:i + 1]))[0], _outs(cs)[0], (cs.name, "alone"))
    for i, side in enumerate(order[:4]):
        sides = T.RAMP_PLANTS[side][1]
        plain = got[order.index("none_all" if sides == T.RAMP_ALL else "none_lr")]
        # output texels that read that side's pad region alone differ by the form; those that read nothing of it (and not
        # the planted texel) are the unplanted image's
        inside, outside = T.ramp_output_regions(side)
        diff = (got[i] != plain).any(-1)
        assert diff[inside].any() and not diff[outside].any(), side


@pytest.mark.parametrize("name", [cs.name for cs in T.CASES if cs.kind == "stats"])
def test_statistics_over_lines_longer_than_a_wave(dev, name):
    """80 x 70 x 3 in maximum, mean, median and minimum: three grey levels (tied medians, the histogram's first and last bin),
    one value per channel, lines of 66 whose mean and median are k + 0.5; pure top / bottom pads (the pad rows' own
    statistics are statistics of statistics), pure left / right pads, both"""
    cs = _case(name)
    img, want = T.image_of(cs), _outs(cs)
    got = _run(dev, _rep(img, len(cs.rows)), _program(cs.rows))
    for i, row in enumerate(cs.rows):
        _same(got[i], want[i], (name, row))
    for i, row in enumerate(cs.rows):
        _same(_run(dev, img[None], _program([row]))[0], want[i], (name, "alone", row))


def _plan_with_crop(b, h, w, seed):
    from pointcloududa_amd.utils.augment import CropPadProgram, sample_heavy_plan
    rng = np.random.default_rng(seed)
    while True:
        plan = sample_heavy_plan(b, "heavy_refpad_device", rng, h, w)
        crop = [s for s in plan.stages if isinstance(s, CropPadProgram)]
        if crop and len(set(crop[0].iarg[crop[0].opcode == 1][:, 4])) >= 3:
            return crop[0]


@pytest.mark.parametrize("name", ("production_256", "production_224"))
def test_production_geometry_equals_the_restatement(dev, name):
    """the workload's shapes with masks, every sample of a batch with its own sides; at 256 also the CropPadProgram of a drawn
    heavy_refpad_device plan, alone, against the restatement (and numpy.pad itself) row by row"""
    cs = _case(name)
    img, lab, want, want_lab = T.image_of(cs), T.labels_of(cs), _outs(cs), T.expected_labels(cs)
    for r in range(len(cs.sets)):
        rows = cs.rows[10 * r:10 * r + 10]
        got, glab = _run(dev, _rep(img, 10), _program(rows), _rep(lab, 10).astype(np.int64)[..., None])
        for m in range(10):
            _same(got[m], want[10 * r + m], (name, r, rows[m]))
            _same(glab[m, :, :, 0], want_lab[(r + m) % len(cs.sets)].astype(np.int64), (name, "mask", r, rows[m]))
    if name != "production_256":
        return
    stage = _plan_with_crop(10, 256, 256, 21)
    x = np.stack([np.roll(img, 17 * i, axis=(0, 1)) for i in range(10)])
    masks = np.stack([np.roll(lab, 17 * i, axis=(0, 1)) for i in range(10)])
    got, glab = _run(dev, x, stage, masks)
    live = 0
    for i in range(10):
        if stage.opcode[i] != 1:
            _same(got[i], x[i], ("copy", i))
            _same(glab[i], masks[i], ("copied mask", i))
            continue
        row = tuple(int(v) for v in stage.iarg[i])
        assert G.sides_valid(256, 256, *row[:4])
        big, res = G.crop_pad_restated(x[i], *row)
        assert np.array_equal(big, G.crop_pad_restated(x[i], *row, pad_fn=G.numpy_pad)[0]), row
        _same(got[i], res, ("drawn", i, row))
        _same(glab[i], G.labels_restated(masks[i], *row[:4]), ("drawn mask", i, row))
        live += 1
    assert live >= 3
