"""The native-size evaluation of MS-CMRSeg on the device (csrc/area_resize.hip), bit for bit: the plain
resize against tests/golden/area_resize.npz and the digests of tests/golden/area_resize_edges.json (scripts/make_area_resize_golden.py),
the fused reconstruct / resize / argmax against argmax over the plain resize of the materialised canvas, and
evaluate_mscmrseg.evaluate_segmentation against the composition of its parts."""
import numpy as np
import pytest
import torch

from area_resize_ref import EDGES, G, GOLD, same_bits

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- the plain resize
@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_six_sizes_equal_the_golden_file(dev, size):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import utils as U
    w, h = size
    src = torch.from_numpy(GOLD["src"]).to(dev)
    want = GOLD["out_%dx%d" % (w, h)]
    assert same_bits(K.area_resize(src, h, w), want)
    assert same_bits(K.area_resize(src[1], h, w), want[1]), "one plane"
    assert same_bits(U.resize_volume(src, w=w, h=h), want) and same_bits(U.resize_volume(GOLD["src"], w=w, h=h), want)
    assert isinstance(U.resize_volume(GOLD["src"], w=w, h=h), np.ndarray)


@pytest.mark.parametrize("size", [(45, 37), (17, 13), (24, 20)], ids=lambda s: "%dx%d" % s)
def test_a_strided_source_is_read_as_it_lies(dev, size):
    from pointcloududa_amd import kernels as K
    w, h = size
    src = GOLD["src"]
    big = torch.full((4, 23, 31), 7.5, dtype=torch.float32, device=dev)
    view = big[::2, 2:22, 3:27]                     # plane stride 2 * 713, row stride 31, an address that is no multiple of 16
    view.copy_(torch.from_numpy(src).to(dev))
    assert view.stride() == (1426, 31, 1) and view.data_ptr() % 16 != 0
    assert same_bits(K.area_resize(view, h, w), GOLD["out_%dx%d" % (w, h)])
    assert float(big[1].min()) == 7.5 and float(big[0, 0].max()) == 7.5, "the source is never written"
    cols = torch.from_numpy(src).to(dev).transpose(1, 2).contiguous().transpose(1, 2)      # no unit column stride: copied by the wrapper
    assert cols.stride(2) != 1 and same_bits(K.area_resize(cols, h, w), GOLD["out_%dx%d" % (w, h)])


def test_a_patch_too_large_to_stage_is_read_from_memory(dev):
    from pointcloududa_amd import kernels as K
    sw, sh, dw, dh = G.TALL
    assert same_bits(K.area_resize(torch.from_numpy(GOLD["tall_src"]).to(dev), dh, dw), GOLD["tall_out"])


def test_two_calls_agree_and_nothing_synchronises(dev):
    from pointcloududa_amd import kernels as K
    src = torch.from_numpy(GOLD["src"]).to(dev)
    logits = torch.from_numpy(GOLD["fused_logits"]).to(dev)
    f = G.FUSED_SMALL

    def run():
        return K.area_resize(src, 37, 45), K.area_resize(src, 13, 17), K.reconstruct_resize_argmax(logits, 23, 29, f["crop"], f["origin"])

    want = run()
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        got = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- fused against unfused
def unfused(logits, h, w, crop, origin):
    """the reference's order on the device with every intermediate in memory: ``reconstuct_volume`` (channels last), the resize of
    every class plane, ``argmax``"""
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import metric as M
    canvas = EM.reconstuct_volume(logits.permute(0, 2, 3, 1).contiguous(), crop, origin)          # [N,origin,origin,C]
    planes = torch.stack([K.area_resize(canvas[..., k].contiguous(), h, w) for k in range(logits.shape[1])], dim=1)
    return planes, M.argmax_labels(planes)


@pytest.mark.parametrize("size", G.FUSED_SMALL["sizes"], ids=lambda s: "%dx%d" % s)
def test_the_small_fused_case_equals_the_golden_file(dev, size):
    from pointcloududa_amd import kernels as K
    f = G.FUSED_SMALL
    w, h = size
    logits = torch.from_numpy(GOLD["fused_logits"]).to(dev)
    got = K.reconstruct_resize_argmax(logits, h, w, f["crop"], f["origin"])
    assert same_bits(got, GOLD["fused_labels_%dx%d" % (w, h)])
    assert torch.equal(got, unfused(logits, h, w, f["crop"], f["origin"])[1])


@pytest.mark.parametrize("c", (1, 4, 5, 8))
def test_fused_equals_argmax_over_the_resized_canvas(dev, c):
    """crop 20 in a canvas of 48 (and of 47: an odd canvas), N = 3, to an enlargement past one row of tiles, the equal size, a
    shrink, and a mixed size; the logits are negative at the window's rim (the zero canvas wins at the border), hold exact ties
    between classes and with the canvas' zero, and one NaN"""
    from pointcloududa_amd import kernels as K
    x = G.logits_case(3, c, 40, seed=20 + c)
    x[2, c - 1, 17, 23] = np.nan
    logits = torch.from_numpy(x).to(dev)
    seen = set()
    for origin in (48, 47):
        for w, h in ((90, 85), (origin, origin), (31, 29), (90, 29), (44, 36)):
            planes, want = unfused(logits, h, w, 20, origin)
            got = K.reconstruct_resize_argmax(logits, h, w, 20, origin)
            assert got.dtype == torch.uint8 and got.shape == (3, h, w) and torch.equal(got, want), (origin, w, h)
            seen |= set(torch.unique(got).tolist())
            if (w, h) == (origin, origin):
                # equal sizes: the canvas itself; its rim outside the window is zero in every class: class 0
                o = origin // 2
                border = torch.ones((h, w), dtype=torch.bool, device=dev)
                border[o - 20:o + 20, o - 20:o + 20] = False
                assert int(got[:, border].max()) == 0
                inner = torch.from_numpy(G.argmax_rule(x)).to(dev)
                assert torch.equal(got[:, o - 20:o + 20, o - 20:o + 20], inner)
                assert int(got[2, o - 20 + 17, o - 20 + 23]) == 0, "a NaN in any class: label 0"
                if c > 1:
                    q = 10
                    assert int(got[0, o - 20 + q:o - 20 + 2 * q, o - 20 + q:o - 20 + 2 * q].eq(1).sum()) == 0, "a tie of classes 0 and 1 is 0's"
    assert seen == set(range(c)) or c == 1 and seen == {0}, seen
    view = torch.zeros((3, c + 1, 40, 44), dtype=torch.float32, device=dev)[:, 1:, :, 2:42]      # strides of a view, as they lie
    view.copy_(logits)
    assert not view.is_contiguous() and torch.equal(K.reconstruct_resize_argmax(view, 85, 90, 20, 48), unfused(logits, 85, 90, 20, 48)[1])


@pytest.mark.parametrize("size", G.FUSED_LARGE["sizes"], ids=lambda s: "%dx%d" % s)
def test_past_one_tile_and_one_wave_against_the_digests(dev, size):
    """N = 2, C = 4, 224 in a 256 canvas to 480 x 480 (two tiles across, 60 down, the dword stores) and to 511 x 257 (a row
    length that is no multiple of 4: the byte stores and the scalar float stores, a last tile of 255 columns and a last row
    alone in its tile)"""
    from pointcloududa_amd import kernels as K
    f = G.FUSED_LARGE
    w, h = size
    rec = EDGES["cases"]["canvas_%dx%d" % (w, h)]
    assert rec["shape"] == [f["n"], f["c"], h, w]
    logits = torch.from_numpy(G.logits_case(f["n"], f["c"], 2 * f["crop"], seed=11)).to(dev)
    planes, want = unfused(logits, h, w, f["crop"], f["origin"])
    assert G.digest(planes.cpu().numpy()) == rec["planes"]
    got = K.reconstruct_resize_argmax(logits, h, w, f["crop"], f["origin"])
    assert torch.equal(got, want) and G.digest(got.cpu().numpy()) == rec["labels"]
    assert len(torch.unique(got)) == f["c"]


# ---------------------------------------------------------------------------------------------- end to end
def _patient(seed, depth, x_size, y_size):
    """``read_img``'s uint8 stack [Z,256,256,3]: three discs that move from slice to slice, under noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:256, 0:256]
    images = np.zeros((depth, 256, 256, 3), np.float64)
    for d in range(depth):
        for k, (cy, cx, rad) in enumerate(((100, 100, 30), (100, 160, 26), (160, 120, 34))):
            images[d, ..., :][(yy - cy - 2 * d) ** 2 + (xx - cx + d) ** 2 <= rad ** 2] = 70.0 * (k + 1)
    return np.clip(images + rng.standard_normal(images.shape) * 20.0 + 20.0, 0, 255).astype(np.uint8)


def _label_file(model, images, x_size, y_size, absent=None):
    """a label file [X,Y,Z] that overlaps what the fixed weights predict: the prediction at that size (from the unfused parts), each
    class's largest component kept, moved by (3, -2) pixels, class `absent` removed; int16 codes, Fortran order as a NIfTI reader
    returns it"""
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd.utils import utils as U
    lab = U.keep_largest_connected_components(unfused(_logits(model, EM.read_volume(images), 2), y_size, x_size, 112, 256)[1])
    lab = torch.roll(lab, (3, -2), (1, 2)).cpu().numpy()
    if absent is not None:
        lab[lab == absent] = 0
    codes = np.array([0, 200, 500, 600], np.int16)[lab]                   # [Z,Y,X]
    return np.asfortranarray(codes.transpose(2, 1, 0))


@pytest.fixture(scope="module")
def end_to_end(dev):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd.networks import Segmentation_model_Point
    torch.manual_seed(7)
    model = Segmentation_model_Point(filters=4, in_channels=3, n_class=4, pointnet=False, heinit=True).to(dev).eval()
    with torch.no_grad():
        model.classifier.bias.copy_(torch.tensor([0.05, -0.05, 0.0, 0.02]))
    patients = []
    for pat_id, seed, depth, x_size, y_size, absent in ((6, 910, 3, 256, 256, None), (7, 911, 4, 320, 288, None), (8, 912, 5, 200, 232, 2)):
        images = _patient(seed, depth, x_size, y_size)
        patients.append((pat_id, images, _label_file(model, images, x_size, y_size, absent)))
    out = EM.evaluate_segmentation(model, patients, bs=2, model_name="d4", toprint=False)
    return model, patients, out


def _logits(model, x, bs):
    with torch.no_grad():
        return torch.cat([model(x[i:i + bs])[0] for i in range(0, x.shape[0], bs)])


def test_read_volume_is_crop_divide_moveaxis(dev, end_to_end):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    images = end_to_end[1][1][1]
    want = np.moveaxis(np.array(images[:, 128 - 112:128 + 112, 128 - 112:128 + 112], np.float32) / 255., -1, 1)
    assert want.dtype == np.float32 and want.shape == (4, 3, 224, 224)
    assert same_bits(EM.read_volume(images), want) and same_bits(EM.read_volume(torch.from_numpy(images).to(dev), 224), want)
    small = np.moveaxis(np.array(images[:, 128 - 48:128 + 48, 128 - 48:128 + 48], np.float32) / 255., -1, 1)
    assert same_bits(EM.read_volume(images, crop_size=96), small)
    vol = torch.from_numpy(np.ascontiguousarray(np.moveaxis(want[:, :, :12, :12], 1, -1))).to(dev)
    assert same_bits(EM.reconstuct_volume(vol, 6, 16), np.moveaxis(G.reconstruct(want[:, :, :12, :12], 6, 16), 1, -1))


def test_evaluate_segmentation_equals_the_composition_of_its_parts(dev, end_to_end):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd.utils import metric as M
    from pointcloududa_amd.utils import utils as U
    model, patients, out = end_to_end
    assert list(out["per_patient"]) == [6, 7, 8] and len(out["rows"]) == 9
    lut = torch.arange(256, dtype=torch.int32, device=dev)
    lut[1:4] = torch.tensor([200, 500, 600], dtype=torch.int32, device=dev)
    classes = set()
    for p, (pat_id, images, nimg) in enumerate(patients):
        x_size, y_size, depth = nimg.shape
        logits = _logits(model, EM.read_volume(images), 2)
        assert logits.shape == (depth, 4, 224, 224)
        planes, lab = unfused(logits, y_size, x_size, 112, 256)
        assert planes.shape == (depth, 4, y_size, x_size)
        classes |= set(torch.unique(lab).tolist())
        pred = lut[U.keep_largest_connected_components(lab).long()]
        gt = torch.from_numpy(np.ascontiguousarray(nimg.T).astype(np.int32)).to(dev)
        want = EM.metrics_from_rows(M.class_metrics(gt, pred, EM.CLASSES).tolist(), True, True)
        got = out["per_patient"][pat_id]
        print("patient %d: %s" % (pat_id, got))
        assert len(got) == 9 and got == want, (pat_id, got, want)
        assert out["rows"][3 * p:3 * p + 3] == [got[0:3] + ["lv", "d4", pat_id], got[3:6] + ["rv", "d4", pat_id], got[6:9] + ["myo", "d4", pat_id]]
    assert len(classes) > 1, "the fixed weights predict more than one class"
    assert out["per_patient"][8][0:3] == [-1, -1, -1], "the third label file holds no endo (500): the -1 triplet"
    assert any(0.0 < res[k] < 1.0 for res in out["per_patient"].values() for k in (0, 3, 6)), "a Dice strictly between 0 and 1"
    assert all(res[4] > 0 for res in out["per_patient"].values()), "the label files are the predictions moved by (3, -2)"
    assert out["table"] == EM.summary_table(list(out["per_patient"].values()))


def test_native_shape_through_evaluate_volume_and_none_as_before(dev, end_to_end):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd import validate as V
    from pointcloududa_amd.utils import metric as M
    from pointcloududa_amd.utils import utils as U
    model, patients, out = end_to_end
    pat_id, images, nimg = patients[1]
    x, gt = EM.read_volume(images), EM.read_labels(nimg)
    assert V.evaluate_volume(model, x, gt, bs=2, variant="mscmrseg", native_shape=nimg.shape[:2]) == out["per_patient"][pat_id]
    ext = V.evaluate_volume(model, x, gt, bs=2, variant="mscmrseg", native_shape=nimg.shape[:2], extended=True)
    assert len(ext) == 15 and [ext[5 * k + n] for k in range(3) for n in range(3)] == out["per_patient"][pat_id]
    assert EM.evaluate_segmentation(model, patients[1:2], bs=2, extended=True, toprint=False)["per_patient"][pat_id] == ext
    # native_shape=None: labels of the network's own size, nothing resized
    gt224 = torch.from_numpy(np.ascontiguousarray(nimg.T[:, :224, :224]).astype(np.int32)).to(dev)
    lut = torch.arange(256, dtype=torch.int32, device=dev)
    lut[1:4] = torch.tensor([200, 500, 600], dtype=torch.int32, device=dev)
    pred = lut[U.keep_largest_connected_components(M.argmax_labels(_logits(model, x, 8))).long()]
    want = EM.metrics_from_rows(M.class_metrics(gt224, pred, EM.CLASSES).tolist(), True, True)
    assert V.evaluate_volume(model, x, gt224, variant="mscmrseg") == want
    assert V.evaluate_volume(model, x, gt224, variant="mscmrseg", native_shape=None, crop_size=100, origin_size=300) == want
    assert EM.metrics_from_rows(V.evaluate_volume_rows(model, x, gt224, variant="mscmrseg").tolist(), True, True) == want
    with pytest.raises(ValueError, match="variant='mscmrseg'"):
        V.evaluate_volume(model, x, gt, variant="mmwhs", native_shape=(320, 288))


def test_the_patient_loop_does_not_synchronise_before_its_end(dev, end_to_end):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd import validate as V
    from pointcloududa_amd.utils import volume as VOL
    model, patients, out = end_to_end
    pat_id, images, nimg = patients[2]
    images, nimg_d = torch.from_numpy(images).to(dev), VOL.as_device_volume(nimg)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        rows = V.evaluate_volume_rows(model, EM.read_volume(images), EM.read_labels(nimg_d), bs=2, variant="mscmrseg",
                                      native_shape=(200, 232))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert EM.metrics_from_rows(rows.tolist(), True, True) == out["per_patient"][pat_id]
