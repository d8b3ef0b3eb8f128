"""The test-volume reader of the evaluate scripts on the device (pointcloududa_amd/utils/volume.py, csrc/evalprep.hip; DESIGN.md
section 6, f13) against numpy, bit for bit: the expected arrays are restated here in plain numpy from seeded inputs (moveaxis,
the mirrored axes, the wrapped neighbour slices, the chained np.where, the class test), nothing is read from a file.  Shapes:
odd sizes, sizes below, at and above the 64 x 64 tile, depth 1 and 2 (the wrap meets itself), a depth of more than one tile.
Memory orders: C (the slice axis fastest: the tile kernel over z), Fortran (the first axis fastest: the tile kernel over r), the
slice axis in the middle (the columns fastest: the row kernels), and views with no unit stride (the gather)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(33, 47, 5), (64, 64, 1), (64, 64, 2), (32, 32, 3), (40, 24, 70), (7, 129, 4)]
ORDERS = ["C", "F", "middle"]
FLIPS = [(False, False), (False, True), (True, False), (True, True)]
SLICE_DTYPES = [np.float32, np.float64, np.int16, np.uint8]
LABEL_DTYPES = [np.uint8, np.int16, np.int32, np.float32, np.float64]


# ---------------------------------------------------------------------------------------------- inputs and the restatement
def values(shape, dtype, seed):
    """a seeded [H,W,D] array in C order; float64 values are not representable in float32 (the cast must round)"""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if dtype == np.int16:
        return rng.integers(-2000, 3000, shape).astype(np.int16)
    return (rng.standard_normal(shape) * 400.0).astype(dtype)


def laid_out(a, order):
    """the same [H,W,D] values in another memory order"""
    if order == "C":
        return np.ascontiguousarray(a)
    if order == "F":
        return np.asfortranarray(a)
    return np.ascontiguousarray(a.transpose(0, 2, 1)).transpose(0, 2, 1)        # memory [H][D][W]: the slice axis in the middle


def oriented(vol, axis, flip):
    v = np.moveaxis(vol, axis, 0)
    if flip[0]:
        v = v[:, ::-1, :]
    if flip[1]:
        v = v[:, :, ::-1]
    return v


def expect_slices(vol, axis, flip, window):
    v = oriented(vol, axis, flip).astype(np.float32)
    depth = v.shape[0]
    if window == 1:
        return np.ascontiguousarray(v[:, None])
    out = np.empty((depth, 3) + v.shape[1:], np.float32)
    for i in range(depth):
        for k in range(3):
            out[i, k] = v[(i + k - 1) % depth]
    return out


def expect_labels(vol, axis, flip, num_classes, remap):
    """-> (labels uint8, onehot uint8, the number of values that are no class)"""
    v = oriented(vol, axis, flip).astype(np.float64)
    for a, b in remap:
        v = np.where(v == a, float(b), v)
    with np.errstate(invalid="ignore"):
        ok = (v >= 0) & (v < num_classes) & (v == np.floor(v))
    lab = np.where(ok, v, 0.0).astype(np.uint8)
    hot = np.zeros((v.shape[0], num_classes) + v.shape[1:], np.uint8)
    for k in range(num_classes):
        hot[:, k] = ok & (lab == k)
    return lab, hot, int(v.size - np.count_nonzero(ok))


def bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(t, want):
    a = bits(t)
    w = want.view(np.uint32) if want.dtype == np.float32 else want
    return a.shape == w.shape and a.dtype == w.dtype and np.array_equal(a, w)


# ---------------------------------------------------------------------------------------------- slices
def test_the_restatement_says_what_the_reference_lines_say():
    """np.moveaxis(img, 2, 0)[:, ::-1, ::-1] and img[[i - 1, i, (i + 1) % D]] in one go, on a small array"""
    a = values((5, 6, 4), np.int16, 1)
    img = np.moveaxis(a, 2, 0)[:, ::-1, ::-1]
    stack = np.array([img[[i - 1, i, (i + 1) % img.shape[0]]] for i in range(img.shape[0])], dtype=np.float32)
    assert np.array_equal(stack, expect_slices(a, 2, (True, True), 3))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_slices_equal_numpy_in_every_dtype_flip_and_window(dev, shape, order):
    from pointcloududa_amd.utils import volume as VOL
    for n, dtype in enumerate(SLICE_DTYPES):
        vol = laid_out(values(shape, dtype, 100 + n), order)
        on_device = VOL.as_device_volume(vol)
        assert tuple(s * vol.itemsize for s in on_device.stride()) == vol.strides or 1 in shape, "uploaded as it lies"
        for flip in FLIPS:
            for window in (1, 3):
                want = expect_slices(vol, 2, flip, window)
                got = VOL.volume_slices(vol, 2, flip, window)
                assert got.dtype == torch.float32 and got.is_contiguous()
                assert same_bits(got, want), (dtype.__name__, flip, window)
                assert same_bits(VOL.volume_slices(on_device, 2, flip, window), want), "device tensor: %s %s %s" % (dtype.__name__, flip, window)


@pytest.mark.parametrize("order", ORDERS)
def test_window_three_at_depth_one_and_two_by_hand(dev, order):
    from pointcloududa_amd.utils import volume as VOL
    one = laid_out(values((64, 64, 1), np.float32, 7), order)
    s = one[::-1, ::-1, 0]
    got = VOL.volume_slices(one)
    assert same_bits(got, np.ascontiguousarray(np.stack([s, s, s])[None])), "depth 1: three copies of the one slice"
    two = laid_out(values((64, 64, 2), np.int16, 8), order)
    s0, s1 = two[::-1, ::-1, 0].astype(np.float32), two[::-1, ::-1, 1].astype(np.float32)
    want = np.stack([np.stack([s1, s0, s1]), np.stack([s0, s1, s0])])
    assert same_bits(VOL.volume_slices(two), want), "depth 2: slice -1 and slice +1 are the same other slice"
    assert same_bits(VOL.volume_slices(two), expect_slices(two, 2, (True, True), 3))


def test_other_slice_axes_and_views_with_no_unit_stride(dev):
    from pointcloududa_amd.utils import volume as VOL
    big = values((26, 38, 18), np.float64, 11)
    t = torch.from_numpy(big).to(dev)
    for axis in (0, 1, 2, -1):
        for flip in ((True, False), (False, True)):
            assert same_bits(VOL.volume_slices(t, axis, flip, 3), expect_slices(big, axis, flip, 3)), (axis, flip)
    view, host = t[1::2, ::3, ::2], big[1::2, ::3, ::2]                    # strides (1368, 54, 2): the gather
    assert 1 not in view.stride()
    for flip in FLIPS:
        for window in (1, 3):
            assert same_bits(VOL.volume_slices(view, 2, flip, window), expect_slices(host, 2, flip, window)), (flip, window)
            assert same_bits(VOL.volume_slices(view, 0, flip, window), expect_slices(host, 0, flip, window)), (flip, window)
    # a numpy array that is contiguous in no axis order is copied on the host, in its own axis order
    assert same_bits(VOL.volume_slices(host), expect_slices(host, 2, (True, True), 3))
    assert same_bits(VOL.volume_slices(big[::-1]), expect_slices(big[::-1], 2, (True, True), 3))


@pytest.mark.parametrize("dtype", SLICE_DTYPES, ids=lambda d: d.__name__)
def test_a_misaligned_view_takes_the_scalar_path_and_an_aligned_one_the_vector_path(dev, dtype):
    """rows of 32 columns (a multiple of four) at a pitch of 33 behind a storage offset of 1: no group of four is aligned;
    next to it the same values contiguous (the four-column kernel), mirrored and not"""
    from pointcloududa_amd.utils import volume as VOL
    a = values((6, 9, 32), dtype, 21)                                    # [Z][R][C]
    buf = torch.zeros(1 + 6 * 9 * 33, dtype=torch.from_numpy(a).dtype, device=dev)
    view = buf[1:].view(6, 9, 33)[:, :, :32]
    view.copy_(torch.from_numpy(a).to(dev))
    assert view.storage_offset() == 1 and view.stride() == (9 * 33, 33, 1)
    aligned = torch.from_numpy(a).to(dev)
    for flip in FLIPS:
        for window in (1, 3):
            want = expect_slices(a, 0, flip, window)
            assert same_bits(VOL.volume_slices(view, 0, flip, window), want), (flip, window)
            assert same_bits(VOL.volume_slices(aligned, 0, flip, window), want), (flip, window)
    assert not buf[0].item(), "nothing is written to the input"


def test_out_tensor_and_empty_volume(dev):
    from pointcloududa_amd.utils import volume as VOL
    vol = laid_out(values((33, 47, 5), np.int16, 31), "F")
    out = torch.full((5, 3, 33, 47), -7.0, device=dev)
    got = VOL.volume_slices(vol, out=out)
    assert got is out and same_bits(out, expect_slices(vol, 2, (True, True), 3))
    with pytest.raises(ValueError, match="out does not match"):
        VOL.volume_slices(vol, out=torch.empty((5, 1, 33, 47), device=dev))
    for shape in ((4, 6, 0), (0, 6, 3), (4, 0, 3)):
        e = VOL.volume_slices(np.zeros(shape, np.float32))
        assert tuple(e.shape) == (shape[2], 3, shape[0], shape[1]) and e.numel() == 0
        lab = VOL.volume_labels(np.zeros(shape, np.uint8))
        assert tuple(lab.shape) == (shape[2], shape[0], shape[1]) and lab.dtype == torch.uint8
        back = VOL.restore_volume(lab, shape)
        assert tuple(back.shape) == shape


def test_an_offset_beyond_two_to_the_31_is_indexed_in_64_bits(dev):
    """a small view at the far end of a uint8 buffer of 2^31 + 2^20 elements, read through strides whose products with the
    indices pass 2^31: the map's offsets must not wrap"""
    from pointcloududa_amd.utils import volume as VOL
    n = 2 ** 31 + 2 ** 20
    buf = torch.empty(n, dtype=torch.uint8, device=dev)
    z, r, c = 3, 5, 36
    sz, sr = 2 ** 30 + 7, 2 ** 17 + 3
    view = buf.as_strided((z, r, c), (sz, sr, 1), storage_offset=11)
    a = values((z, r, c), np.uint8, 41)
    view.copy_(torch.from_numpy(a).to(dev))
    assert view.storage_offset() + (z - 1) * sz + (r - 1) * sr + c - 1 > 2 ** 31
    assert same_bits(VOL.volume_slices(view, 0, (True, True), 3), expect_slices(a, 0, (True, True), 3))
    tall = buf.as_strided((c, r, z), (1, sr, sz), storage_offset=11)     # the same memory with its first axis fastest: the tile
    assert same_bits(VOL.volume_slices(tall, 2, (False, True), 1), expect_slices(a.transpose(2, 1, 0), 2, (False, True), 1))


# ---------------------------------------------------------------------------------------------- labels
def label_values(shape, dtype, seed, codes=(0, 1, 2, 3, 4)):
    rng = np.random.default_rng(seed)
    return np.asarray(codes)[rng.integers(0, len(codes), shape)].astype(dtype)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(33, 47, 5), (64, 64, 2), (40, 24, 70), (7, 129, 4)], ids=lambda s: "x".join(map(str, s)))
def test_labels_equal_numpy_in_every_dtype(dev, shape, order):
    from pointcloududa_amd.utils import volume as VOL
    for n, dtype in enumerate(LABEL_DTYPES):
        vol = laid_out(label_values(shape, dtype, 200 + n), order)
        for flip in FLIPS:
            lab, hot, stray = expect_labels(vol, 2, flip, 5, ())
            assert stray == 0 and sorted(np.unique(lab).tolist()) == [0, 1, 2, 3, 4]
            got = VOL.volume_labels(vol, 2, flip, 5)
            assert same_bits(got, lab), (dtype.__name__, flip)
            got, got_hot = VOL.volume_labels(vol, 2, flip, 5, onehot=True)
            assert same_bits(got, lab) and same_bits(got_hot, hot), (dtype.__name__, flip)
            assert np.array_equal(np.argmax(got_hot.cpu().numpy(), axis=1), lab), "argmax reads the one-hot back"


@pytest.mark.parametrize("dtype", LABEL_DTYPES, ids=lambda d: d.__name__)
def test_a_remap_in_front_is_applied_in_order(dev, dtype):
    from pointcloududa_amd.utils import volume as VOL
    vol = np.asfortranarray(label_values((20, 28, 6), dtype, 300, codes=(0, 7, 9, 3, 4, 1)))
    remap = ((7, 1), (9, 2), (1, 2), (2, 3))                             # chained: 7 -> 1 -> 2 -> 3, 9 -> 2 -> 3, 1 -> 2 -> 3
    lab, hot, stray = expect_labels(vol, 2, (True, True), 5, remap)
    assert stray == 0 and sorted(np.unique(lab).tolist()) == [0, 3, 4]
    got, got_hot = VOL.volume_labels(vol, num_classes=5, remap=remap, onehot=True)
    assert same_bits(got, lab) and same_bits(got_hot, hot)
    lab2, _, stray2 = expect_labels(vol, 2, (True, True), 5, ((7, 1), (9, 2)))
    assert stray2 == 0 and same_bits(VOL.volume_labels(vol, remap=((7, 1), (9, 2))), lab2)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype", LABEL_DTYPES, ids=lambda d: d.__name__)
def test_values_that_are_no_class_are_counted_and_written_as_background(dev, dtype, order):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import volume as VOL
    vol = label_values((24, 36, 9), dtype, 400)
    bad = (2.5, -1.0, 7.0, float("nan"), 5.0, 4.000001) if dtype in (np.float32, np.float64) else \
        (7, 200, 5) if dtype == np.uint8 else (-1, 7, 5, -32768)
    rng = np.random.default_rng(401)
    where = rng.choice(vol.size, 61, replace=False)
    vol.reshape(-1)[where] = np.asarray(bad, dtype=dtype)[np.arange(61) % len(bad)]
    vol = laid_out(vol, order)
    lab, hot, stray = expect_labels(vol, 2, (True, True), 5, ())
    assert stray == 61
    got, got_hot = VOL.volume_labels(vol, onehot=True, check=False)
    assert same_bits(got, lab) and same_bits(got_hot, hot)
    assert int((hot.sum(axis=1) == 0).sum()) == 61 and not lab[hot.sum(axis=1) == 0].any(), "background, and an all-zero one-hot pixel"
    counter = K.volume_labels(VOL.as_device_volume(vol).movedim(2, 0), True, True, 5)[2]
    assert counter.dtype == torch.int64 and counter.tolist() == [61]
    with pytest.raises(ValueError, match="61 values"):
        VOL.volume_labels(vol)
    # the counter starts from zero on every call
    clean = laid_out(label_values((24, 36, 9), dtype, 402), order)
    assert K.volume_labels(VOL.as_device_volume(clean).movedim(2, 0), True, True, 5)[2].tolist() == [0]
    # with a remap in front the same values can become classes
    if dtype != np.uint8:
        lab_r, _, stray_r = expect_labels(vol, 2, (True, True), 5, ((-1, 1), (7, 2)))
        assert 0 < stray_r < 61
        with pytest.raises(ValueError, match="%d values" % stray_r):
            VOL.volume_labels(vol, remap=((-1, 1), (7, 2)))
        assert same_bits(VOL.volume_labels(vol, remap=((-1, 1), (7, 2)), check=False), lab_r)


@pytest.mark.parametrize("dtype", LABEL_DTYPES[1:], ids=lambda d: d.__name__)
def test_raw_keeps_the_mscmrseg_codes_and_equals_the_transpose(dev, dtype):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd.utils import volume as VOL
    for order in ORDERS:
        nimg = laid_out(label_values((45, 38, 7), dtype, 500, codes=(0, 200, 500, 600)), order)      # [X,Y,Z]
        got = EM.read_labels(nimg)
        assert got.dtype == torch.int32 and same_bits(got, np.ascontiguousarray(nimg.T).astype(np.int32)), order
        assert sorted(np.unique(got.cpu().numpy()).tolist()) == [0, 200, 500, 600]
        want = oriented(nimg, 2, (True, False)).astype(np.int32)
        assert same_bits(VOL.volume_labels(nimg, 2, (True, False), raw=True), want), order


# ---------------------------------------------------------------------------------------------- restore
@pytest.mark.parametrize("shape", [(33, 47, 5), (64, 64, 2), (40, 24, 70), (7, 129, 4)], ids=lambda s: "x".join(map(str, s)))
def test_restore_gives_the_volume_back(dev, shape):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import volume as VOL
    x = label_values(shape, np.uint8, 600)
    for order in ORDERS:
        vol = laid_out(x, order)
        for flip in FLIPS:
            for axis in (2, 0):
                p = VOL.volume_labels(vol, axis, flip)
                for fortran in (True, False):
                    back = VOL.restore_volume(p, shape, axis, flip, fortran=fortran)
                    assert back.dtype == torch.uint8 and tuple(back.shape) == shape
                    assert back.permute(2, 1, 0).is_contiguous() if fortran else back.is_contiguous()
                    assert same_bits(back, x), (order, flip, axis, fortran)
                wide = VOL.restore_volume(p, shape, axis, flip, dtype=torch.int16)
                assert wide.dtype == torch.int16 and same_bits(wide, x.astype(np.int16))
            # into a view of the volume's own memory order (the slice axis in the middle included)
            target = torch.full(shape, 9, dtype=torch.uint8, device=dev) if order == "C" else VOL.as_device_volume(np.full_like(vol, 9))
            K.volume_restore(VOL.volume_labels(vol, 2, flip), target.movedim(2, 0), flip[0], flip[1])
            assert same_bits(target, x) and target.stride() == VOL.as_device_volume(vol).stride(), (order, flip)


def test_restore_through_the_table_gives_the_mscmrseg_codes(dev):
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd.utils import volume as VOL
    pred = label_values((7, 38, 45), np.uint8, 700, codes=(0, 1, 2, 3))           # [Z,Y,X]
    codes = np.array([0, 200, 500, 600], np.int16)
    got = EM.restore_prediction(torch.from_numpy(pred).to(dev), (45, 38, 7))
    assert got.dtype == torch.int16 and tuple(got.shape) == (45, 38, 7) and got.permute(2, 1, 0).is_contiguous()
    assert same_bits(got, codes[pred].T)
    assert same_bits(EM.read_labels(got), codes[pred].astype(np.int32)), "read_labels is its inverse orientation"
    lut = np.arange(256); lut[1:4] = (200, 500, 600)
    for fortran in (True, False):
        again = VOL.restore_volume(torch.from_numpy(pred).to(dev), (45, 38, 7), flip=(False, False), transpose=True, lut=lut,
                                   dtype=torch.int16, fortran=fortran)
        assert same_bits(again, codes[pred].T)
    # with the MM-WHS orientation, and into uint8 (the table's values cast)
    small = np.arange(256) % 7
    p2 = label_values((5, 33, 47), np.uint8, 701)
    back = VOL.restore_volume(torch.from_numpy(p2).to(dev), (33, 47, 5), lut=small, dtype=torch.uint8)
    assert same_bits(VOL.volume_labels(back, num_classes=7), small[p2].astype(np.uint8))


# ---------------------------------------------------------------------------------------------- no synchronisation
def test_nothing_synchronises_and_two_calls_agree(dev):
    """every function with check=False under torch.cuda.set_sync_debug_mode("error"); the mode is first shown to be enforced (a
    ``.item()`` raises under it); inputs are device tensors (an upload from pageable host memory makes the host wait)"""
    from pointcloududa_amd import evaluate_mmwhs as EW
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd.utils import volume as VOL
    img = VOL.as_device_volume(np.asfortranarray(values((40, 24, 70), np.int16, 800)))
    mask = VOL.as_device_volume(np.asfortranarray(label_values((40, 24, 70), np.float64, 801)))
    codes = VOL.as_device_volume(np.asfortranarray(label_values((40, 24, 70), np.int16, 802, codes=(0, 200, 500, 600))))
    pred = torch.from_numpy(label_values((70, 24, 40), np.uint8, 803, codes=(0, 1, 2, 3))).to(dev)
    lut = torch.arange(256, dtype=torch.int16, device=dev)

    def run():
        x, gt = EW.read_volume(img, mask, check=False)
        lab, hot = VOL.volume_labels(mask, onehot=True, check=False, remap=((4, 3),))
        return (x, gt, lab, hot, VOL.volume_slices(img, window=1), VOL.volume_labels(codes, raw=True), EM.read_labels(codes),
                VOL.restore_volume(gt, (40, 24, 70)), VOL.restore_volume(gt, (40, 24, 70), lut=lut, dtype=torch.int16, fortran=False),
                EM.restore_prediction(pred, (40, 24, 70)))

    want = run()                                                          # (warm: allocator, library load, the code table)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        got = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(got) == len(want) == 10
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert same_bits(got[0], expect_slices(img.cpu().numpy(), 2, (True, True), 3))


# ---------------------------------------------------------------------------------------------- end to end
SIDE = 96      # the smallest side the segmenter's point head accepts: (96 / 16 - 5)^2 = 1 = fc_inch (32 x 32 leaves it no map)


def _patient(seed, depth, absent=None):
    """a [H,W,D] float64 image and a float64 mask (label files come back as floating point) holding every class but `absent`,
    both Fortran-ordered as a NIfTI reader returns them"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    mask = np.zeros((SIDE, SIDE, depth))
    for k, (cy, cx, rad) in enumerate(((24, 24, 13), (24, 70, 12), (70, 24, 14), (68, 68, 11)), start=1):
        if k == absent:
            continue
        for d in range(depth):
            mask[..., d][(yy - cy - d) ** 2 + (xx - cx + d) ** 2 <= (rad - d % 3) ** 2] = k
    img = mask * 90.0 + rng.standard_normal(mask.shape) * 25.0
    return np.asfortranarray(img), np.asfortranarray(mask)


@pytest.fixture(scope="module")
def end_to_end(dev):
    from pointcloududa_amd import evaluate_mmwhs as EW
    from pointcloududa_amd import validate as V
    from pointcloududa_amd.networks import Segmentation_model_Point
    torch.manual_seed(5)
    model = Segmentation_model_Point(filters=4, in_channels=3, n_class=5, pointnet=True, fc_inch=1).to(dev).eval()
    patients = [(1003, ) + _patient(900, 5), (1008, ) + _patient(901, 7), (1014, ) + _patient(902, 6, absent=4)]
    out = EW.evaluate_segmentation(model, patients, bs=4, model_name="d1d2d4", toprint=False)
    host = {}
    for pat_id, img, mask in patients:
        x, gt = expect_slices(img, 2, (True, True), 3), expect_labels(mask, 2, (True, True), 5, ())[0]
        host[pat_id] = V.evaluate_volume(model, x, gt, bs=4, klc=True, ifhd=True, ifasd=True, variant="mmwhs")
    return model, patients, out, host


def test_evaluate_segmentation_equals_evaluate_volume_on_the_numpy_restated_inputs(dev, end_to_end):
    model, patients, out, host = end_to_end
    assert list(out["per_patient"]) == [1003, 1008, 1014]
    for pat_id, img, mask in patients:
        assert sorted(np.unique(mask).tolist()) == ([0, 1, 2, 3, 4] if pat_id != 1014 else [0, 1, 2, 3])
        res = out["per_patient"][pat_id]
        assert len(res) == 12 and res == host[pat_id], (pat_id, res, host[pat_id])
    for row, (pat_id, _, _) in zip(out["rows"], patients):
        res = host[pat_id]
        assert row == [float(np.mean([res[n], res[3 + n], res[6 + n], res[9 + n]])) for n in range(3)] + ["d1d2d4", pat_id]


def test_the_table_is_numpys_on_those_lists_and_an_absent_class_drops_out(dev, end_to_end):
    import warnings
    model, patients, out, host = end_to_end
    third = host[1014]
    assert third[10] == -1 and third[11] == -1 and third[9] == 0.0, "class 4 (AA) is absent from the third ground truth"
    lists = list(host.values())
    at = {"LVmyo": 0, "LAblood": 3, "LVblood": 6, "AA": 9}
    for n, metric in enumerate(("DC", "HD", "ASD")):
        for name, first in at.items():
            vals = [r[first + n] for r in lists if n == 0 or r[first + n] != -1]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = (np.around(np.mean(np.array(vals)), 3), np.around(np.std(np.array(vals)), 3))
            got = out["table"][metric][name]
            assert np.array_equal(np.array(got), np.array(want), equal_nan=True), (metric, name, got, want)
        means = [out["table"][metric][k][0] for k in ("AA", "LAblood", "LVblood", "LVmyo")]
        stds = [out["table"][metric][k][1] for k in ("AA", "LAblood", "LVblood", "LVmyo")]
        ave = out["table"]["Ave"][metric]
        assert np.array_equal(np.array(ave), np.array([sum(means) / 4., sum(stds) / 4.]), equal_nan=True)
    aa_hd = [r[10] for r in lists if r[10] != -1]
    assert len(aa_hd) <= 2, "the third patient is not in AA's HD list"
    assert len([r[9] for r in lists]) == 3, "but it is in AA's Dice list"


def test_extended_lists_and_the_reader_with_check(dev, end_to_end):
    from pointcloududa_amd import evaluate_mmwhs as EW
    from pointcloududa_amd import validate as V
    model, patients, out, host = end_to_end
    ext = EW.evaluate_segmentation(model, patients[:1], bs=4, extended=True, toprint=False)
    pat_id, img, mask = patients[0]
    x, gt = EW.read_volume(img, mask)
    assert same_bits(x, expect_slices(img, 2, (True, True), 3)) and same_bits(gt, expect_labels(mask, 2, (True, True), 5, ())[0])
    want = V.evaluate_volume(model, x, gt, bs=4, variant="mmwhs", extended=True)
    assert len(want) == 20 and ext["per_patient"][pat_id] == want
    assert [want[5 * k + n] for k in range(4) for n in range(3)] == host[pat_id], "the first three of each five are the default's bits"
    bad = mask.copy(order="F")
    bad[3, 4, 1] = 6.0
    with pytest.raises(ValueError, match="1 values"):
        EW.read_volume(img, bad)
    with pytest.raises(ValueError, match="patient 77: 1 values"):
        EW.evaluate_segmentation(model, [(77, img, bad)], toprint=False)


def test_the_patient_loop_does_not_synchronise_before_its_end(dev, end_to_end):
    from pointcloududa_amd import evaluate_mmwhs as EW
    from pointcloududa_amd import validate as V
    from pointcloududa_amd.utils import volume as VOL
    model, patients, out, host = end_to_end
    img, mask = VOL.as_device_volume(patients[0][1]), VOL.as_device_volume(patients[0][2])
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        x, gt, counter = EW._read_volume(img, mask)
        rows = V.evaluate_volume_rows(model, x, gt, bs=4, klc=True, variant="mmwhs")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert EW.metrics_from_rows(rows.tolist(), True, True) == host[patients[0][0]] and counter.tolist() == [0]
