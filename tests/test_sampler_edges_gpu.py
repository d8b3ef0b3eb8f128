"""sampler.hip away from the 256 x 256 masks of tests/test_sampler_gpu.py: exact equality with oracle/sampler.py (numpy).

surface_vertices (one workgroup per mask, thread t owns rows t, t + 256, ...), "lex" and "mc" order:
  (40, 300), (300, 40)   non-square both ways: a swapped h / w shows
  (257, 64)              row 256 is thread 0's second row (mc: 512 cell rows, two trips for every thread)
  (513, 8)               three trips for thread 0 (mc: 1024 cell rows)
  (2, 2)                 one cell
  (1, 1), (1, 64), (64, 1)   lex only: no row / column neighbours; "mc" needs two rows and raises
  per shape: three different random masks, then all foreground (count 0), all background, foreground along the four
  borders, a checkerboard, one foreground pixel
  truncation through the C ABI: max_verts inside the first plane of the list and inside the second; the buffer behind
  max_verts rows keeps its sentinel, the count is the full one
fps (one workgroup per cloud, the running distances in dynamic LDS):
  npts_max 500 -> 4097 -> 19200 -> 500   across the opt-in to more than 32 KB of dynamic LDS (npts_max > 4096) and back;
                                         19200 is the limit, 19201 raises
  n = 1 with k = 300; all points identical; k = 1; first = -1, -n-1, >= n (the oracle gets first % n); counts far below
  npts_max; an integer lattice with symmetric ties; integer and real (normal) coordinates
masks_to_pointclouds: non-square masks; foreground area 50 -> zeros, 51 -> sampled; a checkerboard overflows the default
  max_verts and raises"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(40, 300), (300, 40), (257, 64), (513, 8), (2, 2)]
LEX_ONLY = [(1, 1), (1, 64), (64, 1)]
PAD = 1e6            # coordinates behind a cloud's count: far away, so a kernel that read them would pick them


def _random_masks(rng, h, w):
    """three different masks: an ellipse plus a bar on the left border, salt and pepper, a half plane with holes"""
    yy, xx = np.mgrid[0:h, 0:w]
    a = (((yy - 0.45 * h) / (0.3 * h + 1)) ** 2 + ((xx - 0.55 * w) / (0.35 * w + 1)) ** 2 < 1).astype(np.uint8) * 2
    a[:, 0:max(1, w // 16)] = 255
    b = (rng.random((h, w)) > 0.7).astype(np.uint8)
    c = ((yy >= h // 2) & (rng.random((h, w)) > 0.1)).astype(np.uint8) * 7
    return np.stack([a, b, c])


def _content_masks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    border = np.zeros((h, w), np.uint8)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = 1
    one = np.zeros((h, w), np.uint8)
    one[h // 2, w // 2] = 200
    return np.stack([np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8), border, ((yy + xx) % 2).astype(np.uint8), one])


def _oracle(order):
    from oracle import sampler as OS
    return OS.surface_vertices if order == "lex" else OS.surface_vertices_mc


def _check_batch(dev, masks, order):
    from pointcloududa_amd import kernels as K
    n, h, w = masks.shape
    max_verts = 12 * h * w + 1               # a pixel has 4 neighbours, the list 3 planes: nothing is cut
    verts, counts = K.surface_vertices(torch.from_numpy(masks).to(dev), max_verts, order)
    verts, counts = verts.cpu().numpy(), counts.cpu().numpy()
    for i in range(n):
        ref = _oracle(order)(masks[i])
        assert int(counts[i]) == len(ref), (i, int(counts[i]), len(ref))
        assert np.array_equal(verts[i, :len(ref)], ref), i
        assert not verts[i, len(ref):].any(), i               # nothing written behind the list
    return counts


@pytest.mark.parametrize("order", ["lex", "mc"])
@pytest.mark.parametrize("h,w", SHAPES + LEX_ONLY, ids=lambda v: str(v))
def test_surface_vertices_shapes_and_contents(dev, h, w, order):
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(h * 1000 + w)
    if order == "mc" and (h, w) in LEX_ONLY:      # the cell grid needs two rows and two columns
        with pytest.raises(RuntimeError, match="surface_vertices_mc: bad arguments"):
            K.surface_vertices(torch.zeros((1, h, w), dtype=torch.uint8, device=dev), 16, "mc")
        return
    _check_batch(dev, _random_masks(rng, h, w), order)
    counts = _check_batch(dev, _content_masks(h, w), order)
    assert counts[0] == 0 and counts[1] == 0                  # all foreground, all background: no surface
    if h * w > 1:
        assert counts[3] > 0 and counts[4] > 0


@pytest.mark.parametrize("plane", [0, 1])
@pytest.mark.parametrize("order", ["lex", "mc"])
def test_surface_vertices_truncation_keeps_the_rest_of_the_buffer(dev, order, plane):
    """"lex" lists the plane z = 0, then 1, then 2, a third of the list each.  "mc" lists the cells of slice 0, then those of
    slice 1; the slices are copies, so only in-plane edges cross, and a slice-0 cell owns the crossing edges of planes 0 and 1
    (two thirds of the list), a slice-1 cell those of plane 2."""
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    rng = np.random.default_rng(11)
    h, w = 257, 64
    masks = np.stack([(rng.random((h, w)) > 0.7), (rng.random((h, w)) > 0.68)]).astype(np.uint8)
    refs = [_oracle(order)(m) for m in masks]
    first = [len(r) // 3 * (1 if order == "lex" else 2) for r in refs]           # rows of the first plane / slice
    second_end = [len(r) // 3 * 2 if order == "lex" else len(r) for r in refs]
    max_verts = min(first) // 2 if plane == 0 else (max(first) + min(second_end)) // 2
    if plane == 0:
        assert 0 < max_verts < min(first)
    else:
        assert max(first) < max_verts < min(second_end)
    extra, sentinel = 64, -7
    buf = torch.full((2 * max_verts + extra, 3), sentinel, dtype=torch.int32, device=dev)
    counts = torch.full((2,), sentinel, dtype=torch.int32, device=dev)
    m = torch.from_numpy(masks).to(dev)
    lib = L.lib()
    if order == "lex":
        rc = lib.pcuda_surface_vertices(m.data_ptr(), 2, h, w, buf.data_ptr(), max_verts, counts.data_ptr(), None, 0, K._stream())
    else:
        rc = lib.pcuda_surface_vertices_mc(m.data_ptr(), 2, h, w, buf.data_ptr(), max_verts, counts.data_ptr(), K._stream())
    L.check(rc, "surface_vertices")
    got = buf.cpu().numpy()
    assert counts.cpu().tolist() == [len(r) for r in refs]
    for i in range(2):
        assert np.array_equal(got[i * max_verts:(i + 1) * max_verts], refs[i][:max_verts]), i
    assert (got[2 * max_verts:] == sentinel).all()


def _fps(dev, clouds, firsts, k, npts_max=None):
    """K.fps on a padded batch of [n_i, 3] clouds -> int array [B, k]"""
    from pointcloududa_amd import kernels as K
    npts_max = npts_max or max(len(c) for c in clouds)
    pts = np.full((len(clouds), npts_max, 3), PAD)
    for i, c in enumerate(clouds):
        pts[i, :len(c)] = c
    idx = K.fps(torch.from_numpy(pts).to(dev), torch.tensor([len(c) for c in clouds], dtype=torch.int32, device=dev),
                torch.tensor(firsts, dtype=torch.int32, device=dev), k)
    return idx.cpu().numpy()


def _fps_check(dev, clouds, firsts, k, npts_max=None):
    from oracle import sampler as OS
    got = _fps(dev, clouds, firsts, k, npts_max)
    for i, c in enumerate(clouds):
        assert np.array_equal(got[i], OS.fps_indices(c, k, firsts[i] % len(c))), i
    return got


def _clouds(rng, n, small):
    """an integer cloud (many ties), a real-valued one, and one far shorter than the batch's npts_max"""
    return [rng.integers(0, 50, (n, 3)).astype(np.float64), rng.standard_normal((n, 3)), rng.integers(0, 9, (small, 3)).astype(np.float64)]


def test_fps_across_the_lds_opt_in_and_back(dev):
    rng = np.random.default_rng(21)
    for npts_max, small in ((500, 3), (4097, 10), (19200, 7), (500, 3)):
        _fps_check(dev, _clouds(rng, npts_max, small), [npts_max - 1, 17, 2], 300)


def test_fps_above_the_limit_is_unsupported(dev):
    from pointcloududa_amd import kernels as K
    pts = torch.zeros((1, 19201, 3), dtype=torch.float64, device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    launches = K.launch_count()
    with pytest.raises(RuntimeError, match=r"\(-2\): fps: at most 19200 points per cloud"):      # PCUDA_E_UNSUPPORTED
        K.fps(pts, one, one, 4)
    assert K.launch_count() == launches


@pytest.mark.parametrize("real", [False, True], ids=["integer", "real"])
def test_fps_degenerate_clouds_and_first_index(dev, real):
    rng = np.random.default_rng(22 + real)
    draw = (lambda n: rng.standard_normal((n, 3))) if real else (lambda n: rng.integers(0, 20, (n, 3)).astype(np.float64))
    # one point, asked for 300: index 0 every time
    got = _fps_check(dev, [draw(1)], [0], 300)
    assert not got.any()
    # all points identical: the first index, then the first occurrence of the (zero) maximum
    got = _fps_check(dev, [np.repeat(draw(1), 100, 0)], [5], 300)
    assert got[0, 0] == 5 and not got[0, 1:].any()
    # k = 1: the first index alone
    assert _fps_check(dev, [draw(70), draw(300)], [69, 123], 1).tolist() == [[69], [123]]
    # first outside [0, n): taken modulo n, Python's (non-negative) modulo
    n = 700
    c = draw(n)
    got = _fps_check(dev, [c] * 5, [-1, -n - 1, n, 3 * n + 5, -2 * n], 40)
    assert got[:, 0].tolist() == [n - 1, n - 1, 0, 5, 0]
    # counts far below npts_max
    _fps_check(dev, [draw(2), draw(1), draw(33)], [1, 0, 40], 50, npts_max=5000)


def test_fps_lattice_with_symmetric_ties(dev):
    g = np.stack(np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), np.arange(-1, 2), indexing="ij"), -1).reshape(-1, 3)
    centre = int(np.flatnonzero((g == 0).all(1))[0])
    _fps_check(dev, [g.astype(np.float64), g[::-1].astype(np.float64), g.astype(np.float64)], [centre, centre, 0], 243)


@pytest.mark.parametrize("order", ["lex", "mc"])
def test_masks_to_pointclouds_non_square(dev, order):
    from oracle import sampler as OS
    from pointcloududa_amd.utils import npy2point as S
    rng = np.random.default_rng(31)
    for h, w in ((40, 300), (300, 40)):
        masks = _random_masks(rng, h, w)[[0, 2]]                  # (salt and pepper overflows the default max_verts)
        firsts = np.array([123456, -3], dtype=np.int32)
        out = S.masks_to_pointclouds(torch.from_numpy(masks).to(dev), torch.from_numpy(firsts).to(dev), order=order).cpu().numpy()
        for i in range(2):
            ref = OS.mask_to_pointcloud(masks[i], 300, first=int(firsts[i]), order=order)
            assert ref.any() and np.array_equal(out[i], ref), (h, w, i)


def test_masks_to_pointclouds_area_threshold(dev):
    from oracle import sampler as OS
    from pointcloududa_amd.utils import npy2point as S
    masks = np.zeros((2, 24, 40), np.uint8)
    masks[:, 3:8, 10:20] = 1                                      # 50 pixels: not sampled (npy2point.py:116 asks for > 50)
    masks[1, 8, 10] = 1                                           # 51
    out = S.masks_to_pointclouds(torch.from_numpy(masks).to(dev), torch.tensor([4, 4], dtype=torch.int32, device=dev)).cpu().numpy()
    assert masks[0].sum() == 50 and not out[0].any()
    ref = OS.mask_to_pointcloud(masks[1], 300, first=4)
    assert masks[1].sum() == 51 and ref.any() and np.array_equal(out[1], ref)
    assert not OS.mask_to_pointcloud(masks[0], 300, first=4).any()


def test_masks_to_pointclouds_overflow_raises(dev):
    from pointcloududa_amd.utils import npy2point as S
    yy, xx = np.mgrid[0:64, 0:64]
    m = torch.from_numpy(((yy + xx) % 2).astype(np.uint8)[None]).to(dev)     # 3 * 2048 vertices > 3 * 8 * (64 + 64)
    with pytest.raises(RuntimeError, match="surface has more than max_verts=3072 vertices"):
        S.masks_to_pointclouds(m, torch.zeros(1, dtype=torch.int32, device=dev))
