"""The case table of the Fourier adaptation edge tests (tests/test_fourier_edges.py, tests/test_fourier_edges_gpu.py): plain
data, seeded input builders and their float64 references (tests/fourier_refs.py), numpy only; nothing here touches a device.

fourier_refs.CASES stops at W = 256, which is exactly one column chunk of ``fourier_spectrum_kernel``, has H <= W everywhere, is
drawn as uint8 throughout and keeps ``|S| >= 1`` on every bin.  Every case below is the smallest shape that first reaches one of
the paths csrc/fourier.hip takes beyond that (``plan`` restates its ``make_plan``; test_fourier_edges.py asserts each claim):

  0  (1, 3, 257, 1, 1)      a second chunk of ONE column; g = 3, seg = 42: 41 of the 42 segments are empty in it
  1  (2, 5, 300, 2, 2)      g = 5, seg = 17; a second chunk of 44 columns, len = 3, two empty segments; C = 2
  2  (1, 40, 513, 3, 9)     three chunks, the last of one column; seg = 1; two spectrum bands, the second ragged; three apply
                            bands; C = 3
  3  (1, 130, 70, 4, 7)     tall; C = 4; five spectrum bands, the last of 2 rows
  4  (1, 3, 4096, 1, 1)     the side limit on W: 16 full chunks, a 64 KiB twiddle table
  5  (1, 4096, 3, 1, 1)     the side limit on H: 128 spectrum bands, 256 apply bands, seg capped by W = 3
  6  (1, 67, 1000, 1, 32)   the radius limit over four chunks (the last of 232); g = 7; bands of 28 rows, the last band one full
                            group and 4 rows
  7  (1, 65, 259, 1, 32)    the full-height block (2 b + 1 == H) with a 3-column last chunk

Case i draws from ``default_rng(2000 + i)``, in this order: the uint8 source ``[B,H,W,C]``, a uint8 bank of R = B + 1 references,
then the fp32 families: the ``ct`` source ``(normal(0, 1) * 1000).astype(float32)`` and its references, the ``unit`` source
``random(dtype=float32)`` and its references.  ``index[k] = B - k``: the LAST references, out of order, with R > B.  The zero-plane
case Z is (1, 33, 300, 3, 4) from ``default_rng(5)`` with source channel 1 all zero (and a variant whose whole sample is zero);
the degenerate planes (a constant, equal rows, equal columns) share its shape and references."""
import numpy as np

import fourier_refs as R

CASES = ((1, 3, 257, 1, 1), (2, 5, 300, 2, 2), (1, 40, 513, 3, 9), (1, 130, 70, 4, 7), (1, 3, 4096, 1, 1), (1, 4096, 3, 1, 1),
         (1, 67, 1000, 1, 32), (1, 65, 259, 1, 32))
ZERO_CASE = (1, 33, 300, 3, 4)
FAMILIES = ("u8", "ct", "unit")        # "u8": the uint8 draws (as they are, or their values as fp32); the other two are fp32 only
RADII_CASE, RADII_BATCH, RADII_INDEX, RADII = 2, 3, (3, -1, 0), (0, 4, 40)    # case 2 with B raised to 3

# the fp32 bound is |out - ref| <= 2^-24 |ref| + additive(M): test_fourier_adapt_gpu.py's bound with its 1e-9, sized for values
# up to 255, scaled to the largest input magnitude M.  MARGIN is the factor that module keeps between the agreement of two
# float64 algorithms and that term (1e-9 against 1.8e-12)
MARGIN = 500.0
# the largest difference between |fft2(t)| and |E_y t E_x^T| over the half block, relative to M H W, over every case and family
# (test_fourier_edges.py measures 1.15e-16, at the DC bin of the all-positive ``unit`` case 2, and asserts this constant: two
# float64 roundings of a value of up to M H W); MARGIN times it is the bank tolerance of the GPU test
BANK_REL = 2e-16

# chunk, group and band sizes of csrc/fourier.hip
K_THREADS, K_CHUNK, K_MAX_GROUP, K_BAND_ROWS, K_APPLY_ROWS, K_MAX_SIDE, K_MAX_RADIUS = 256, 256, 16, 32, 16, 4096, 32

_CACHE = {}


def plan(h, w, b):
    """``make_plan`` of csrc/fourier.hip restated: g rows per group, seg column segments per row, band rows per workgroup and
    nbands of the spectrum pass, the bands of the apply pass, the column chunks"""
    nb = b + 1
    g = max(1, min(K_THREADS // nb, K_MAX_GROUP, h))
    seg = max(1, min(K_THREADS // (g * nb), min(w, K_CHUNK)))
    gp = max(1, K_BAND_ROWS // g)
    band = g * gp
    chunks = [min(K_CHUNK, w - c0) for c0 in range(0, w, K_CHUNK)]
    return dict(g=g, seg=seg, gp=gp, band=band, nbands=-(-h // band), apply_bands=-(-h // K_APPLY_ROWS), chunks=chunks)


def chunk_segments(cn, seg):
    """``(len, segments that hold a column)`` of a chunk of ``cn`` columns cut into ``seg`` segments"""
    length = -(-cn // seg)
    return length, sum(1 for s in range(seg) if s * length < cn)


def additive(m):
    """the additive term of the fp32 bound at the largest input magnitude ``m``: 1e-9 at 255"""
    return 1e-9 * float(m) / 255.0


def magnitude(src, refs):
    """the largest magnitude in source and references"""
    return float(max(np.abs(np.asarray(src, np.float64)).max(), np.abs(np.asarray(refs, np.float64)).max()))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def case_index(i):
    """``index[k] = B - k``"""
    b = CASES[i][0]
    return np.array([b - k for k in range(b)], dtype=np.int64)


def case_inputs(i, batch=None):
    """``{family: (source, references)}`` of case ``i`` (``batch`` replaces its B): "u8" uint8, "ct" and "unit" float32; computed
    once per process and never written"""
    key = ("in", i, batch)
    if key not in _CACHE:
        b, h, w, c, _ = CASES[i]
        b = b if batch is None else batch
        s, r = (b, h, w, c), (b + 1, h, w, c)
        rng = np.random.default_rng(2000 + i)
        u8 = _frozen(rng.integers(0, 256, s, dtype=np.uint8), rng.integers(0, 256, r, dtype=np.uint8))
        ct = _frozen((rng.normal(0, 1, s) * 1000).astype(np.float32), (rng.normal(0, 1, r) * 1000).astype(np.float32))
        unit = _frozen(rng.random(s, dtype=np.float32), rng.random(r, dtype=np.float32))
        _CACHE[key] = {"u8": u8, "ct": ct, "unit": unit}
    return _CACHE[key]


def case_reference(i, family, fn=R.adapt_plane_fft):
    """``(source, references, index, float64 reference)`` of case ``i`` and a family; computed once per process"""
    key = ("ref", i, family, fn.__name__)
    if key not in _CACHE:
        src, refs = case_inputs(i)[family]
        idx = case_index(i)
        _CACHE[key] = (src, refs, idx) + _frozen(R.adapt_batch(src, refs, CASES[i][4], idx, fn=fn))
    return _CACHE[key]


def radii_reference(fn=R.adapt_plane_fft):
    """``(source, references, float64 reference)`` of case 2 at B = 3 under RADII_INDEX and RADII (uint8 draws)"""
    key = ("radii", fn.__name__)
    if key not in _CACHE:
        src, refs = case_inputs(RADII_CASE, RADII_BATCH)["u8"]
        _CACHE[key] = (src, refs) + _frozen(R.adapt_batch(src, refs, CASES[RADII_CASE][4], RADII_INDEX, RADII, fn=fn))
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------- zero and degenerate planes
def zero_inputs(whole=False):
    """``(source, references)`` uint8 of Z: source channels 0 and 2 drawn, channel 1 all zero; ``whole``: the sample all zero"""
    key = ("zero", bool(whole))
    if key not in _CACHE:
        b, h, w, c, _ = ZERO_CASE
        rng = np.random.default_rng(5)
        src = np.zeros((b, h, w, c), dtype=np.uint8)
        src[..., 0] = rng.integers(0, 256, (b, h, w))
        src[..., 2] = rng.integers(0, 256, (b, h, w))
        refs = rng.integers(0, 256, (1, h, w, c), dtype=np.uint8)
        if whole:
            src[:] = 0
        _CACHE[key] = _frozen(src, refs)
    return _CACHE[key]


def zero_reference(whole=False, fn=R.adapt_plane_fft):
    """``(source, references, float64 reference)`` of Z against its one reference"""
    key = ("zeroref", bool(whole), fn.__name__)
    if key not in _CACHE:
        src, refs = zero_inputs(whole)
        _CACHE[key] = (src, refs) + _frozen(R.adapt_batch(src, refs, ZERO_CASE[4], [0], fn=fn))
    return _CACHE[key]


def block_mask(h, w, b):
    """1.0 on the block's bins of an ``[H,W]`` spectrum in numpy's FFT order, 0.0 elsewhere"""
    keep = np.zeros((h, w))
    keep[np.ix_(R.block_index(h, b), R.block_index(w, b))] = 1.0
    return keep


def zero_plane_closed_form(t, b):
    """what an all-zero source plane becomes: phase 0 on every bin, so the inverse transform of ``|T|`` on the block"""
    t = np.asarray(t, np.float64)
    return np.real(np.fft.ifft2(np.abs(np.fft.fft2(t)) * block_mask(t.shape[0], t.shape[1], b)))


def degenerate_inputs():
    """``(source, references)`` float32 at Z's shape: plane 0 the constant 7, plane 1 with all rows equal, plane 2 with all
    columns equal (``default_rng(7)``: the row, then the column); Z's references as fp32"""
    if "degenerate" not in _CACHE:
        b, h, w, c, _ = ZERO_CASE
        rng = np.random.default_rng(7)
        src = np.empty((b, h, w, c), dtype=np.float32)
        src[..., 0] = 7.0
        src[..., 1] = rng.integers(0, 256, w)[None, None, :]
        src[..., 2] = rng.integers(0, 256, h)[None, :, None]
        _CACHE["degenerate"] = _frozen(src, zero_inputs()[1].astype(np.float32))
    return _CACHE["degenerate"]


# ---------------------------------------------------------------------------------------------- the bank
def bank_fft(refs, b):
    """``|fft2(t)|`` at ``block_index(H, b)`` x ``0..b`` of every plane: float64 ``[R, C, 2b+1, b+1]``, the layout of
    ``FourierBank.bank``"""
    refs = np.asarray(refs, np.float64)
    T = np.abs(np.fft.fft2(refs, axes=(1, 2)))
    return np.ascontiguousarray(T[:, R.block_index(refs.shape[1], b)][:, :, :b + 1].transpose(0, 3, 1, 2))


def bank_dft(refs, b):
    """the same amplitudes from the explicit DFT matrices of ``fourier_refs.adapt_plane_lowrank``"""
    refs = np.asarray(refs, np.float64)
    _, h, w, _ = refs.shape
    ky, kx = np.arange(-b, b + 1), np.arange(0, b + 1)
    ey = np.exp(-2j * np.pi * ((ky[:, None] * np.arange(h)[None, :]) % h) / h)       # [2b+1, H]
    ex = np.exp(-2j * np.pi * ((kx[:, None] * np.arange(w)[None, :]) % w) / w)       # [b+1, W]
    return np.abs(ey @ refs.transpose(0, 3, 1, 2) @ ex.T)


def bank_tolerance(refs):
    """the absolute tolerance of a device bank against ``bank_fft``: MARGIN BANK_REL M H W"""
    refs = np.asarray(refs)
    return MARGIN * BANK_REL * float(np.abs(refs.astype(np.float64)).max()) * refs.shape[1] * refs.shape[2]
