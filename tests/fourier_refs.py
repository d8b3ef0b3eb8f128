"""Two restatements, in numpy float64, of the Fourier domain adaptation rule of ``pointcloududa_amd/utils/fourier.py``
(``csrc/fourier.hip``): the full-FFT definition and the low-rank form with explicit DFT matrices that the kernels compute.  The
test modules share them; nothing here touches a device."""
import numpy as np

# (B, H, W, C, b): the smallest shapes that reach odd and unequal sizes, every channel count of the interleaved layout, a
# ragged last row band, widths that are no multiple of a wave or of four, the full-width block (2 b + 1 == min), the radius
# limit and the two workload sizes
CASES = ((1, 1, 1, 1, 0), (2, 3, 3, 1, 1), (2, 5, 7, 1, 1), (3, 17, 23, 2, 1), (2, 33, 64, 3, 2), (2, 70, 130, 4, 7),
         (2, 65, 65, 1, 32), (2, 224, 224, 1, 22), (2, 256, 256, 3, 2), (2, 256, 256, 3, 12))

_CACHE = {}


def case_inputs(i):
    """``(source, references)`` uint8 ``[B,H,W,C]`` of case ``i``: ``default_rng(1000 + i)``, the source drawn first"""
    b, h, w, c, _ = CASES[i]
    rng = np.random.default_rng(1000 + i)
    src = rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)
    refs = rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)
    return src, refs


def block_index(n, b):
    """the indices, in numpy's FFT order, of the frequencies -b..b of an axis of length n"""
    return np.arange(-b, b + 1) % n


def adapt_plane_fft(s, t, b):
    """the definition: ``s``, ``t`` real ``[H,W]``, radius ``b`` -> float64 ``[H,W]``"""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    h, w = s.shape
    assert t.shape == s.shape and b >= 0 and 2 * b + 1 <= min(h, w)
    S, T = np.fft.fft2(s), np.fft.fft2(t)
    Ss, Ts = np.fft.fftshift(S), np.fft.fftshift(T)
    y0, x0 = h // 2 - b, w // 2 - b
    blk = (slice(y0, y0 + 2 * b + 1), slice(x0, x0 + 2 * b + 1))
    Ss[blk] = np.abs(Ts[blk]) * np.exp(1j * np.angle(Ss[blk]))
    return np.real(np.fft.ifft2(np.fft.ifftshift(Ss)))


def adapt_plane_lowrank(s, t, b):
    """the form the kernels compute: ``v = s + real(E_y^H D E_x^H) / (H W)`` with explicit DFT matrices over the block's bins"""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    h, w = s.shape
    assert t.shape == s.shape and b >= 0 and 2 * b + 1 <= min(h, w)
    k = np.arange(-b, b + 1)
    ey = np.exp(-2j * np.pi * ((k[:, None] * np.arange(h)[None, :]) % h) / h)       # [2b+1, H]
    ex = np.exp(-2j * np.pi * ((k[:, None] * np.arange(w)[None, :]) % w) / w)       # [2b+1, W]
    S = ey @ s @ ex.T
    T = ey @ t @ ex.T
    aS, aT = np.abs(S), np.abs(T)
    safe = np.where(aS == 0.0, 1.0, aS)
    D = np.where(aS == 0.0, aT, (aT - aS) * S / safe)
    return s + np.real(ey.conj().T @ D @ ex.conj()) / (h * w)


def adapt_batch(src, refs, b, index=None, radius=None, fn=adapt_plane_fft):
    """``src [B,H,W,C]`` against ``refs [R,H,W,C]`` -> float64 ``[B,H,W,C]``; ``index[i] < 0`` keeps sample ``i``; ``radius``: per
    sample, clamped into ``[0, b]``"""
    src, refs = np.asarray(src), np.asarray(refs)
    n, _, _, c = src.shape
    index = np.arange(n) if index is None else np.asarray(index)
    out = src.astype(np.float64)
    for i in range(n):
        if index[i] < 0:
            continue
        ri = min(int(index[i]), refs.shape[0] - 1)
        bi = b if radius is None else min(max(int(radius[i]), 0), b)
        for ch in range(c):
            out[i, ..., ch] = fn(src[i, ..., ch], refs[ri, ..., ch], bi)
    return out


def case_reference(i):
    """``(source, references, full-FFT reference float64)`` of case ``i``, computed once per process and never written"""
    if i not in _CACHE:
        src, refs = case_inputs(i)
        ref = adapt_batch(src, refs, CASES[i][4])
        for a in (src, refs, ref):
            a.setflags(write=False)
        _CACHE[i] = (src, refs, ref)
    return _CACHE[i]


def to_u8(v):
    """the uint8 store: ``uint8(clip(rint(v), 0, 255))``, ``rint`` half to even"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def block_min_amplitude(src, b):
    """the smallest ``|S[k]|`` over the block bins of every plane of ``src [B,H,W,C]``"""
    src = np.asarray(src, np.float64)
    S = np.fft.fft2(src, axes=(1, 2))
    iy, ix = block_index(src.shape[1], b), block_index(src.shape[2], b)
    return float(np.abs(S[:, iy][:, :, ix]).min())
