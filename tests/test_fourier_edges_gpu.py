"""GPU checks of Fourier domain adaptation past the shapes of fourier_refs.CASES (pointcloududa_amd/utils/fourier.py,
csrc/fourier.hip) against the full-FFT definition in numpy float64: the table of
tests/fourier_edge_cases.py -- rows of more than one 256-column chunk, tall images, 4096 on either side, radius 32 over several
chunks, a bank larger than the batch read from its end -- with fp32 inputs that are no integers in 0..255, planes that are
all zero (the ``amp == 0`` branch of ``fourier_delta_kernel``) and planes that are constant along an axis.

Tolerances, each from the references alone (tests/test_fourier_edges.py asserts and prints what they rest on):

fp32: ``|out - ref| <= 2^-24 |ref| + a`` on every pixel, ``a = 1e-9 M / 255`` with M the largest magnitude in source and
  references.  One float32 rounding of a float64 value (half an ulp) plus test_fourier_adapt_gpu.py's additive term scaled to
  the inputs: 1e-9 for the uint8 values, 1.4e-8 to 1.9e-8 for ``ct`` (normal * 1000), 3.9e-12 for ``unit`` ([0, 1)).  ``a`` is at
  least 500 times what the two float64 restatements differ by on these inputs: measured 5.1e-13 (uint8 values), 2.3e-12
  (``ct``), 2.3e-15 (``unit``), asserted ``<= a / 500``.  The phases are well defined: the smallest block ``|S|`` is 936 for ``ct``
  (floor 100) and 0.92 for ``unit`` (floor 0.5).
uint8: equal to ``uint8(clip(rint(ref), 0, 255))`` on EVERY pixel.  No reference value lies within 1e-8 of a half-integer
  (smallest distance 7.4e-6 at case 3, 1.5e-5 for Z, 3.0e-6 for case 2 at B = 3 under per-sample radii), every block bin of a
  non-zero source plane has ``|S| >= 1`` (smallest 240 at case 7; 90 under the per-sample radii), and every case's reference
  leaves 0..255 (case 7 spans -62 to 334), so the saturating store acts.
bank: ``|bank - |fft2(t)|| <= 500 * 2e-16 * M H W``.  2e-16 bounds what ``|fft2(t)|`` and the explicit DFT matrices differ by
  over the half block relative to M H W (measured 1.15e-16, at a DC bin: two float64 roundings of a value of up to M H W); 500 is
  the same margin as above.  ``fourier_edge_cases.bank_tolerance`` derives it from the constant the CPU test asserts.
zero planes: the bounds above, against the definition AND against the closed form ``real(ifft2(|T| on the block))`` (phase 0);
  the two agree exactly in float64 here, and the closed form is at least 8.9e-5 from a tie.
degenerate planes (constant, equal rows, equal columns): noise bins have an arbitrary phase in numpy and here alike, so nothing is
  compared pixel for pixel and the block's amplitudes are not asserted; the output is finite, two runs give the same bits, and
  the bins OUTSIDE the block of ``fft2(out)`` equal the source's within ``H W (2^-24 max|out| + a)``, the per-pixel bound summed
  over the pixels (about 0.1; the numpy references rounded to float32 are 1e-3 away).

Measured on an MI355X with these tolerances (every test prints its figures): fp32, the largest ``|out - ref| - bound`` lies
between ``-a`` and ``-20 a`` in every case and family (-1.0e-9 on the uint8 values, -1.8e-8 on ``ct``, -4.0e-12 on ``unit``), so the
additive term is not drawn on; the bank lies 8e-12 to 1.6e-9 from ``|fft2(t)|`` against tolerances of 2e-8 to 3e-5 (at most
1e-3 of the tolerance); degenerate planes 1.0e-3 to 1.2e-3 against bounds of 0.089 to 0.16."""
import numpy as np
import pytest
import torch

import fourier_edge_cases as T
import fourier_refs as R

pytestmark = pytest.mark.gpu

IDS = ["%d-%s" % (i, "x".join(str(v) for v in cs)) for i, cs in enumerate(T.CASES)]


def _F():
    from pointcloududa_amd.utils import fourier as F
    return F


def _same(got, want, what):
    got, want = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (got, want))
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = (a.view(np.uint32) if a.dtype == np.float32 else a for a in (got, want))
    bad = g != w
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _within_f32(got, ref, add, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref)
    excess = err - (2.0 ** -24 * np.abs(ref) + add)
    print("%s: a = %.3g, max (|out - ref| - bound) = %.3g, max |out - ref| = %.3g" % (what, add, excess.max(), err.max()))
    assert np.isfinite(got).all() and excess.max() <= 0.0, (what, int((excess > 0).sum()), float(excess.max()))


def _device_bank(bank):
    """``FourierBank.bank`` as float64 ``[R, C, 2b+1, b+1]``"""
    r, _, _, c = bank.shape
    b = bank.radius
    n = r * c * (2 * b + 1) * (b + 1)
    return bank.bank.cpu().numpy()[:8 * n].view(np.float64).reshape(r, c, 2 * b + 1, b + 1)


@pytest.mark.parametrize("i", range(len(T.CASES)), ids=IDS)
def test_uint8_equals_the_rounded_definition_on_every_pixel(dev, i):
    F = _F()
    src, refs, idx, ref = T.case_reference(i, "u8")
    b = T.CASES[i][4]
    tie, amp = float(np.abs(ref - np.floor(ref) - 0.5).min()), R.block_min_amplitude(src, b)
    print("case %d: smallest tie distance %.3g, smallest |S| %.4g" % (i, tie, amp))
    assert tie >= 1e-8 and amp >= 1.0, "the reference alone decides every pixel"
    x = torch.from_numpy(src).to(dev)
    bank = F.FourierBank(refs, dev, radius=b)
    assert (bank.size, bank.radius, bank.shape) == (src.shape[0] + 1, b, refs.shape)
    out = F.fourier_adapt(x, bank, index=idx)
    _same(out, R.to_u8(ref), "case %d %r" % (i, T.CASES[i]))
    _same(F.fourier_adapt(x, bank, index=idx), out, "two runs")
    _same(x, src, "the input is never written")


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("i", range(len(T.CASES)), ids=IDS)
def test_fp32_within_one_rounding_of_the_full_fft_definition(dev, i, family):
    F = _F()
    src, refs, idx, ref = T.case_reference(i, family)
    src, refs = src.astype(np.float32), refs.astype(np.float32)
    add = T.additive(T.magnitude(src, refs))
    assert family != "u8" or add == 1e-9
    x = torch.from_numpy(src).to(dev)
    bank = F.FourierBank(refs, dev, radius=T.CASES[i][4])
    out = F.fourier_adapt(x, bank, index=idx)
    _within_f32(out, ref, add, "%s case %d %r" % (family, i, T.CASES[i]))
    _same(F.fourier_adapt(x, bank, index=idx), out, "two runs")
    _same(x, src, "the input is never written")


@pytest.mark.parametrize("family", ("u8", "ct"))
@pytest.mark.parametrize("i", range(len(T.CASES)), ids=IDS)
def test_the_bank_holds_the_amplitudes_of_numpys_fft2(dev, i, family):
    F = _F()
    refs = T.case_inputs(i)[family][1]
    b = T.CASES[i][4]
    got = _device_bank(F.FourierBank(refs, dev, radius=b))
    want, tol = T.bank_fft(refs, b), T.bank_tolerance(refs)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print("%s case %d %r: max |bank - |fft2(t)|| = %.3g, tolerance %.3g, largest amplitude %.4g" % (family, i, T.CASES[i], err, tol, want.max()))
    assert np.isfinite(got).all() and err <= tol


@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("f32", "u8"))
@pytest.mark.parametrize("whole", (False, True), ids=("plane", "sample"))
def test_zero_planes_take_the_targets_amplitudes_at_phase_zero(dev, whole, dtype):
    F = _F()
    src, refs, ref = T.zero_reference(whole)
    b, add = T.ZERO_CASE[4], T.additive(255.0)
    assert not src[..., 1].any() and (whole or (src[..., 0].any() and src[..., 2].any()))
    x = torch.from_numpy(src.astype(dtype)).to(dev)
    bank = F.FourierBank(refs.astype(dtype), dev, radius=b)
    out = F.fourier_adapt(x, bank, index=[0])
    zero_planes = (0, 1, 2) if whole else (1,)
    closed = np.stack([T.zero_plane_closed_form(refs[0, ..., ch], b) for ch in zero_planes], axis=-1)[None]
    assert closed.min() > 1.0, "a zero result would not pass for it"
    if dtype == np.uint8:
        _same(out, R.to_u8(ref), "Z against the definition")
        _same(out[..., list(zero_planes)], R.to_u8(closed), "the zero planes against the inverse transform of |T| on the block")
    else:
        _within_f32(out, ref, add, "Z against the definition")
        _within_f32(out[..., list(zero_planes)], closed, add, "the zero planes against the inverse transform of |T| on the block")
    _same(F.fourier_adapt(x, bank, index=[0]), out, "two runs")
    _same(x, src.astype(dtype), "the input is never written")
    if whole:
        _same(F.fourier_adapt(x, bank, index=[-1]), np.zeros(src.shape, dtype), "a zero sample passed through stays zero")


def test_degenerate_planes_stay_finite_repeatable_and_untouched_outside_the_block(dev):
    F = _F()
    src, refs = T.degenerate_inputs()
    _, h, w, c, b = T.ZERO_CASE
    add = T.additive(T.magnitude(src, refs))
    x = torch.from_numpy(src).to(dev)
    bank = F.FourierBank(refs, dev, radius=b)
    out = F.fourier_adapt(x, bank, index=[0])
    _same(F.fourier_adapt(x, bank, index=[0]), out, "two runs")
    _same(x, src, "the input is never written")
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    outside = T.block_mask(h, w, b) == 0.0
    for ch, name in enumerate(("constant", "equal rows", "equal columns")):
        diff = float(np.abs(np.fft.fft2(got[0, ..., ch]) - np.fft.fft2(src[0, ..., ch].astype(np.float64)))[outside].max())
        bound = h * w * (2.0 ** -24 * float(np.abs(got[0, ..., ch]).max()) + add)
        print("%s: max |fft2(out) - fft2(src)| outside the block = %.3g, bound %.3g, out spans %.4g .. %.4g"
              % (name, diff, bound, got[0, ..., ch].min(), got[0, ..., ch].max()))
        assert diff <= bound, name


@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("f32", "u8"))
def test_per_sample_radii_and_pass_through_over_three_chunks(dev, dtype):
    """case 2 at B = 3: the ``ref_index < 0`` return of the spectrum pass and the radius mask of the delta pass on a plan with
    ``c0 > 0`` and two bands"""
    F = _F()
    src, refs, ref = T.radii_reference()
    b = T.CASES[T.RADII_CASE][4]
    assert src.shape == (3, 40, 513, 3) and refs.shape[0] == 4 and T.RADII_INDEX == (3, -1, 0) and T.RADII == (0, 4, 40)
    x = torch.from_numpy(src.astype(dtype)).to(dev)
    bank = F.FourierBank(refs.astype(dtype), dev, radius=b)
    out = F.fourier_adapt(x, bank, index=list(T.RADII_INDEX), radius=list(T.RADII))
    _same(out[1], x[1], "index -1 passes the sample through")
    if dtype == np.uint8:
        _same(out, R.to_u8(ref), "index %r, radii %r" % (T.RADII_INDEX, T.RADII))
    else:
        _within_f32(out, ref, T.additive(255.0), "index %r, radii %r" % (T.RADII_INDEX, T.RADII))
    _same(F.fourier_adapt(x, bank, index=list(T.RADII_INDEX), radius=list(T.RADII)), out, "two runs")
    _same(x, src.astype(dtype), "the input is never written")
