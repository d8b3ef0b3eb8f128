"""CPU checks of the Fourier adaptation edge table (tests/fourier_edge_cases.py): the table reaches
the plans it names, and the conditions that tests/test_fourier_edges_gpu.py rests on hold on the numpy references alone -- no
uint8 reference near a tie, no vanishing block bin outside the planted zero planes, a saturating store that acts, the two
float64 restatements within a five-hundredth of the fp32 bound's additive term, the bank's amplitudes two ways.  Every measured
value is printed.  These are conditions, not measurements: if a generator change breaks one, another seed is the answer."""
import numpy as np
import pytest

import fourier_edge_cases as T
import fourier_refs as R

IDS = ["%d-%s" % (i, "x".join(str(v) for v in cs)) for i, cs in enumerate(T.CASES)]


def test_the_table_reaches_what_it_names():
    assert len(T.CASES) == 8 and T.ZERO_CASE == (1, 33, 300, 3, 4)
    for b, h, w, c, rad in T.CASES + (T.ZERO_CASE,):
        assert 1 <= c <= 4 and 2 * rad + 1 <= min(h, w) and rad <= T.K_MAX_RADIUS and max(h, w) <= T.K_MAX_SIDE
    p = [T.plan(h, w, rad) for _, h, w, _, rad in T.CASES]
    # 0: a second chunk of one column, 41 of 42 segments empty in it
    assert (p[0]["g"], p[0]["seg"], p[0]["chunks"]) == (3, 42, [256, 1]) and T.chunk_segments(1, 42) == (1, 1)
    # 1: a second chunk of 44 columns cut into segments of 3: two of the 17 are empty
    assert (p[1]["g"], p[1]["seg"], p[1]["chunks"]) == (5, 17, [256, 44]) and T.chunk_segments(44, 17) == (3, 15)
    # 2: three chunks, one segment, two spectrum bands (32 + 8 rows), three apply bands
    assert (p[2]["seg"], p[2]["chunks"], p[2]["band"], p[2]["nbands"], p[2]["apply_bands"]) == (1, [256, 256, 1], 32, 2, 3)
    # 3: tall, five bands, the last of 2 rows
    assert T.CASES[3][1] > T.CASES[3][2] and (p[3]["band"], p[3]["nbands"]) == (32, 5) and 130 - 4 * 32 == 2
    # 4, 5: the side limit on either axis
    assert p[4]["chunks"] == [256] * 16 and T.CASES[4][2] == T.K_MAX_SIDE and 16 * T.CASES[4][2] == 64 * 1024
    assert (p[5]["nbands"], p[5]["apply_bands"], p[5]["seg"]) == (128, 256, 3) and T.CASES[5][1] == T.K_MAX_SIDE
    # 6: the radius limit over four chunks; bands of 28 rows, the last of 11 = one group of 7 and 4 rows
    assert (p[6]["g"], p[6]["seg"], p[6]["band"], p[6]["nbands"], p[6]["chunks"]) == (7, 1, 28, 3, [256, 256, 256, 232])
    assert T.CASES[6][4] == T.K_MAX_RADIUS and 67 - 2 * 28 == 7 + 4
    # 7: the full-height block with a 3-column last chunk
    assert 2 * T.CASES[7][4] + 1 == T.CASES[7][1] and p[7]["chunks"] == [256, 3]
    # every channel count, and a bank larger than the batch read from its end, out of order
    assert {cs[3] for cs in T.CASES} == {1, 2, 3, 4}
    for i, cs in enumerate(T.CASES):
        src, refs = T.case_inputs(i)["u8"]
        assert refs.shape[0] == src.shape[0] + 1 and T.case_index(i).tolist() == list(range(cs[0], 0, -1))
    assert T.case_index(1).tolist() == [2, 1]


def test_the_generators_draw_what_the_table_says():
    for i, (b, h, w, c, _) in enumerate(T.CASES):
        rng = np.random.default_rng(2000 + i)
        fam = T.case_inputs(i)
        assert np.array_equal(fam["u8"][0], rng.integers(0, 256, (b, h, w, c), dtype=np.uint8))
        assert np.array_equal(fam["u8"][1], rng.integers(0, 256, (b + 1, h, w, c), dtype=np.uint8))
        for k in ("ct", "unit"):
            assert fam[k][0].dtype == fam[k][1].dtype == np.float32
            assert fam[k][0].shape == (b, h, w, c) and fam[k][1].shape == (b + 1, h, w, c)
        assert fam["ct"][0].min() < -1000.0 and fam["ct"][0].max() > 1000.0 and not np.array_equal(fam["ct"][0], np.rint(fam["ct"][0]))
        assert 0.0 <= fam["unit"][0].min() and fam["unit"][0].max() < 1.0
    src, refs = T.zero_inputs()
    assert not src[..., 1].any() and src[..., 0].any() and src[..., 2].any() and refs.shape == (1, 33, 300, 3)
    assert not T.zero_inputs(whole=True)[0].any() and np.array_equal(T.zero_inputs(whole=True)[1], refs)
    deg = T.degenerate_inputs()[0][0]
    assert np.all(deg[..., 0] == 7.0) and np.all(deg[..., 1] == deg[:1, :, 1]) and np.all(deg[..., 2] == deg[:, :1, 2])
    assert len(np.unique(deg[0, :, 1])) > 100 and len(np.unique(deg[:, 0, 2])) > 20


# ---------------------------------------------------------------------------------------------- uint8 conditions
def _tie(ref):
    return float(np.abs(ref - np.floor(ref) - 0.5).min())


def test_the_uint8_references_have_no_tie_no_vanishing_bin_and_saturate():
    """what makes 'equal on every pixel' a fair demand of the GPU tests"""
    worst_tie, worst_amp = (np.inf, None), (np.inf, None)
    for i, cs in enumerate(T.CASES):
        src, _, _, ref = T.case_reference(i, "u8")
        tie, amp = _tie(ref), R.block_min_amplitude(src, cs[4])
        print("case %d %r: smallest tie distance %.3g, smallest |S| %.4g, reference spans %.4g .. %.4g" % (i, cs, tie, amp, ref.min(), ref.max()))
        assert tie >= 1e-8 and amp >= 1.0
        assert ref.min() < -0.5 or ref.max() > 255.5, "the saturating store acts"
        worst_tie, worst_amp = min(worst_tie, (tie, i)), min(worst_amp, (amp, i))
    print("smallest tie distance %.3g at case %d, smallest |S| %.4g at case %d" % (worst_tie + worst_amp))
    # the per-sample radii on case 2 at B = 3: samples 0 and 2 are adapted (radius 0 and 9)
    src, _, ref = T.radii_reference()
    tie, amp = _tie(ref[[0, 2]]), R.block_min_amplitude(src[[0, 2]], T.CASES[T.RADII_CASE][4])
    print("case 2 at B = 3, radii %r: smallest tie distance %.3g, smallest |S| %.4g" % (T.RADII, tie, amp))
    assert tie >= 1e-8 and amp >= 1.0 and np.array_equal(ref[1], src[1])


def test_the_zero_planes_vanish_exactly_and_the_others_do_not():
    b = T.ZERO_CASE[4]
    for whole in (False, True):
        src, refs, ref = T.zero_reference(whole)
        tie = _tie(ref)
        print("Z%s: smallest tie distance %.3g, reference spans %.4g .. %.4g" % (" (whole sample zero)" if whole else "", tie, ref.min(), ref.max()))
        assert tie >= 1e-8
        for ch in range(3):
            S = np.fft.fft2(src[0, ..., ch].astype(np.float64))
            if whole or ch == 1:
                assert not S.real.any() and not S.imag.any(), "the zero plane's fft2 is exactly 0 on every bin"
                closed = T.zero_plane_closed_form(refs[0, ..., ch], b)
                err = float(np.abs(ref[0, ..., ch] - closed).max())
                print("  channel %d: max |definition - inverse transform of |T| on the block| = %.3g, tie distance of the closed form %.3g"
                      % (ch, err, _tie(closed)))
                assert err <= T.additive(255.0) / T.MARGIN and _tie(closed) >= 1e-8
            else:
                amp = R.block_min_amplitude(src[:, ..., ch:ch + 1], b)
                print("  channel %d: smallest |S| %.4g" % (ch, amp))
                assert amp >= 1.0


# ---------------------------------------------------------------------------------------------- fp32 families
@pytest.mark.parametrize("family,floor", (("ct", 100.0), ("unit", 0.5)))
def test_the_fp32_families_keep_every_phase_well_defined(family, floor):
    worst = np.inf
    for i, cs in enumerate(T.CASES):
        amp = R.block_min_amplitude(T.case_inputs(i)[family][0], cs[4])
        print("%s case %d: smallest |S| %.4g" % (family, i, amp))
        worst = min(worst, amp)
    print("%s: smallest |S| %.4g" % (family, worst))
    assert worst >= floor


# ---------------------------------------------------------------------------------------------- reference agreement
@pytest.mark.parametrize("family", T.FAMILIES)
def test_the_low_rank_form_equals_the_full_fft_definition(family):
    """within additive(M) / 500: the margin test_fourier_adapt_gpu.py keeps between two float64 algorithms and its bound"""
    worst = 0.0
    for i, cs in enumerate(T.CASES):
        src, refs, _, ref = T.case_reference(i, family)
        low = T.case_reference(i, family, fn=R.adapt_plane_lowrank)[3]
        err, a = float(np.abs(low - ref).max()), T.additive(T.magnitude(src, refs))
        print("%s case %d %r: max |low-rank - full FFT| = %.3g, additive term %.3g / %g = %.3g" % (family, i, cs, err, a, T.MARGIN, a / T.MARGIN))
        assert err <= a / T.MARGIN
        worst = max(worst, err)
    print("%s: largest difference %.3g" % (family, worst))
    if family == "u8":
        assert T.additive(255.0) == 1e-9, "the existing bound, not a wider one"
        for name, (src, refs, ref), low in (("Z", T.zero_reference(), T.zero_reference(fn=R.adapt_plane_lowrank)[2]),
                                            ("Z whole", T.zero_reference(True), T.zero_reference(True, fn=R.adapt_plane_lowrank)[2]),
                                            ("radii", T.radii_reference(), T.radii_reference(fn=R.adapt_plane_lowrank)[2])):
            err = float(np.abs(low - ref).max())
            print("%s: max |low-rank - full FFT| = %.3g" % (name, err))
            assert err <= 1e-9 / T.MARGIN


# ---------------------------------------------------------------------------------------------- the bank
def test_the_bank_amplitudes_two_ways():
    """``|fft2(t)|`` against the explicit DFT matrices over the half block, relative to M H W: the figure behind the bank
    tolerance of the GPU test (``fourier_edge_cases.BANK_REL``)"""
    worst = 0.0
    for i, cs in enumerate(T.CASES):
        for family in T.FAMILIES:
            refs = T.case_inputs(i)[family][1]
            a, d = T.bank_fft(refs, cs[4]), T.bank_dft(refs, cs[4])
            assert a.shape == d.shape == (refs.shape[0], cs[3], 2 * cs[4] + 1, cs[4] + 1)
            rel = float(np.abs(a - d).max()) / (float(np.abs(refs.astype(np.float64)).max()) * cs[1] * cs[2])
            print("%s case %d %r: max ||fft2| - |DFT matrices|| / (M H W) = %.3g" % (family, i, cs, rel))
            worst = max(worst, rel)
            assert T.bank_tolerance(refs) == T.MARGIN * T.BANK_REL * np.abs(refs.astype(np.float64)).max() * cs[1] * cs[2]
    print("largest: %.3g (BANK_REL = %g)" % (worst, T.BANK_REL))
    assert worst <= T.BANK_REL
    # the layout: ky = -b..b in that order, kx = 0..b, per (reference, channel)
    refs = T.case_inputs(1)["u8"][1]
    full = np.abs(np.fft.fft2(refs[2, ..., 1].astype(np.float64)))
    assert T.bank_fft(refs, 2)[2, 1, 0, 1] == full[-2 % 5, 1] and T.bank_fft(refs, 2)[2, 1, 4, 2] == full[2, 2]


# ---------------------------------------------------------------------------------------------- degenerate planes
def test_degenerate_planes_keep_the_bins_outside_the_block_on_the_references():
    """the one property the GPU test asserts on planes that are constant along an axis, held here by both restatements"""
    src, refs = T.degenerate_inputs()
    _, h, w, c, b = T.ZERO_CASE
    a = T.additive(T.magnitude(src, refs))
    outside = T.block_mask(h, w, b) == 0.0
    for fn in (R.adapt_plane_fft, R.adapt_plane_lowrank):
        out = R.adapt_batch(src, refs, b, [0], fn=fn).astype(np.float32).astype(np.float64)      # (the fp32 store)
        assert np.isfinite(out).all()
        for ch in range(c):
            diff = np.abs(np.fft.fft2(out[0, ..., ch]) - np.fft.fft2(src[0, ..., ch].astype(np.float64)))[outside].max()
            bound = h * w * (2.0 ** -24 * np.abs(out[0, ..., ch]).max() + a)
            print("%s plane %d: max |fft2(out) - fft2(src)| outside the block = %.3g, bound %.3g" % (fn.__name__, ch, diff, bound))
            assert diff <= bound
