"""CPU checks of tests/conv_exact_ref.py: the hi/lo split, the operand-exact references against the unrounded fp64
convolution, the size of the fp32 yardstick e32, and the Python mirrors of the variant keys against csrc/built_variants.h."""
import itertools

import numpy as np
import pytest
import torch

import conv_exact_ref as R

# 3x3 / 4x4 stride 2 / dilated
GEOMS = {
    "3x3": R.Geom(2, 24, 40, 20, 24, 3, 1, 1, 1),
    "4x4s2": R.Geom(2, 16, 48, 21, 18, 4, 2, 2, 1),
    "dil4": R.Geom(2, 40, 24, 16, 16, 3, 1, 4, 4),
}


def _data(g, seed=0):
    rng = np.random.default_rng(seed)
    t = lambda *s, sd=1.0: torch.from_numpy(rng.normal(0, sd, s).astype(np.float32))
    return (t(g.n, g.cin, g.h, g.w), t(g.cout, g.cin, g.k, g.k, sd=0.1), t(g.cout, sd=0.1), t(g.n, g.cout, g.oh, g.ow))


def test_hi_lo_split_reproduces_the_operand_to_2_pow_minus_16():
    rng = np.random.default_rng(1)
    a = torch.from_numpy(np.concatenate([rng.normal(0, 1, 1 << 16), rng.normal(0, 1e-6, 1 << 12), rng.normal(0, 1e6, 1 << 12),
                                         [1.0, -1.0, 0.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 3.0 - 2.0 ** -7]]).astype(np.float32))
    hi, lo = R.split_hi_lo(a)
    for p in (hi, lo):      # both planes are bf16 values: the low 16 bits of the fp32 pattern are clear
        assert not np.any(p.numpy().view(np.uint32) & 0xffff)
    err = (hi.double() + lo.double() - a.double()).abs()
    assert bool((err <= 2.0 ** -16 * a.double().abs()).all())
    assert bool(((hi.double() - a.double()).abs() <= 2.0 ** -8 * a.double().abs()).all())
    # round to nearest EVEN: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 -> 1; 3 - 2^-7 is a tie between 3 - 2^-6 and 3 -> 3
    assert R.bf16_rne(torch.tensor([1.0 + 2.0 ** -8, 3.0 - 2.0 ** -7])).tolist() == [1.0, 3.0]


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_references_against_the_unrounded_convolution_and_e32(name):
    g = GEOMS[name]
    x, w, b, dz = _data(g)
    ops = {
        "fwd": lambda prec: (lambda dt: R.forward_ref(g, x, w, b, 0.2, prec, dt)),
        "dgrad": lambda prec: (lambda dt: R.dgrad_ref(g, dz, w, prec, dt)),
        "wgrad": lambda prec: (lambda dt: R.wgrad_ref(g, x, dz, prec, dt)),
    }
    for opname, mk in ops.items():
        plain = mk(None)(torch.float64)
        for prec in ("bf16x3", "bf16"):
            e32, exact = R.e32_of(mk(prec), axis=0 if opname == "wgrad" else 1)
            assert exact.shape == plain.shape
            assert R.rel_err(exact, plain) < R.OLD_TOL[prec], (opname, prec)
            assert 0.0 < e32 < 1e-5, (opname, prec, e32)
        # the two modes differ (the lo planes are not empty) and bf16x3 is the closer one by orders of magnitude
        e3 = R.rel_err(mk("bf16x3")(torch.float64), plain)
        e1 = R.rel_err(mk("bf16")(torch.float64), plain)
        assert e3 < 1e-2 * e1, (opname, e3, e1)


def test_fp32_steps_behind_the_sum():
    g = R.Geom(2, 8, 8, 8, 8, 3, 1, 1, 1, in_up=True)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.normal(0, 1, (2, 8, 4, 4)).astype(np.float32))
    w = torch.from_numpy(rng.normal(0, 0.1, (8, 8, 3, 3)).astype(np.float32))
    dz = torch.from_numpy(rng.normal(0, 1, (2, 8, 8, 8)).astype(np.float32))
    base = torch.from_numpy(rng.normal(0, 1, (2, 8, 8, 8)).astype(np.float32))
    a = torch.from_numpy(rng.normal(0, 1, (2, 8, 8, 8)).astype(np.float32))
    d = R.dgrad_ref(g, dz, w, "bf16x3")
    assert torch.equal(R.dgrad_ref(g, dz, w, "bf16x3", fold=True), R.fold2(d)) and R.fold2(d).shape == (2, 8, 4, 4)
    assert torch.equal(R.dgrad_ref(g, dz, w, "bf16x3", base=base), d + base.double())
    assert torch.equal(R.dgrad_ref(g, dz, w, "bf16x3", mask=(a, 0.2)), torch.where(a > 0, d, d * 0.2))
    # the in_up forward reads the stored tensor through the nearest-x2 fold: its weight gradient sees the upsampled one
    gup = R.Geom(2, 8, 8, 8, 8, 3, 1, 1, 1)
    xu = torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
    assert torch.equal(R.wgrad_ref(g, x, dz, "bf16"), R.wgrad_ref(gup, xu, dz, "bf16"))
    assert torch.equal(R.forward_ref(g, x, w, None, 1.0, "bf16"), R.forward_ref(gup, xu, w, None, 1.0, "bf16"))
    (s1, a1), (s2, a2) = R.bn_fwd_sums(d)
    assert torch.allclose(s1, d.sum((0, 2, 3))) and torch.allclose(s2, (d * d).sum((0, 2, 3))) and bool((a1 >= s1.abs()).all())
    # the measures: a wrong channel cannot hide behind a large one
    ref = torch.ones(1, 2, 4, 4, dtype=torch.float64)
    ref[:, 1] *= 1000.0
    got = ref.clone()
    got[0, 0, 0, 0] += 0.5
    assert R.rel_err(got, ref) == pytest.approx(5e-4) and R.chan_err(got, ref) == pytest.approx(0.5)
    got[0, 0, 0, 0] = float("nan")
    assert R.chan_err(got, ref) == float("inf")


def test_key_mirrors_round_trip():
    n = 0
    for x3, cb, cl, npb, pf, xq, st, te in itertools.product((0, 1), (1, 2), (0, 1), (1, 2), (1, 2, 3), (0, 1), (0, 1, 2), (0, 1)):
        k = R.pipe_key(x3, cb, cl, npb, pf, xq, st, te)
        assert R.pipe_fields(k) == dict(x3=x3, co_blks=cb, clamp=cl, npb=npb, pf=pf, xq=xq, stats=st, te=te) and k < 1 << 10
        assert R.pipe_key(**R.pipe_fields(k)) == k
        n += 1
    for x3, cb, cl, npbt, pf, xq, st in itertools.product((0, 1), (1, 2), (0, 1), (4, 8), (1, 2), (0, 1), (0, 1)):
        k = R.ig8_key(x3, cb, cl, npbt, pf, xq, st)
        assert R.ig8_fields(k) == dict(x3=x3, co_blks=cb, clamp=cl, npbt=npbt, pf=pf, xq=xq, stats=st) and k < 1 << 8
        n += 1
    for x3, cb, md, tm, pf, nw, xq in itertools.product((0, 1), (1, 2), (0, 1, 2), (1, 9, 16), (0, 1, 2, 3), (4, 8), (0, 1)):
        k = R.wgrad_key(x3, cb, md, tm, pf, nw, xq)
        assert R.wgrad_fields(k) == dict(x3=x3, co_blks=cb, mode=md, taps_max=tm, pf=pf, nw=nw, xq=xq) and k < 1 << 10
        n += 1
    assert n == 2 * 2 * 2 * 2 * 3 * 2 * 3 * 2 + 2 ** 4 * 2 * 2 * 2 + 2 * 2 * 3 * 3 * 4 * 2 * 2
    # the encodings of csrc/variants.h, spelled out once each
    assert R.pipe_key(True, 2, False, 2, 3, True, 2, True) == 1 + 2 + 8 + 32 + 64 + 256 + 512
    assert R.ig8_key(True, 2, True, 8, 2, True, True) == 1 + 2 + 4 + 8 + 16 + 64 + 128
    assert R.wgrad_key(True, 2, 1, 9, 3, 4, True) == 663 and R.wgrad_key(False, 1, 2, 16, 2, 8, False) == 8 + 32 + 192 + 256
    assert R.variant_id("wgrad", 663) == "wgrad-663-bf16x3-cb2-mode1-t9-pf3-xq"


def test_built_variants_header_decodes_to_legal_fields_and_counts():
    lists, counts = R.parse_built_variants()
    assert tuple(len(lists[f]) for f in ("pipe", "ig8", "wgrad")) == counts == (44, 31, 52)
    ids = set()
    for fam, keys in lists.items():
        assert len(set(keys)) == len(keys) and keys == sorted(keys), fam
        for k in keys:
            assert 0 <= k < 1 << R.KEY_BITS[fam], (fam, k)
            f = R.FIELDS_FN[fam](k)
            assert R.fields_legal(fam, f), (fam, k, f)
            assert R.KEY_FN[fam](**f) == k, (fam, k, f)
            ids.add(R.variant_id(fam, k))
    assert len(ids) == sum(counts)


def test_one_accumulator_for_three_planes_rounds_more_than_one_chain():
    """The model behind ACC_CHAINS: the bf16x3 kernels add the three planes of every 16-product step into ONE fp32 accumulator
    (one rounding per MFMA, idealised as round-to-nearest), the float32 evaluation behind e32 sums each plane on its own and
    adds the three results.  The interleaved chain rounds three times per step at the full sum's magnitude: between sqrt(3)
    (independent roundings) and 3 (all one way) times the single chain's error."""
    rng = np.random.default_rng(0)
    m, k = 1024, 1024
    a = torch.from_numpy(rng.normal(0, 1, (m, k)).astype(np.float32))
    b = torch.from_numpy(rng.normal(0, 0.1, (m, k)).astype(np.float32))
    pl = [(x.double().numpy(), y.double().numpy()) for x, y in R.planes(a, b, "bf16x3")]
    assert R.ACC_CHAINS == {"bf16": 1, "bf16x3": len(pl)} and len(R.planes(a, b, "bf16")) == 1
    ref = sum((x * y).sum(1) for x, y in pl)
    one, sep = np.zeros(m, np.float32), [np.zeros(m, np.float32) for _ in pl]
    for s in range(0, k, 16):
        for i, (x, y) in enumerate(pl):
            g = (x[:, s:s + 16] * y[:, s:s + 16]).sum(1)          # exact products, float64 sum of 16
            one = (one.astype(np.float64) + g).astype(np.float32)
            sep[i] = (sep[i].astype(np.float64) + g).astype(np.float32)
    e_one = np.abs(one - ref)
    e_sep = np.abs((sep[0] + sep[1]) + sep[2] - ref)
    ratio = float(np.sqrt((e_one ** 2).mean() / (e_sep ** 2).mean()))
    print("interleaved / separate rms error:", ratio)
    assert 1.4 < ratio <= 3.0
