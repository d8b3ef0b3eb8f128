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


# ------------------------------------------------------------------------------------------ the purpose-built kernels' paths
def _affine_data(seed=5, n=2, c1=24, c2=16, cout=40, h=12, w_=16, k=3):
    rng = np.random.default_rng(seed)
    t = lambda *s, sd=1.0, mu=0.0: torch.from_numpy(rng.normal(mu, sd, s).astype(np.float32))
    # shifts far from zero: a border padded BEFORE the affine would carry them
    return dict(x1=t(n, c1, h, w_), x2=t(n, c2, h, w_), sc=t(c1, sd=0.3, mu=1.0), sh=t(c1, sd=0.3, mu=2.5),
                w=t(cout, c1 + c2, k, k, sd=0.1), b=t(cout, sd=0.1), dz=t(n, cout, h, w_),
                g=R.Geom(n, c1 + c2, cout, h, w_, k, 1, k // 2, 1))


def test_affine_operand_is_the_singly_rounded_fma():
    d = _affine_data()
    a = R.affine_operand(d["x1"], d["sc"], d["sh"])
    exact = d["x1"].double() * d["sc"].double()[None, :, None, None] + d["sh"].double()[None, :, None, None]
    assert a.dtype == torch.float32
    # within half an fp32 ulp of the exact value (2^-24 relative), and NOT the doubly rounded fp32 product + sum everywhere
    assert bool(((a.double() - exact).abs() <= 2.0 ** -24 * exact.abs()).all())
    two_step = d["x1"] * d["sc"][None, :, None, None] + d["sh"][None, :, None, None]
    assert bool((two_step != a).any())
    assert torch.equal(R.affine_operand(d["x1"]), d["x1"])
    cat = R.source_operand(d["x1"], d["sc"], d["sh"], d["x2"])
    assert torch.equal(cat[:, :24], a) and torch.equal(cat[:, 24:], d["x2"])


def test_affine_and_two_sources_equal_autograd_in_float64():
    """prec=None: forward, weight gradient and data gradient of conv(cat(x1 * sc + sh, x2)) against torch autograd in float64
    (the operand's own fp32 rounding taken out by building the autograd graph ON the operand)"""
    d = _affine_data()
    g = d["g"]
    xin = R.source_operand(d["x1"], d["sc"], d["sh"], d["x2"]).double().requires_grad_(True)
    wt = d["w"].double().requires_grad_(True)
    bias = d["b"].double().requires_grad_(True)
    z = torch.nn.functional.conv2d(xin, wt, bias, padding=1)
    y = torch.nn.functional.leaky_relu(z, 0.2)
    z.backward(d["dz"].double())
    op = R.source_operand(d["x1"], d["sc"], d["sh"], d["x2"])
    assert torch.allclose(R.forward_ref(g, op, d["w"], d["b"], 0.2, None), y.detach(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(R.wgrad_ref(g, op, d["dz"], None), wt.grad, rtol=1e-13, atol=1e-12)
    assert torch.allclose(R.dgrad_ref(g, d["dz"], d["w"], None), xin.grad, rtol=1e-13, atol=1e-13)
    assert torch.allclose(R.chan_sums(d["dz"])[0], bias.grad, rtol=1e-13, atol=1e-12)
    # the direct model with prec=None is the same unrounded expression
    assert torch.equal(R.forward_ref(g, op, d["w"], d["b"], 0.2, None, model="direct"), R.forward_ref(g, op, d["w"], d["b"], 0.2, None))
    # an affine on the gradient (the row-streaming data gradient's AFF instantiations): the operand is the transformed dy
    sc, sh = d["sc"].repeat(2)[:g.cout], d["sh"].repeat(2)[:g.cout]
    dyo = R.affine_operand(d["dz"], sc, sh)
    want = torch.nn.grad.conv2d_input((g.n, g.cin, g.h, g.w), d["w"].double(), dyo.double(), padding=1)
    assert torch.allclose(R.dgrad_ref(g, dyo, d["w"], None), want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("prec", [None, "bf16x3", "bf16"])
def test_padding_after_the_affine_differs_from_affine_after_padding_by_the_border_term(prec):
    """conv(pad0(fma(x))) against conv(fma(pad0(x))): the second sees ``sh`` on the padding ring, so the difference is the
    convolution of a tensor that is ``sh`` on the ring and zero inside -- evaluated on the same operand planes -- and it
    vanishes away from the border"""
    d = _affine_data(c2=0, c1=32)
    g, F = d["g"], torch.nn.functional
    op = R.affine_operand(d["x1"], d["sc"], d["sh"])
    after = R.forward_ref(g, op, d["w"], None, 1.0, prec)                                 # the kernels' order
    g0 = R.Geom(g.n, g.cin, g.cout, g.h + 2, g.w + 2, 3, 1, 0, 1)
    padded = R.affine_operand(F.pad(d["x1"], (1, 1, 1, 1)), d["sc"], d["sh"])             # the wrong order
    before = R.forward_ref(g0, padded, d["w"], None, 1.0, prec)
    ring = padded.clone()
    ring[:, :, 1:-1, 1:-1] = 0.0
    term = R.forward_ref(g0, ring, d["w"], None, 1.0, prec)
    assert before.shape == after.shape == term.shape
    assert torch.allclose(before - after, term, rtol=0, atol=1e-12 * float(after.abs().max()))
    assert float(term[:, :, 1:-1, 1:-1].abs().max()) == 0.0
    # with shifts of 2.5 the border term is of the size of the output itself: a wrongly padded border cannot pass any bound
    assert float(term[:, :, 0].abs().max()) > 0.5 * float(after.abs().max())
    # the same for the weight gradient: its border term is the gradient against the ring
    wa = R.wgrad_ref(g, op, d["dz"], prec)
    wb = R.wgrad_ref(g0, padded, d["dz"], prec)
    assert torch.allclose(wb - wa, R.wgrad_ref(g0, ring, d["dz"], prec), rtol=0, atol=1e-12 * float(wa.abs().max()))
    assert R.rel_err(wb, wa) > 1e-2


@pytest.mark.parametrize("op", ["fwd", "dgrad"])
def test_direct_model_against_the_bf16x3_model(op):
    """direct - bf16x3 = sum xl wl + sum r (wh + wl) <= 2^-17 (1 + 2^-8) sum |x| |w| (module docstring of conv_exact_ref), and
    it is not zero; in bf16 mode the direct model keeps the unrounded activation: (x - xh) wh, <= 2^-9 sum |x| |wh|"""
    d = _affine_data()
    g, F = d["g"], torch.nn.functional
    x = R.source_operand(d["x1"], d["sc"], d["sh"], d["x2"])
    if op == "fwd":
        f = lambda prec, model: R.forward_ref(g, x, d["w"], None, 1.0, prec, model=model)
        mag = lambda wabs: F.conv2d(x.double().abs(), wabs, padding=1)
    else:
        f = lambda prec, model: R.dgrad_ref(g, d["dz"], d["w"], prec, model=model)
        mag = lambda wabs: torch.nn.grad.conv2d_input((g.n, g.cin, g.h, g.w), wabs, d["dz"].double().abs(), padding=1)
    diff = (f("bf16x3", "direct") - f("bf16x3", "mfma")).abs()
    lim = 2.0 ** -17 * (1 + 2.0 ** -8) * mag(d["w"].double().abs())
    assert bool((diff <= lim).all()) and float(diff.max()) > 0.0
    assert float((diff / lim).max()) > 1e-3            # the bound is not vacuous: the terms are of that order
    wh = R.split_hi_lo(d["w"])[0].double()
    diff1 = (f("bf16", "direct") - f("bf16", "mfma")).abs()
    assert bool((diff1 <= 2.0 ** -9 * mag(wh.abs())).all()) and float(diff1.max()) > 0.0
    # and the direct model is the closer one to the unrounded convolution in bf16x3 mode: only the weight's 2^-18 is left
    plain = f(None, "mfma")
    assert bool(((f("bf16x3", "direct") - plain).abs() <= 2.0 ** -17 * mag(d["w"].double().abs())).all())
    assert R.bound_of(1.0, None) == R.FACTOR      # one chain
