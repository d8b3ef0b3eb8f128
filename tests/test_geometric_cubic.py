"""Order 3 of the device-side geometric augmentation without a GPU: the fixture
tests/golden/geometric_cubic.npz regenerates exactly (scripts/make_geometric_cubic_golden.py: a numpy restatement pinned by one
in exact rational arithmetic), the weights and the anchors of the rule hold on the restatement, GeoProgram accepts the orders
{0, 1, 3}, the samplers' ``interp`` keyword draws what the issue sets, and the assembly keeps the order-0 / 1 kernel's
registers."""
import importlib.util
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLD, ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")


def _load(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))


C = _load("make_geometric_cubic_golden")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLD, "geometric_cubic.npz"))


# ---------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_exactly_and_is_small(fixture):
    assert os.path.getsize(os.path.join(GOLD, "geometric_cubic.npz")) < 1000000
    g = C.build()      # (asserts that the two restatements agree, the cap, the clean chain and both clips)
    assert sorted(g) == sorted(fixture.files)
    for k in fixture.files:
        assert np.array_equal(g[k], fixture[k]), k
    tot, exc = (int(v) for v in fixture["counts"])
    assert exc <= 1e-5 * tot
    lo, hi = fixture["stripes_extremes"]
    assert lo < -0.5 and hi >= 255.5, "the 0 / 255 case reaches both clips"


def test_fixture_holds_the_cases_the_rule_needs_and_numpy_reproduces_them(fixture):
    cases = C.load_cases(fixture)
    names = [c["name"] for c in cases]
    for (h, w), ch in C.SHAPES:
        for kind in ("modes", "perspective", "crop_pad", "elastic", "piecewise"):
            assert "%s_%dx%d_c%d" % (kind, h, w, ch) in names
    by = {c["name"]: c for c in cases}
    for (h, w), ch in C.SHAPES:
        tag = "_%dx%d_c%d" % (h, w, ch)
        m = by["modes" + tag]
        assert set(m["iarg"][:, 0, 1]) == set(range(5)) and np.all(m["iarg"][:, 0, 0] == 3)
        assert sorted(by["elastic" + tag]["iarg"][:, 0, 3]) == [0, 1, 4] and sorted(by["piecewise" + tag]["iarg"][:, 0, 3]) == [2, 3, 4]
    chain = [c for c in cases if c["chain"]]
    assert len(chain) == 1 and set(chain[0]["iarg"][..., 0].ravel()) == {0, 1, 3}
    assert any(c["kind"] == "stripes" and set(np.unique(c["images"])) == {0, 255} for c in cases)
    for c in cases:
        assert len(c["exc"]) == 0 and np.all(c["iarg"][..., 0][c["opcode"] != 0] != 2)
        assert not np.array_equal(c["lab"], c["labels"]), "labels move in every case"
        got, lab, _, _ = C.run_program(c["images"], c["labels"], c["opcode"], c["iarg"], c["farg"], c["seed_arr"], backend="numpy")
        assert np.array_equal(got, c["u8"]) and np.array_equal(lab, c["lab"]), c["name"]


# ---------------------------------------------------------------------------------------------- the rule
def test_weights_match_the_values_the_rule_states():
    assert C.cubic_weights(np.float64(0.0)) == (0.0, 1.0, 0.0, 0.0)
    assert C.cubic_weights(np.float64(0.5)) == (-0.09375, 0.59375, 0.59375, -0.09375)
    w = C.cubic_weights(np.float64(0.5))
    row = lambda p: ((p[0] * w[0] + p[1] * w[1]) + p[2] * w[2]) + p[3] * w[3]
    assert row((255.0, 0.0, 0.0, 255.0)) == -47.8125 and row((0.0, 255.0, 255.0, 0.0)) == 302.8125
    rng = np.random.default_rng(0)
    for t in list(rng.random(200)) + [0.0, 0.5, 2.0 ** -52, 1.0 - 2.0 ** -53]:
        exact = C.cubic_weights_exact(Fraction(float(t)))
        num, den = C._int_weights(Fraction(float(t)))
        assert [Fraction(n, den) for n in num] == exact and sum(exact) == 1
        # (the float recipe passes through intermediates of up to 6 in magnitude: a few roundings of 6 x 2^-53 each)
        assert np.allclose([float(v) for v in exact], C.cubic_weights(np.float64(t)), rtol=0, atol=1e-14)


def _one(img, lab, matrix, order, mode, cval=7):
    p = C.Prog(1)
    p.homography(0, 0, matrix, order, mode, cval)
    out, labels, _, _ = C.run_program(img[None], lab[None], p.opcode, p.iarg, p.farg, p.seed, backend="numpy")
    return out[0], labels[0]


@pytest.mark.parametrize("shape", [(9, 11, 3), (2, 2, 1), (3, 3, 2), (2, 5, 4)])
def test_anchors_hold_on_the_restatement(shape):
    h, w, c = shape
    rng = np.random.default_rng(3)
    img, lab = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 5, (h, w)).astype(np.int64)
    for mode in range(5):
        out, labels = _one(img, lab, np.eye(3), 3, mode)
        assert np.array_equal(out, img) and np.array_equal(labels, lab), "identity, mode %d" % mode
        for m in (C.G.flip_lr(w), C.G.flip_ud(h)):
            a, b = _one(img, lab, m, 3, mode), _one(img, lab, m, 0, mode)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for ty, tx in ((1, 2), (-3, 5), (h + 1, -2 * w - 1)):
        out, _ = _one(img, lab, np.array([[1.0, 0.0, -tx], [0.0, 1.0, -ty], [0.0, 0.0, 1.0]]), 3, C.WRAP)
        assert np.array_equal(out, np.roll(img, (ty, tx), axis=(0, 1)))


# ---------------------------------------------------------------------------------------------- the host side
def test_validate_accepts_orders_0_1_3_and_rejects_the_rest():
    from pointcloududa_amd.utils import geometric as P
    h, w = 32, 24
    prog = P.GeoProgram.identity(2, 6)
    assert not prog.uses_cubic()
    prog.set_homography(0, 0, np.eye(3), order=3, mode=P.MODE_WRAP, cval=3)
    prog.set_affine(0, 1, h, w, rotate=10.0, order=3)
    prog.set_elastic(0, 2, 2.0, 0.25, 5, order=3)
    prog.set_piecewise(0, 3, h, w, np.zeros((3, 3)), np.zeros((3, 3)), order=3)
    prog.set_elastic(1, 0, 2.0, 0.25, 5)
    prog.validate(h, w)
    assert prog.uses_cubic() and list(prog.iarg[0, :4, 0]) == [3, 3, 3, 3] and prog.iarg[1, 0, 0] == 1
    for bad in (2, -1, 4, 5):
        q = P.GeoProgram.identity(2, 2)
        q.set_flip_lr(1, 1, w)
        q.iarg[1, 1, 0] = bad
        with pytest.raises(ValueError, match="order"):
            q.validate(h, w)
    # an order-3 NOP slot is nobody's business: the entry stays the old one
    q = P.GeoProgram.identity(1, 1)
    q.iarg[0, 0, 0] = 3
    q.validate(h, w)
    assert not q.uses_cubic()
    assert P.ORDERS == (0, 1, 3)


def test_the_entry_is_declared_and_bound():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    assert re.search(r"int pcuda_geometric_cubic\(", hdr) and "#define PCUDA_ABI_VERSION 5" in hdr
    assert _lib._PROTOS["pcuda_geometric_cubic"] == _lib._PROTOS["pcuda_geometric"]
    src = open(os.path.join(CSRC, "geometric.hip")).read()
    assert 'extern "C" int pcuda_geometric_cubic(' in src
    import inspect
    from pointcloududa_amd import kernels as K
    assert inspect.signature(K.geometric).parameters["cubic"].default is False


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_cubic_instance_does_not_spill_and_the_old_instance_keeps_its_registers():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=geometric.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(os.path.join(CSRC, "build", "isa", "geometric.s")).read()
    meta = re.findall(r"\.name:\s+(\S*geometric_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text)
    rows = {("cubic" if "ILb1E" in name else "plain"): (int(scratch), int(vgpr)) for name, scratch, vgpr in meta}
    assert set(rows) == {"cubic", "plain"}, meta
    assert rows["cubic"][0] == 0 and rows["plain"][0] == 0, "a kernel spills to scratch"
    assert rows["plain"][1] <= 71, "the order-0 / 1 instance grew: %d VGPRs (71 before order 3)" % rows["plain"][1]
    print("VGPRs: order 0 / 1 instance %d, cubic instance %d" % (rows["plain"][1], rows["cubic"][1]))


# ---------------------------------------------------------------------------------------------- the samplers
def _state(rng):
    return rng.bit_generator.state["state"]


def _stage_arrays(st):
    return [(k, getattr(st, k)) for k in ("opcode", "iarg", "farg", "seed", "table") if hasattr(st, k)]


def test_interp_is_linear_by_default_and_unknown_strings_raise():
    from pointcloududa_amd.utils import augment as A
    for fn in (A.sample_geo_program, A.sample_style_program, A.sample_heavy_plan):
        a, b = np.random.default_rng(5), np.random.default_rng(5)
        x, y = fn(4, "heavy_full_device", a, 64, 48), fn(4, "heavy_full_device", b, 64, 48, interp="linear")
        assert _state(a) == _state(b)
        for p, q in zip(getattr(x, "stages", [x]), getattr(y, "stages", [y])):
            assert all(np.array_equal(u[1], v[1]) for u, v in zip(_stage_arrays(p), _stage_arrays(q)))
        for bad in ("nearest", "Cubic", "", None, 3):
            with pytest.raises(ValueError, match="interp"):
                fn(4, "heavy_full_device", np.random.default_rng(5), 64, 48, interp=bad)
    with pytest.raises(ValueError, match="interp"):
        A.AugmentedBatches(iter(()), None, None, np.random.default_rng(0), rescale="div255", heavy_preset="heavy_device", heavy_interp="spline")
    from pointcloududa_amd.utils import heavy
    assert len(heavy._PRESETS) == 8, "interp adds no preset"


def test_cubic_draws_over_1000_seeds():
    """every elastic slot has order 3, a noise-alpha slot is cubic exactly where the extra draw is below 0.35, every other
    array equals the linear draw of the same seed, and the generator is consumed by exactly one random(B) more"""
    from pointcloududa_amd.utils import geometric as P, heavy, stylize as St
    presets = sorted(heavy._PRESETS)
    b, h, w = 4, 32, 24
    seen = dict(elastic=0, cubic_up=0, other_up=0)
    for seed in range(1000):
        preset = presets[seed % len(presets)]
        for fn in (heavy.sample_heavy_plan, heavy.sample_geo_program, heavy.sample_style_program):
            lin_rng, cub_rng = np.random.default_rng(seed), np.random.default_rng(seed)
            try:
                lin = fn(b, preset, lin_rng, h, w)
            except ValueError:      # (sample_style_program on a preset without a stylize entry)
                with pytest.raises(ValueError):
                    fn(b, preset, cub_rng, h, w, interp="cubic")
                continue
            cub = fn(b, preset, cub_rng, h, w, interp="cubic")
            extra = lin_rng.random(b)
            assert _state(lin_rng) == _state(cub_rng), "exactly one random(B) more, after every other draw"
            ls, cs = getattr(lin, "stages", [lin]), getattr(cub, "stages", [cub])
            assert [type(s) for s in ls] == [type(s) for s in cs]
            for p, q in zip(ls, cs):
                want_iarg = p.iarg.copy()
                if isinstance(p, P.GeoProgram):
                    el = p.opcode == P.OP_ELASTIC
                    assert np.all(p.iarg[el][:, 0] == 1) and np.all(q.iarg[el][:, 0] == 3)
                    want_iarg[..., 0][el] = 3
                    seen["elastic"] += int(el.sum())
                    assert q.uses_cubic() == bool(el.any()) and not p.uses_cubic()
                elif isinstance(p, St.StyleProgram):
                    na = (p.opcode == St.OP_NOISE_ALPHA_CONV3X3) & (extra < St.NOISE_CUBIC_P)[:, None]
                    want_iarg[..., 1][na] = St.UPSCALE_CUBIC
                    seen["cubic_up"] += int(na.sum())
                    seen["other_up"] += int(((p.opcode == St.OP_NOISE_ALPHA_CONV3X3) & ~na).sum())
                    q.validate(h, w, 3)
                for (k, u), (_, v) in zip(_stage_arrays(p), _stage_arrays(q)):
                    assert np.array_equal(want_iarg if k == "iarg" else u, v), (seed, preset, k)
    assert St.NOISE_CUBIC_P == 0.35
    assert seen["elastic"] > 100 and seen["cubic_up"] > 100
    share = seen["cubic_up"] / float(seen["cubic_up"] + seen["other_up"])
    assert 0.30 < share < 0.40, share
