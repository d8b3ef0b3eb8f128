"""CPU checks of the device-side stylize augmentation (pointcloududa_amd/utils/stylize.py, csrc/stylize.hip; DESIGN.md
section 6, f9): the independent restatement against the vectorised one (scripts/make_stylize_golden.py), the fixture
regenerating exactly, its case set, hand-computable hue cases, the edge-weight helpers, the simplex grid, the package's
encoders against the generator's, validation, the presets' statistics, and the C declaration against the binding.  No GPU and
no library load.

scipy runs in a child process (see tests/test_eval_metrics.py)."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import GOLD, ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
GEN = os.path.join(ROOT, "scripts", "make_stylize_golden.py")
needs_scipy = pytest.mark.skipif(importlib.util.find_spec("scipy") is None, reason="the restatement needs scipy")


def _helper():
    sys.path.insert(0, os.path.dirname(GEN))
    try:
        spec = importlib.util.spec_from_file_location("make_stylize_golden", GEN)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(os.path.dirname(GEN))
    return m


def _in_child(body):
    code = "import sys, numpy as np\nsys.path.insert(0, %r)\nimport make_stylize_golden as G\n" % os.path.dirname(GEN)
    r = subprocess.run([sys.executable, "-c", code + textwrap.dedent(body)], capture_output=True, text=True,
                       env=dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1"), timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------- the two restatements
@needs_scipy
def test_independent_restatement_matches_the_vectorised_one_and_the_fixture_regenerates():
    """hue and superpixels (plain Python integers) identical, noise-alpha (scipy) identical outside the excusable set;
    excusable pixels <= 1e-5 of all pixels; the committed file is what the generator builds"""
    _in_child("""
        tot, exc = G.check_restatement()
        assert tot > 900000 and exc <= 1e-5 * tot, (tot, exc)
        g = np.load(G.OUT)
        new = G.build()
        assert sorted(g.files) == sorted(new)
        for k in new:
            a, b = np.asarray(new[k]), g[k]
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a, b), k
    """)
    assert os.path.getsize(os.path.join(GOLD, "stylize.npz")) < 1000 * 1000


def test_fixture_case_set():
    """every opcode alone on 64x48 and 96x80 with C = 1 and 3 (hue: 3), the three input kinds, superpixels on 50x70, its grid,
    update and p_replace corners, the constant image, the empty-centre case, three chains mixing the three opcodes; the numpy
    restatement reproduces the stored images without scipy"""
    G = _helper()
    cases = G.load_cases(np.load(os.path.join(GOLD, "stylize.npz")))
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    by_op = {op: [c for c in cases if not c["chain"] and set(np.unique(c["opcode"])) == {op}] for op in (1, 2, 3)}
    for op, want in ((1, {(64, 48, 3), (96, 80, 3)}), (2, {(64, 48, 1), (64, 48, 3), (96, 80, 1), (96, 80, 3)}),
                     (3, {(64, 48, 1), (64, 48, 3), (96, 80, 1), (96, 80, 3), (50, 70, 1), (50, 70, 3)})):
        assert {(c["h"], c["w"], c["c"]) for c in by_op[op]} == want, op
        assert {c["kind"] for c in by_op[op]} >= {"random", "smooth", "grey3"}, op
    hue = np.concatenate([c["iarg"][:, 0, :2] for c in by_op[1]])
    assert {(-14, -20), (14, 20), (180, 255), (-180, -255)} <= {tuple(v) for v in hue.tolist()}
    na = np.concatenate([c["iarg"][:, 0] for c in by_op[2]])
    assert set(na[:, 0]) == {1, 2, 3} and set(na[:, 1]) == {0, 1} and set(na[:, 2]) == {0, 1, 2} and set(na[:, 3]) == {0, 1}
    assert na[:, 4:10].max() == 16 and na[:, 4:6].min() == 2
    sp_i = np.concatenate([c["iarg"][:, 0] for c in by_op[3]])
    sp_f = np.concatenate([c["farg"][:, 0] for c in by_op[3]])
    assert {(1, 1), (4, 5), (10, 20), (16, 16)} == {tuple(v) for v in sp_i[:, :2].tolist()}
    assert set(sp_i[:, 2]) == {0, 5} and sp_f[:, 0].min() == 0.0 and sp_f[:, 0].max() == 1.0 and np.any((sp_f[:, 0] > 0.2) & (sp_f[:, 0] < 0.8))
    for h, w in ((64, 48), (96, 80), (50, 70)):      # every grid on every shape it fits; 50x70 does not divide by any of them
        assert {tuple(c["iarg"][i, 0, :2]) for c in by_op[3] if (c["h"], c["w"]) == (h, w) for i in range(c["b"])} >= {(4, 5), (10, 20)}
    assert any(c["kind"] == "const" for c in by_op[3])
    empty = [c for c in by_op[3] if c["name"].endswith("_empty")]
    assert empty and all(c["empty"] > 0 for c in empty) and 0 in set(sp_i[:, 3])
    chains = [c for c in cases if c["chain"]]
    assert len(chains) == 3 and all(set(np.unique(c["opcode"])) == {1, 2, 3} for c in chains)
    assert len({tuple(c["opcode"][i]) for c in chains for i in range(c["b"])}) >= 6
    tot = exc = 0
    for c in cases:
        tot += c["u8"].size
        exc += len(c["exc"])
        if c["chain"] or np.all(np.isin(c["opcode"], G.INTEGER_OPS)):
            assert len(c["exc"]) == 0, c["name"]
    assert exc <= 1e-5 * tot
    for c in cases[::4] + chains:
        got, e = G.run_program(G.case_inputs(c), c["opcode"], c["iarg"], c["farg"], c["table"], c["seed_arr"], backend="numpy")
        assert np.array_equal(got, c["u8"]) and int(e.sum()) == len(c["exc"]), c["name"]


# ---------------------------------------------------------------------------------------------- hue by hand
def test_hue_saturation_by_hand():
    G = _helper()
    px = lambda *rgb: np.array(rgb, dtype=np.uint8).reshape(1, 1, 3)
    both = lambda img, dh, ds: (G.hue_numpy(img, dh, ds), G.hue_python(img, dh, ds))
    for got in both(px(255, 0, 0), 60, 0):
        assert got.reshape(3).tolist() == [0, 255, 0], "pure red turned by 60 (of 180) is pure green"
    for got in both(px(255, 0, 0), 120, 0):
        assert got.reshape(3).tolist() == [0, 0, 255]
    grey = np.arange(256, dtype=np.uint8)[:, None, None].repeat(3, axis=2)
    for dh, ds in ((0, 0), (37, 0), (-90, -255), (13, -20)):
        for got in both(grey, dh, ds):
            assert np.array_equal(got, grey), "grey with ds <= 0 is unchanged"
    img = np.random.default_rng(0).integers(0, 256, (40, 30, 3), dtype=np.uint8)
    for ds in (0, 20, -20):
        a, b = both(img, 0, ds)
        assert np.array_equal(a, b)
        for dh in (180, -180, 360):
            assert np.array_equal(G.hue_numpy(img, dh, ds), a) and np.array_equal(G.hue_python(img, dh, ds), a), "dh = +-180 is 0"
    # g < b under a red maximum: num is negative and rdiv has to floor.  (200, 10, 60): d = 190, num = -50,
    # rdiv(-1500, 190) = floor(-2810 / 380) = -8 (truncation would give -7), H = 172
    V, d = 200, 190
    assert (2 * 30 * -50 + d) // (2 * d) == -8
    S = (2 * 255 * d + V) // (2 * V)
    H2, F = 172, 172 % 30
    want = [V, (2 * V * (255 - S) + 255) // 510, (2 * V * (7650 - S * F) + 7650) // 15300]      # sector 5: (V, p, q)
    for got in both(px(200, 10, 60), 0, 0):
        assert got.reshape(3).tolist() == want
    assert G.hue_pixel_python(200, 10, 60, 8, 0)[0] == V and G.hue_pixel_python(200, 10, 60, 8, 0) != tuple(want)      # H' = 0: sector 0
    neg = img[(img[..., 0] >= img[..., 1]) & (img[..., 0] >= img[..., 2]) & (img[..., 1] < img[..., 2])]
    assert len(neg) > 50      # (the random image holds such pixels, and the two interpreters agreed on them above)
    # a round trip without a change keeps the maximum; H is rounded to 1/30 of a sector, so the middle channel moves by at
    # most d / 60 <= 4.25, plus half a level each for S's rounding (V / 510) and the final rounding
    a = G.hue_numpy(img, 0, 0)
    assert np.array_equal(a.max(-1), img.max(-1)) and np.abs(a - img.astype(np.int64)).max() <= 5


# ---------------------------------------------------------------------------------------------- helpers
def test_edge_weight_helpers():
    from pointcloududa_amd.utils import stylize as S
    G = _helper()
    ident = np.zeros((3, 3)); ident[1, 1] = 1.0
    for alpha in (0.5, 0.77, 1.0):
        wts = S.edge_detect_weights(alpha)
        assert np.array_equal(wts, G.edge(alpha))
        assert abs(((wts - (1 - alpha) * ident) / alpha).sum()) < 1e-12, "the effect matrix sums to 0"
        for direction in (0.0, 0.125, 0.3, 0.5, 0.81, 1.0):
            wts = S.directed_edge_weights(alpha, direction)
            eff = (wts - (1 - alpha) * ident) / alpha
            assert abs(eff.sum()) < 1e-12 and abs(eff[1, 1] + 1.0) < 1e-12 and np.all(np.delete(eff.ravel(), 4) >= 0)
            assert np.allclose(wts, G.directed_edge(alpha, direction), rtol=0, atol=1e-12)
            mirror = S.directed_edge_weights(alpha, direction + 0.5)
            assert np.allclose(mirror, wts[::-1, ::-1], rtol=0, atol=1e-12), "direction + 0.5 is the point mirror"
    up = S.directed_edge_weights(1.0, 0.0)
    assert up[0, 1] == up.ravel()[[0, 1, 2, 3, 5, 6, 7, 8]].max() and abs(up[2, 1]) < 1e-12, "direction 0 looks up"
    right = S.directed_edge_weights(1.0, 0.25)
    assert right[1, 2] == np.delete(right.ravel(), 4).max()


def test_simplex_grid_scalar_vectorised_range_and_seed():
    from pointcloududa_amd.utils import stylize as S
    G = _helper()
    seen = []
    for h2, w2, seed in ((2, 2, 1), (16, 16, 2 ** 63 + 5), (7, 5, 12345), (3, 16, 99), (16, 2, 7)):
        a, b = S.simplex_grid(h2, w2, seed), S.simplex_grid_scalar(h2, w2, seed)
        assert a.shape == (h2, w2) and a.dtype == np.float64 and np.array_equal(a, b)
        assert np.array_equal(a, G.simplex_grid(h2, w2, seed)), "the package's grid is the generator's"
        assert a.min() >= 0.0 and a.max() <= 1.0
        seen.append(a.ravel())
    assert not np.array_equal(S.simplex_grid(16, 16, 1), S.simplex_grid(16, 16, 2))
    big = np.concatenate([S.simplex_grid(16, 16, s).ravel() for s in range(200)])
    assert big.min() < 0.25 and big.max() > 0.75 and abs(big.mean() - 0.5) < 0.02 and big.std() > 0.1
    assert np.abs(big - 0.5).min() > 1e-9, "no mask value sits on 1/2 (a blend of two integers would sit on a rounding boundary)"


def test_superpixel_grid_and_threshold():
    from pointcloududa_amd.utils import stylize as S
    assert S.superpixel_grid(20, 256, 256) == (4, 5) and S.superpixel_grid(200, 256, 256) == (14, 14)
    assert S.superpixel_grid(100, 128, 512) == (5, 20) and S.superpixel_grid(1, 256, 256) == (1, 1)
    for n in range(1, 2000, 37):
        for h, w in ((256, 256), (50, 70), (16, 400), (3, 5)):
            gy, gx = S.superpixel_grid(n, h, w)
            assert 1 <= gy <= h and 1 <= gx <= w and gy * gx <= 256
    assert S.threshold(0.0) == 0 and S.threshold(1.0) == 2 ** 32 - 1 and S.threshold(0.5) == 2 ** 31


def test_package_encoders_match_the_generators():
    from pointcloududa_amd.utils import stylize as S
    G = _helper()
    rng = np.random.default_rng(3)
    for op in (G.HUE_SATURATION, G.NOISE_ALPHA, G.SUPERPIXELS):
        slots = G.corner_slots(op, rng) + [G.random_slot(op, rng) for _ in range(4)]
        want, got = G.Prog(len(slots), 1), S.StyleProgram.identity(len(slots), 1)
        for i, kw in enumerate(slots):
            want.put(i, 0, op, **kw)
            if op == G.HUE_SATURATION:
                got.set_hue_saturation(i, 0, kw["dh"], kw["ds"])
            elif op == G.NOISE_ALPHA:
                grids = [S.simplex_grid(h2, w2, kw["seed"] + k) for k, (h2, w2) in enumerate(kw["sizes"])]
                got.set_noise_alpha(i, 0, kw["weights"], grids, kw["upscale"], kw["aggregation"], kw["sigmoid"], kw["thresh"])
            else:
                got.set_superpixels(i, 0, kw["gy"], kw["gx"], kw["p"], kw["seed"], kw["iters"], kw.get("compactness", 10))
        for k in ("opcode", "iarg", "farg", "table", "seed"):
            assert np.array_equal(getattr(want, k), getattr(got, k)), (op, k)
        got.validate(64, 48, 3)
        ia = got.kernel_arrays(64, 48, 3)[1]
        if op == G.SUPERPIXELS:
            assert [int(v) for v in ia[:, 0, 4].view(np.uint32)] == [G.threshold(p) for p in got.farg[:, 0, 0]]
            assert np.all(got.iarg[:, 0, 4] == 0), "kernel_arrays works on a copy"
    assert [S.OP_NOP, S.OP_HUE_SATURATION, S.OP_NOISE_ALPHA_CONV3X3, S.OP_SUPERPIXELS] == [G.NOP, G.HUE_SATURATION, G.NOISE_ALPHA, G.SUPERPIXELS]
    p = S.StyleProgram.identity(2, 3)
    assert p.is_identity() and p.batch == 2 and p.slots == 3
    p.set_hue_saturation(1, 2, 3, 4)
    assert not p.is_identity()
    p.set_nop(1, 2)
    assert p.is_identity() and not p.iarg.any()


# ---------------------------------------------------------------------------------------------- validation
def test_programs_are_validated_on_the_host():
    from pointcloududa_amd.utils import stylize as S

    def good():
        p = S.StyleProgram.identity(2, 3)
        p.set_hue_saturation(0, 0, 14, 20)
        p.set_noise_alpha(0, 1, S.edge_detect_weights(0.7), [S.simplex_grid(4, 5, 1), S.simplex_grid(16, 2, 2)], 1, 2, True, 1.5)
        p.set_superpixels(0, 2, 4, 5, 0.5, 77)
        return p
    good().validate(64, 48, 3)
    good().validate()

    def bad(match, fn, *args):
        p = good()
        fn(p)
        with pytest.raises(ValueError, match=match):
            p.validate(*(args or (64, 48, 3)))
    bad("opcode", lambda p: setattr(p, "opcode", p.opcode.astype(np.int64)))
    bad("slots", lambda p: [setattr(p, k, np.concatenate([getattr(p, k)] * 3, axis=1)) for k in ("opcode", "iarg", "farg", "table", "seed")])
    bad("iarg", lambda p: setattr(p, "iarg", p.iarg[:, :, :4]))
    bad("farg", lambda p: setattr(p, "farg", p.farg.astype(np.float32)))
    bad("table", lambda p: setattr(p, "table", p.table[:, :, :256]))
    bad("seed", lambda p: setattr(p, "seed", p.seed.astype(np.int64)))
    bad("unknown opcode", lambda p: p.opcode.__setitem__((1, 0), 4))
    bad("unknown opcode", lambda p: p.opcode.__setitem__((1, 0), -1))
    bad("channels", lambda p: None, 64, 48, 5)
    bad("farg must be finite", lambda p: p.farg.__setitem__((0, 1, 3), np.nan))
    bad("table must be finite", lambda p: p.table.__setitem__((0, 1, 3), np.inf))
    bad("HUE_SATURATION takes 3 channels", lambda p: None, 64, 48, 1)
    bad("dh", lambda p: p.iarg.__setitem__((0, 0, 0), 181))
    bad("ds", lambda p: p.iarg.__setitem__((0, 0, 1), -256))
    bad("grid count", lambda p: p.iarg.__setitem__((0, 1, 0), 4))
    bad("grid count", lambda p: p.iarg.__setitem__((0, 1, 0), 0))
    bad("upscale", lambda p: p.iarg.__setitem__((0, 1, 1), 2))
    bad("aggregation", lambda p: p.iarg.__setitem__((0, 1, 2), 3))
    bad("sigmoid", lambda p: p.iarg.__setitem__((0, 1, 3), 2))
    bad("grid sides", lambda p: p.iarg.__setitem__((0, 1, 4), 1))
    bad("grid sides", lambda p: p.iarg.__setitem__((0, 1, 7), 17))
    bad("mask values", lambda p: p.table.__setitem__((0, 1, 0), 1.5))
    bad("mask values", lambda p: p.table.__setitem__((0, 1, 300), -0.1))
    bad("threshold", lambda p: p.farg.__setitem__((0, 1, 9), 1e6))
    bad("gy, gx", lambda p: p.iarg.__setitem__((0, 2, 0), 0))
    bad("gy, gx", lambda p: p.iarg.__setitem__((0, 2, 1), 49))
    bad("gy gx", lambda p: p.iarg.__setitem__((0, 2, slice(0, 2)), (17, 16)))
    bad("updates", lambda p: p.iarg.__setitem__((0, 2, 2), 11))
    bad("M2", lambda p: p.iarg.__setitem__((0, 2, 3), -1))
    bad("p_replace", lambda p: p.farg.__setitem__((0, 2, 0), 1.01))
    # a live grid side only: the third grid of a two-grid slot is not looked at
    p = good()
    p.iarg[0, 1, 8:10] = 0
    p.validate(64, 48, 3)
    with pytest.raises(ValueError, match="grids"):
        good().set_noise_alpha(0, 0, np.eye(3), [np.zeros((17, 16))])
    with pytest.raises(ValueError, match="grids"):
        good().set_noise_alpha(0, 0, np.eye(3), [])
    import torch
    with pytest.raises(TypeError, match="program is required"):
        S.stylize_aug(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(TypeError, match="uint8"):
        S.stylize_aug(torch.zeros((1, 8, 8, 3)), good())
    with pytest.raises(ValueError, match="batch of 1"):
        S.upload_style_program(good(), 1, 64, 48, 3, torch.device("cpu"))


# ---------------------------------------------------------------------------------------------- presets
def test_full_presets_statistics_and_ranges():
    """over many draws: how often each of the three entries occurs against the SomeOf expectation (a uniform count 0..5 of
    distinct entries out of N: E[count] / N = 2.5 / N per entry, halved behind sometimes(0.5)), the parameter ranges, and the
    stage structure; tolerance: four standard deviations of a binomial share, as tests/test_photometric.py"""
    from pointcloududa_amd.utils import stylize as S
    from pointcloududa_amd.utils.augment import GeoProgram, PhotoProgram, StyleProgram, sample_heavy_plan, sample_style_program
    b, rounds, h, w = 64, 40, 96, 80
    n = b * rounds
    tol = lambda q: 4 * np.sqrt(q * (1 - q) / n)
    for preset, block in (("heavy_full_device", 15), ("mscmrseg_aug2_full_device", 12)):
        rng = np.random.default_rng(5 + block)
        counts = np.zeros(4)
        photo_slots = geo_slots = 0
        hue, na_i, na_f, sp_i, sp_f = [], [], [], [], []
        for _ in range(rounds):
            plan = sample_heavy_plan(b, preset, rng, h, w)
            kinds = [type(st) for st in plan.stages]
            assert all(k1 is not k2 for k1, k2 in zip(kinds, kinds[1:])), "consecutive entries of one kind form one stage"
            for st in plan.stages:
                assert st.batch == b and not st.is_identity()
                if isinstance(st, StyleProgram):
                    st.validate(h, w, 3)
                    assert st.slots <= 3 and st.opcode.dtype == np.int32
                    for op in (1, 2, 3):
                        counts[op] += (st.opcode == op).sum()
                    hue.append(st.iarg[st.opcode == 1]); na_i.append(st.iarg[st.opcode == 2]); na_f.append(st.farg[st.opcode == 2])
                    sp_i.append(st.iarg[st.opcode == 3]); sp_f.append(st.farg[st.opcode == 3])
                    live = st.opcode == 2
                    assert np.all((st.table >= 0) & (st.table <= 1)) and not st.table[~live].any() and (not live.any() or st.table[live].any())
                elif isinstance(st, PhotoProgram):
                    photo_slots += int((st.opcode != 0).sum())
                else:
                    assert isinstance(st, GeoProgram)
                    geo_slots += int((st.opcode != 0).sum())
        q = 2.5 / block
        assert abs(counts[1] / n - q) < tol(q), ("hue", counts[1] / n, q)
        assert abs(counts[2] / n - q) < tol(q), ("noise-alpha", counts[2] / n, q)
        assert abs(counts[3] / n - q / 2) < tol(q / 2), ("superpixels", counts[3] / n, q / 2)
        assert min(counts[1:]) > 100, "the three new entries occur"
        # f7's nine entries: a Gaussian below sigma 0.125 is encoded as NOP (1/3 of the blurs, sigma U(0, 3))
        q9 = 9 * q - q / 3 * 0.125 / 3.0
        f, cs = 9.0 / block, np.arange(6.0)      # the count of f7's entries in a sample: hypergeometric in the SomeOf count
        var9 = f * f * cs.var() + np.mean(cs * f * (1 - f) * (block - cs) / (block - 1))
        assert abs(photo_slots / n - q9) < 4 * np.sqrt(var9 / n), (photo_slots / n, q9)
        hue, na_i, na_f, sp_i, sp_f = (np.concatenate(v) for v in (hue, na_i, na_f, sp_i, sp_f))
        assert hue[:, 1].min() == -20 and hue[:, 1].max() == 20 and hue[:, 0].min() == -14 and hue[:, 0].max() == 14
        assert np.array_equal(hue[:, 0], np.floor(hue[:, 1] * 180.0 / 255.0 + 0.5).astype(np.int32))
        assert set(na_i[:, 0]) == {1, 2, 3} and set(na_i[:, 1]) == {0, 1} and set(na_i[:, 2]) == {0, 1, 2} and set(na_i[:, 3]) == {1}
        live = np.repeat(np.arange(3)[None, :] < na_i[:, 0:1], 2, axis=1)
        sides = na_i[:, 4:10]
        assert sides[live].min() == 2 and sides[live].max() == 16 and not sides[~live].any()
        assert abs(na_f[:, 9].mean()) < 4 * 5 / np.sqrt(len(na_f)) and 4 < na_f[:, 9].std() < 6
        eff_centre = na_f[:, 4]      # (1 - a) + a * (-4 | -1): alpha in [0.5, 1] -> centre in [-4, 0]
        assert eff_centre.min() >= -4 - 1e-12 and eff_centre.max() <= 1e-12 and np.all(np.abs(na_f[:, :9].sum(1) - (1 - _alpha(na_f))) < 1e-9)
        assert sp_f[:, 0].min() < 0.05 and sp_f[:, 0].max() > 0.95 and np.all((sp_f[:, 0] >= 0) & (sp_f[:, 0] <= 1))
        assert np.all(sp_i[:, 2] == 5) and np.all(sp_i[:, 3] == 100) and np.all(sp_f[:, 1] == 10)
        segs = sp_i[:, 0] * sp_i[:, 1]
        assert segs.min() >= 15 and segs.max() <= 256 and segs.max() > 150
        # the stylize entries alone: three slots, the same ranges
        prog = sample_style_program(b, preset, np.random.default_rng(1), h, w)
        assert prog.slots == 3 and prog.batch == b and set(np.unique(prog.opcode)) == {0, 1, 2, 3}
        prog.validate(h, w, 3)
    with pytest.raises(ValueError, match="no stylize entry"):
        sample_style_program(4, "heavy_device", np.random.default_rng(1), h, w)


def _alpha(fa):
    """alpha of an edge kernel from its weights: the off-centre weights sum to alpha * 4 (EdgeDetect) or alpha (directed)"""
    off = fa[:, :9].sum(1) - fa[:, 4]
    centre = fa[:, 4]
    # EdgeDetect: centre = 1 - 5 a, off = 4 a; directed: centre = 1 - 2 a, off = a
    is_edge = np.abs((1 - centre) / 5 - off / 4) < 1e-9
    a = np.where(is_edge, off / 4, off)
    assert np.all((a >= 0.5 - 1e-9) & (a <= 1 + 1e-9)) and 0.3 < is_edge.mean() < 0.7
    return a


def test_old_presets_draw_what_they_drew_and_hold_no_style_program():
    """"heavy_device", "mscmrseg_aug2_device" and "mscmrseg_aug2_photometric" consume the generator exactly as before (their
    draws are followed by the same next value as a replay of the documented sequence) and never hold a StyleProgram"""
    from pointcloududa_amd.utils import geometric as Geo
    from pointcloududa_amd.utils import heavy as Hv
    from pointcloududa_amd.utils.augment import StyleProgram, sample_heavy_plan
    for preset in ("heavy_device", "mscmrseg_aug2_device"):
        for seed in range(20):
            rng = np.random.default_rng(seed)
            plan = sample_heavy_plan(16, preset, rng, 64, 48)
            assert not any(isinstance(st, StyleProgram) for st in plan.stages)
            twin = np.random.default_rng(seed)
            spec = Hv._PRESETS[preset]
            assert all(e == "block" or e[0] in "pg" for e in spec["outer"] + spec["block"])
            # the documented sequence: two orders, the count, the ranks, one sometimes per warp of the block, the outer
            # coins, then the geometric and the photometric parameters -- and nothing after them
            twin.permutation(len(spec["outer"])); twin.permutation(len(spec["block"]))
            twin.integers(0, 6, 16); twin.random((16, len(spec["block"])))
            for e in spec["block"]:
                if e[0] == "g":
                    twin.random(16)
            for e in spec["outer"]:
                if e != "block":
                    twin.random(16)
            Geo._draw_geo(16, twin, 64, 48); Hv._draw_photo(16, twin)
            assert rng.integers(0, 2 ** 62) == twin.integers(0, 2 ** 62), (preset, seed)


def test_heavy_still_raises_and_the_presets_are_known():
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import stylize as S
    rng = np.random.default_rng(0)
    for fn in (lambda: A.sample_heavy_plan(2, "heavy", rng, 32, 32), lambda: A.sample_style_program(2, "heavy", rng, 32, 32),
               lambda: A.sample_geo_program(2, "heavy", rng, 32, 32), lambda: A.sample_program(2, "heavy", rng),
               lambda: A.AugmentedBatches(iter(()), "cpu", None, rng, num_classes=5, heavy_preset="heavy")):
        with pytest.raises(NotImplementedError) as e:
            fn()
        assert str(e.value) == A.HEAVY_MESSAGE
    with pytest.raises(ValueError, match="unknown heavy preset"):
        A.sample_heavy_plan(2, "heavy_fuller_device", rng, 32, 32)
    assert (A.HEAVY_FULL_PRESET, A.AUG2_FULL_PRESET) == ("heavy_full_device", "mscmrseg_aug2_full_device")
    assert A.StyleProgram is S.StyleProgram and A.stylize_aug is S.stylize_aug and A.simplex_grid is S.simplex_grid
    # PhotoProgram keeps its twelve opcodes
    from pointcloududa_amd.utils import photometric as P
    assert len(P.OP_NAMES) == 12 and (P.MAX_SLOTS, P.IARGS, P.FARGS) == (8, 4, 16)


def test_heavy_aug_refuses_an_unknown_stage():
    import torch
    from pointcloududa_amd.utils.augment import HeavyPlan, heavy_aug
    with pytest.raises(TypeError, match="a stage is"):
        heavy_aug(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), None, HeavyPlan(1, [object()]))


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_declares_what_the_binding_binds():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p}
    for name, ret in (("pcuda_stylize", "int"), ("pcuda_stylize_workspace_size", "size_t")):
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (s.strip() for s in m.group(2).split(","))]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
    m = re.search(r"int pcuda_stylize\(([^;]*)\);", hdr)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "in", "out", "b", "h", "w", "c", "slots", "opcode", "iarg", "farg", "table", "seed", "workspace", "workspace_bytes", "s"]
    from pointcloududa_amd.utils import stylize as S
    for n in S.OP_NAMES:
        assert re.search(r"#define PCUDA_STYLE_%s %d\b" % (n, getattr(S, "OP_" + n)), hdr), n
    assert len(re.findall(r"#define PCUDA_STYLE_\w+ \d+", hdr)) == len(S.OP_NAMES)
    assert int(re.search(r"#define\s+PCUDA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _lib.PCUDA_ABI_VERSION
    assert "stylize.hip" in open(os.path.join(CSRC, "Makefile")).read()
    src = open(os.path.join(CSRC, "stylize.hip")).read()
    assert "kIArgs = %d" % S.IARGS in src and "kFArgs = %d" % S.FARGS in src and "kTable = 3 * kGrid" in src and "kGrid = %d" % S.GRID_VALUES in src
