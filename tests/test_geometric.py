"""CPU checks of the device-side geometric augmentation (pointcloududa_amd/utils/geometric.py, csrc/geometric.hip; DESIGN.md
section 6, f8): the plain-numpy restatement (scripts/make_geometric_golden.py) reproducing the fixture, the scipy restatement
agreeing where scipy is installed, the fixture's case set and excusable share, the package's encoders against the generator's
and against f6's matrices, validation, the samplers, the C declaration against the binding, and the new kernel's ISA.  No GPU
and no library load.

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
GEN = os.path.join(ROOT, "scripts", "make_geometric_golden.py")
needs_scipy = pytest.mark.skipif(importlib.util.find_spec("scipy") is None, reason="the restatement needs scipy")


def _helper():
    sys.path.insert(0, os.path.dirname(GEN))
    try:
        spec = importlib.util.spec_from_file_location("make_geometric_golden", GEN)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(os.path.dirname(GEN))
    return m


def _in_child(body):
    code = "import sys, numpy as np\nsys.path.insert(0, %r)\nimport make_geometric_golden as G\n" % os.path.dirname(GEN)
    r = subprocess.run([sys.executable, "-c", code + textwrap.dedent(body)], capture_output=True, text=True,
                       env=dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1"), timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


def _cases():
    G = _helper()
    return G, G.load_cases(np.load(os.path.join(GOLD, "geometric.npz")))


# ---------------------------------------------------------------------------------------------- the fixture
def test_numpy_restatement_reproduces_every_fixture_case():
    """bit for bit outside the excusable pixels, images and labels; the stored inputs are the seeded ones"""
    G, cs = _cases()
    for c in cs:
        x, lab = G.case_inputs(c)
        assert np.array_equal(x, c["images"]) and np.array_equal(lab, c["labels"]), c["name"]
        out, lab_out, exc, exc_lab, earlier = G.run_program(c["images"], c["labels"], c["opcode"], c["iarg"], c["farg"], c["seed_arr"],
                                                            backend="numpy")
        e, el = G.exc_masks(c)
        assert np.array_equal(out[~e], c["u8"][~e]) and np.array_equal(lab_out[~el], c["lab"][~el]), c["name"]
        assert not (exc & ~e).any() and not (exc_lab & ~el).any(), c["name"]
        if c["chain"]:
            assert earlier == 0 and not e.any() and not el.any(), c["name"]


@needs_scipy
def test_scipy_restatement_agrees_and_the_fixture_regenerates_exactly():
    """build() asserts that scipy and numpy agree on every non-excusable pixel, that excusable pixels are <= 1e-5 of all
    pixels and that no slot of a chain has one"""
    _in_child("""
        g = np.load(G.OUT)
        new = G.build()
        assert sorted(g.files) == sorted(new)
        for k in new:
            a, b = np.asarray(new[k]), g[k]
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a, b), k
    """)
    assert os.path.getsize(os.path.join(GOLD, "geometric.npz")) < 1000 * 1000


def test_fixture_case_set_and_excusable_share():
    """64x48 and 96x80 with C = 1 and 3; every mode x order for HOMOGRAPHY; the affine near the ends of its ranges; a crop and
    a pad; a perspective close to the validity limit; elastic r = 0, 1, 4; piecewise G = 2, 3, 4; three chains of 4-5 slots;
    labels in every case; excusable pixels <= 1e-5 of all pixels"""
    G, cs = _cases()
    single = [c for c in cs if not c["chain"]]
    assert {(c["h"], c["w"], c["c"]) for c in cs} == {(64, 48, 1), (64, 48, 3), (96, 80, 1), (96, 80, 3)}
    for op in (G.HOMOGRAPHY, G.ELASTIC, G.PIECEWISE):
        got = {(c["h"], c["w"], c["c"]) for c in single if set(np.unique(c["opcode"])) == {op}}
        assert got == {(64, 48, 1), (64, 48, 3), (96, 80, 1), (96, 80, 3)}, (op, got)
    hom = np.concatenate([c["iarg"][c["opcode"] == G.HOMOGRAPHY] for c in single])
    assert {(int(o), int(m)) for o, m in hom[:, :2]} == {(o, m) for o in (0, 1) for m in range(5)}
    assert hom[:, 2].min() == 0 and hom[:, 2].max() == 255
    el_i = np.concatenate([c["iarg"][c["opcode"] == G.ELASTIC] for c in single])
    el_f = np.concatenate([c["farg"][c["opcode"] == G.ELASTIC] for c in single])
    assert set(el_i[:, 3]) == {0, 1, 4} and el_f[:, 0].min() < 0.56 and 3.44 < np.sort(el_f[:, 0])[-5]
    assert set(np.concatenate([c["iarg"][c["opcode"] == G.PIECEWISE] for c in single])[:, 3]) == {2, 3, 4}
    for c in cs:
        assert np.any(c["labels"] > 0) and np.any(c["lab"] > 0) and not np.array_equal(c["labels"], c["lab"]), c["name"]
    # the named homographies: the flips, a crop and a pad, a perspective close to the limit, the affine's corners
    by = {c["name"]: c for c in cs}
    f = by["affine_flips_64x48_c1"]["farg"][:, 0, :9]
    assert np.array_equal(f[3], G.flip_lr(48).ravel()) and np.array_equal(f[4], G.flip_ud(64).ravel())
    rot = np.degrees(np.arctan2(-f[:3, 3], f[:3, 0]))           # the inverse rotates by -rotate (shear and scale bend it a little)
    assert rot.max() > 30 and rot.min() < -30
    f = by["crop_pad_96x80_c3"]["farg"][:, 0, :9]
    assert f[0, 0] < 1 and f[0, 4] < 1 and f[1, 0] > 1 and f[1, 4] > 1, "a crop zooms in, a pad zooms out"
    f = by["perspective_64x48_c1"]["farg"][:, 0, :9]
    d = f[:, 6:7] * np.array([0.0, 47.0, 47.0, 0.0]) + f[:, 7:8] * np.array([0.0, 0.0, 63.0, 63.0]) + f[:, 8:9]
    assert np.all(d > 0) and np.all(f[0, [0, 4]] < 0.2), "the quad of the first sample is a tenth of the image"
    chains = [c for c in cs if c["chain"]]
    assert len(chains) == 3 and all(c["opcode"].shape[1] in (4, 5) and np.all(c["opcode"] != 0) for c in chains)
    assert set(np.concatenate([c["opcode"].ravel() for c in chains])) == {1, 2, 3}
    assert len({tuple(row) for c in chains for row in c["opcode"]}) >= 5
    g = np.load(os.path.join(GOLD, "geometric.npz"))
    tot, exc = (int(v) for v in g["counts"])
    assert tot == sum(c["u8"].size + c["lab"].size for c in cs) and tot > 1500000
    assert exc == sum(len(c["exc"]) + len(c["exc_lab"]) for c in cs) and exc <= 1e-5 * tot
    assert all(len(c["exc"]) == 0 and len(c["exc_lab"]) == 0 for c in chains)


def test_index_folding_matches_numpy_pad():
    G = _helper()
    for n in (2, 3, 7):
        base = np.arange(n)
        idx = np.arange(-3 * n - 1, 4 * n + 2)
        for mode, pad in ((G.EDGE, "edge"), (G.REFLECT, "reflect"), (G.SYMMETRIC, "symmetric"), (G.WRAP, "wrap")):
            want = np.pad(base, (3 * n + 1, 3 * n + 2), mode=pad)
            got, inside = G.fold_index(idx, n, mode)
            assert np.array_equal(got, want) and inside.all(), (n, pad)
        got, inside = G.fold_index(idx, n, G.CONSTANT)
        assert np.array_equal(inside, (idx >= 0) & (idx < n)) and got.min() == 0 and got.max() == n - 1


# ---------------------------------------------------------------------------------------------- the package's encoders
def _run_np(G, prog, x, lab):
    return G.run_program(x, lab, prog.opcode, prog.iarg, prog.farg, prog.seed, backend="numpy")[:2]


def test_package_encoders_match_the_generators():
    from pointcloududa_amd.utils import geometric as P
    G = _helper()
    assert [P.OP_NOP, P.OP_HOMOGRAPHY, P.OP_ELASTIC, P.OP_PIECEWISE] == [G.NOP, G.HOMOGRAPHY, G.ELASTIC, G.PIECEWISE]
    assert [P.MODE_CONSTANT, P.MODE_EDGE, P.MODE_REFLECT, P.MODE_SYMMETRIC, P.MODE_WRAP] == list(range(5))
    assert (P.MAX_SLOTS, P.IARGS, P.FARGS) == (8, 4, 32)
    rng = np.random.default_rng(8)
    h, w = 96, 80
    want, got = G.Prog(8, 1), P.GeoProgram.identity(8, 1)
    want.homography(0, 0, G.flip_lr(w), 0); got.set_flip_lr(0, 0, w)
    want.homography(1, 0, G.flip_ud(h), 0); got.set_flip_ud(1, 0, h)
    kw = dict(scale_x=1.17, scale_y=0.83, translate_x=-0.19, translate_y=0.2, rotate=-44.0, shear=15.5)
    want.homography(2, 0, G.affine_inverse(h, w, **kw), 0, 3, 200); got.set_affine(2, 0, h, w, order=0, mode=3, cval=200, **kw)
    want.homography(3, 0, G.crop_and_pad(h, w, -5, 8, 10, -4), 1, 2, 31); got.set_crop_and_pad(3, 0, h, w, -5, 8, 10, -4, 2, 31)
    jit = rng.normal(0, 0.08, (4, 2))
    want.homography(4, 0, G.perspective(h, w, jit), 1, 0, 0); got.set_perspective(4, 0, h, w, jit)
    want.elastic(5, 0, 3.3, 0.25, 2 ** 64 - 3, 1, 0, 0); got.set_elastic(5, 0, 3.3, 0.25, 2 ** 64 - 3)
    want.elastic(6, 0, 9.0, 1.1, 77, 0, 4, 9); got.set_elastic(6, 0, 9.0, 1.1, 77, order=0, mode=4, cval=9)
    dx, dy = rng.normal(0, 3, (4, 4)), rng.normal(0, 3, (4, 4))
    want.piecewise(7, 0, h, w, dx, dy, 1, 0, 0); got.set_piecewise(7, 0, h, w, dx, dy)
    got.validate(h, w)
    for f in ("opcode", "iarg", "seed"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), f
    assert np.array_equal(got.farg[[0, 1, 3, 4, 5, 6, 7]], want.farg[[0, 1, 3, 4, 5, 6, 7]])
    assert np.allclose(got.farg[2], want.farg[2], rtol=0, atol=1e-9)      # (f6's composition inverts once more: last bits)
    assert got.iarg[6, 0, 3] == 4 and got.iarg[5, 0, 3] == 1 and got.farg[5, 0, 31] == 0.25
    op, ia, fa, sd = got.kernel_arrays(h, w)
    assert sd.dtype == np.int64 and sd[5, 0] == -3 and op is got.opcode


def test_encoders_hold_their_identities():
    """a flip as a homography is an exact permutation; an affine with mode 0 equals f6's inverse_matrices; zero crop / pad,
    zero jitter and alpha = 0 are the identity"""
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import geometric as P
    G = _helper()
    rng = np.random.default_rng(2)
    b, h, w, c = 7, 37, 52, 3
    x = rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)
    lab = rng.integers(0, 5, (b, h, w)).astype(np.int64)
    prog = P.GeoProgram.identity(b, 1)
    prog.set_flip_lr(0, 0, w)
    prog.set_flip_ud(1, 0, h)
    prog.set_crop_and_pad(2, 0, h, w, 0, 0, 0, 0, P.MODE_WRAP, 99)
    prog.set_perspective(3, 0, h, w, np.zeros((4, 2)))
    prog.set_elastic(4, 0, 0.0, 0.25, 12345, mode=P.MODE_REFLECT)
    prog.set_piecewise(5, 0, h, w, np.zeros((4, 4)), np.zeros((4, 4)))
    prog.set_affine(6, 0, h, w)
    prog.validate(h, w)
    assert not prog.is_identity()
    out, lab_out = _run_np(G, prog, x, lab)
    assert np.array_equal(out[0], x[0, :, ::-1]) and np.array_equal(lab_out[0], lab[0, :, ::-1])
    assert np.array_equal(out[1], x[1, ::-1]) and np.array_equal(lab_out[1], lab[1, ::-1])
    for i in range(2, 7):
        assert np.array_equal(out[i], x[i]) and np.array_equal(lab_out[i], lab[i]), i
    assert np.array_equal(prog.farg[2, 0, :9], np.eye(3).ravel()) and np.array_equal(prog.farg[6, 0, :9], np.eye(3).ravel())
    # f6's matrices, bit for bit, for sampled light AND heavy parameters
    params = A.sample_params(16, "mscmrseg_simple", np.random.default_rng(4))
    params.affine_on[:] = True
    params.flip_lr[:] = False
    params.flip_ud[:] = False
    params.rotate[:8] = np.linspace(-45, 45, 8)
    params.translate_x[:8] = 0.2
    inv = A.inverse_matrices(params, h, w)
    prog = P.GeoProgram.identity(16, 1)
    for i in range(16):
        prog.set_affine(i, 0, h, w, params.scale_x[i], params.scale_y[i], params.translate_x[i], params.translate_y[i], params.rotate[i],
                        params.shear[i], int(params.order[i]), P.MODE_CONSTANT, int(params.cval[i]))
    assert np.array_equal(prog.farg[:, 0, :6].reshape(16, 2, 3), inv)
    assert np.array_equal(prog.farg[:, 0, 6:9], np.tile([0.0, 0.0, 1.0], (16, 1)))
    assert np.array_equal(prog.iarg[:, 0, 0], params.order) and np.array_equal(prog.iarg[:, 0, 2], params.cval)
    # ... and the restatement of such a slot is f6's restatement of the same warp (scripts/make_augment_golden.py)
    sys.path.insert(0, os.path.dirname(GEN))
    try:
        import make_augment_golden as F6
    finally:
        sys.path.remove(os.path.dirname(GEN))
    xs = rng.integers(0, 256, (16, h, w, 1), dtype=np.uint8)
    out, _ = _run_np(G, prog, xs, np.zeros((16, h, w), dtype=np.int64))
    for i in range(16):
        v = F6.warp_np(xs[i, :, :, 0], inv[i], int(params.order[i]), int(params.cval[i]))
        assert np.array_equal(out[i, :, :, 0], F6.to_u8(v)), i
    # crop / pad: the pad's border shows cval, the crop's centre is the input's centre
    prog = P.GeoProgram.identity(2, 1)
    prog.set_crop_and_pad(0, 0, h, w, 4, 5, 4, 5, P.MODE_CONSTANT, 255)
    prog.set_crop_and_pad(1, 0, h, w, -2, -3, -2, -3)
    flat = np.full((2, h, w, 1), 100, dtype=np.uint8)
    out, _ = _run_np(G, prog, flat, np.zeros((2, h, w), dtype=np.int64))
    assert out[0, 0, 0, 0] == 255 and out[0, h // 2, w // 2, 0] == 100 and np.all(out[1] == 100)
    # the perspective's corners land on the jittered quad
    jit = np.array([[0.1, 0.2], [0.05, 0.1], [0.2, 0.0], [0.0, 0.15]])
    m = P.perspective_matrix(jit, h, w)
    for (xo, yo), (xs_, ys_) in zip(((0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)),
                                    ((0.1 * w, 0.2 * h), (w - 1 - 0.05 * w, 0.1 * h), (w - 1 - 0.2 * w, h - 1.0), (0.0, h - 1 - 0.15 * h))):
        p = m @ np.array([xo, yo, 1.0])
        assert np.allclose(p[:2] / p[2], (xs_, ys_), atol=1e-9)


def test_programs_are_validated_on_the_host():
    import torch
    from pointcloududa_amd.utils import geometric as P
    from pointcloududa_amd.utils import heavy as Hv
    h, w = 40, 30

    def one(setter, *args, **kw):
        p = P.GeoProgram.identity(2, 2)
        getattr(p, setter)(1, 1, *args, **kw)
        return p
    assert P.GeoProgram.identity(3, 0).is_identity() and P.GeoProgram.identity(3).slots == 1
    P.GeoProgram.identity(3, 8).validate(h, w)
    good = one("set_affine", h, w, rotate=30.0, mode=4, cval=255)
    good.validate(); good.validate(h, w)
    bad = []
    p = one("set_flip_lr", w); p.opcode[0, 0] = 4; bad.append((p, "unknown opcode"))
    p = one("set_flip_lr", w); p.opcode[0, 0] = -1; bad.append((p, "unknown opcode"))
    p = one("set_flip_lr", w); p.iarg[1, 1, 0] = 2; bad.append((p, "order"))
    p = one("set_flip_lr", w); p.iarg[1, 1, 0] = -1; bad.append((p, "order"))
    bad += [(one("set_affine", h, w, mode=m), "mode") for m in (-1, 5)]
    bad += [(one("set_affine", h, w, cval=v), "cval") for v in (-1, 256)]
    p = one("set_flip_lr", w); p.farg[1, 1, 2] = np.nan; bad.append((p, "finite"))
    p = one("set_flip_lr", w); p.farg[1, 1, 30] = np.inf; bad.append((p, "finite"))
    bad.append((one("set_homography", np.zeros((3, 3))), "singular"))
    bad.append((one("set_homography", [[1, 2, 0], [2, 4, 0], [0, 0, 1]]), "singular"))
    bad.append((one("set_crop_and_pad", h, w, 0, -15, 0, -15), "singular"))                   # the whole width cropped away
    bad.append((one("set_homography", [[1, 0, 0], [0, 1, 0], [-0.05, 0, 1]]), "denominator"))      # d < 0 at x = W - 1
    bad.append((one("set_homography", [[1, 0, 0], [0, 1, 0], [0, 0, -1]]), "denominator"))
    bad.append((one("set_elastic", 2.0, 1.2, 1), "radius"))                                   # int(4.8 + 0.5) = 5
    bad.append((one("set_elastic", -1.0, 0.25, 1), "alpha"))
    p = one("set_elastic", 2.0, 0.5, 1); p.farg[1, 1, 2] *= 1.5; bad.append((p, "weights"))
    p = one("set_elastic", 2.0, 0.5, 1); p.iarg[1, 1, 3] = -1; bad.append((p, "radius"))
    p = one("set_piecewise", h, w, np.zeros((4, 4)), np.zeros((4, 4))); p.iarg[1, 1, 3] = 5; bad.append((p, "G must"))
    p = one("set_piecewise", h, w, np.zeros((2, 2)), np.zeros((2, 2))); p.iarg[1, 1, 3] = 1; bad.append((p, "G must"))
    p = P.GeoProgram.identity(2, 9); bad.append((p, "slots"))
    p = P.GeoProgram.identity(2, 2); p.iarg = p.iarg.astype(np.int64); bad.append((p, "iarg"))
    p = P.GeoProgram.identity(2, 2); p.farg = p.farg[:, :, :16]; bad.append((p, "farg"))
    p = P.GeoProgram.identity(2, 2); p.seed = p.seed.astype(np.int64); bad.append((p, "seed"))
    p = P.GeoProgram.identity(2, 2); p.opcode = p.opcode.astype(np.int64); bad.append((p, "opcode"))
    for p, what in bad:
        with pytest.raises(ValueError, match=what):
            p.validate(h, w)
    for hw in ((1, 30), (40, 1)):
        with pytest.raises(ValueError, match="at least 2"):
            good.validate(*hw)
    with pytest.raises(ValueError, match=r"\[G,G\]"):
        one("set_piecewise", h, w, np.zeros((4, 3)), np.zeros((4, 4)))
    with pytest.raises(TypeError, match="program is required"):
        P.geometric_aug(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), None)
    with pytest.raises(TypeError, match="uint8"):
        P.geometric_aug(torch.zeros(1, 4, 4, 3), None, P.GeoProgram.identity(1))
    with pytest.raises(TypeError, match="plan is required"):
        Hv.heavy_aug(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), None)
    with pytest.raises(ValueError, match="batch"):
        P.upload_geo_program(P.GeoProgram.identity(2), 3, 8, 8, torch.device("cpu"))
    with pytest.raises(ValueError, match="batch"):
        Hv.heavy_aug(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), None, Hv.HeavyPlan(2))


# ---------------------------------------------------------------------------------------------- the samplers
def _homography_kind(f, h, w):
    if np.array_equal(f[:9], [-1, 0, w - 1, 0, 1, 0, 0, 0, 1]):
        return "fliplr"
    if np.array_equal(f[:9], [1, 0, 0, 0, -1, h - 1, 0, 0, 1]):
        return "flipud"
    if f[6] != 0 or f[7] != 0:
        return "perspective"
    if f[1] == 0 and f[3] == 0:
        return "crop_and_pad"
    return "affine"


def test_sample_geo_program_stays_in_range_over_1000_draws():
    from pointcloududa_amd.utils import geometric as P
    from pointcloududa_amd.utils import heavy as Hv
    h, w = 256, 224
    rng = np.random.default_rng(5)
    seen, orders = {}, set()
    crop_modes, aff_modes, aff_orders = set(), set(), set()
    for _ in range(1000):
        prog = Hv.sample_geo_program(4, "heavy_device", rng, h, w)
        prog.validate(h, w)
        assert prog.opcode.shape == (4, 7) and prog.farg.shape == (4, 7, 32) and prog.seed.dtype == np.uint64
        for i in range(4):
            kinds = []
            live = prog.opcode[i] != 0
            assert not live[np.argmin(live):].any() or live.all(), "active slots are packed to the front"
            for s in np.nonzero(live)[0]:
                op, ia, f = prog.opcode[i, s], prog.iarg[i, s], prog.farg[i, s]
                if op == P.OP_ELASTIC:
                    kind = "elastic"
                    assert 0.5 <= f[0] <= 3.5 and ia[3] == 1 and f[31] == 0.25 and tuple(ia[:3]) == (1, 0, 0)
                    assert np.array_equal(f[1:3], P.gaussian_weights(0.25)) and prog.seed[i, s] != 0
                elif op == P.OP_PIECEWISE:
                    kind = "piecewise"
                    gx, gy = P.control_grid(4, h, w)
                    dx, dy = f[:16].reshape(4, 4) - gx[None, :], f[16:].reshape(4, 4) - gy[:, None]
                    assert ia[3] == 4 and np.abs(dx).max() < 6 * 0.05 * w and np.abs(dy).max() < 6 * 0.05 * h and np.abs(dx).max() > 0
                else:
                    kind = _homography_kind(f, h, w)
                    if kind == "crop_and_pad":
                        assert ia[0] == 1 and 0 <= ia[1] <= 4 and 0 <= ia[2] <= 255
                        crop_modes.add(int(ia[1]))
                        # W + l + r and l back from the matrix: signed pixels inside (-0.05, 0.1) of the size
                        for a, t, size in ((f[0], f[2], w), (f[4], f[5], h)):
                            tot, first = a * size - size, 0.5 * a - 0.5 - t
                            lo, hi = np.floor(-0.05 * size + 0.5), np.floor(0.1 * size + 0.5)
                            assert abs(tot - round(tot)) < 1e-9 and abs(first - round(first)) < 1e-9
                            assert lo <= round(first) <= hi and lo <= round(tot) - round(first) <= hi
                    elif kind == "affine":
                        aff_modes.add(int(ia[1])); aff_orders.add(int(ia[0]))
                        m = np.linalg.inv(np.vstack([f[:6].reshape(2, 3), [0, 0, 1]]))      # forward: R . Sh . S about the centre
                        sx, sy = np.hypot(m[0, 0], m[1, 0]), np.linalg.det(m[:2, :2]) / np.hypot(m[0, 0], m[1, 0])
                        assert 0.8 - 1e-9 <= sx <= 1.2 + 1e-9 and 0.8 - 1e-9 <= sy <= 1.2 + 1e-9
                        assert abs(np.degrees(np.arctan2(m[1, 0], m[0, 0]))) <= 45 + 1e-9
                        cx, cy = (w - 1) / 2, (h - 1) / 2
                        tx, ty = m[:2] @ np.array([cx, cy, 1.0]) - (cx, cy)
                        assert abs(tx) <= 0.2 * w + 1e-6 and abs(ty) <= 0.2 * h + 1e-6
                    elif kind == "perspective":
                        assert tuple(ia[:3]) == (1, 0, 0)
                        m = f[:9].reshape(3, 3)
                        for xo, yo in ((0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)):
                            p = m @ np.array([xo, yo, 1.0])
                            q = p[:2] / p[2]
                            assert p[2] > 0 and abs(q[0] - xo) <= 0.45 * w + 1e-6 and abs(q[1] - yo) <= 0.45 * h + 1e-6
                    else:
                        assert ia[0] == 0
                kinds.append(kind)
                seen[kind] = seen.get(kind, 0) + 1
            assert len(set(kinds)) == len(kinds), "an entry is applied once"
            orders.add(tuple(kinds))
    assert set(seen) == set(P.GEO_ENTRY_NAMES), seen
    n = 4000
    tol = lambda q: 5 * np.sqrt(q * (1 - q) / n)
    warp_p = 0.5 * 2.5 / 12                        # a uniform count 0..5 of twelve entries, behind sometimes(0.5)
    for kind, want in (("fliplr", 0.5), ("flipud", 0.2), ("crop_and_pad", 0.5), ("affine", 0.5), ("elastic", warp_p),
                       ("piecewise", warp_p), ("perspective", warp_p)):
        assert abs(seen[kind] / n - want) <= tol(want), (kind, seen[kind] / n, want)
    assert crop_modes == set(range(5)) and aff_modes == set(range(5)) and aff_orders == {0, 1}
    assert len(orders) > 100
    # the aug2 preset: one slot, sometimes(CropAndPad)
    cnt = 0
    for _ in range(200):
        prog = Hv.sample_geo_program(8, "mscmrseg_aug2_device", rng, h, w)
        prog.validate(h, w)
        assert prog.opcode.shape == (8, 1) and set(np.unique(prog.opcode)) <= {0, 1}
        cnt += int(prog.opcode.sum())
        for i in np.nonzero(prog.opcode[:, 0])[0]:
            assert _homography_kind(prog.farg[i, 0], h, w) in ("crop_and_pad",) or np.array_equal(prog.farg[i, 0, :9], np.eye(3).ravel())
    assert abs(cnt / 1600 - 0.5) < 5 * 0.5 / 40


def test_sample_heavy_plan_stays_in_range_over_1000_draws():
    from pointcloududa_amd.utils import geometric as P
    from pointcloududa_amd.utils import heavy as Hv
    from pointcloududa_amd.utils import photometric as F7
    h, w = 128, 160
    rng = np.random.default_rng(6)
    geo_ops, photo_ops, nstages, block_counts = set(), set(), set(), []
    for it in range(1000):
        preset = ("heavy_device", "mscmrseg_aug2_device")[it % 4 == 3]
        plan = Hv.sample_heavy_plan(4, preset, rng, h, w)
        assert plan.batch == 4
        nstages.add(len(plan.stages))
        photo_slots = np.zeros(4, dtype=int)
        warps = np.zeros(4, dtype=int)
        for a, b in zip(plan.stages, plan.stages[1:]):
            assert type(a) is not type(b), "consecutive entries of one kind share a program"
        for st in plan.stages:
            # no stage carries an unused slot (a Gaussian blur with sigma < 0.125 is a NOP inside the slot it was drawn for)
            assert st.batch == 4 and 1 <= st.slots <= 8 and ((st.opcode[:, -1] != 0).any() or isinstance(st, F7.PhotoProgram))
            if isinstance(st, P.GeoProgram):
                st.validate(h, w)
                geo_ops |= set(np.unique(st.opcode))
                warps += np.isin(st.opcode, (P.OP_ELASTIC, P.OP_PIECEWISE)).sum(1)
                warps += ((st.opcode == P.OP_HOMOGRAPHY) & ((st.farg[:, :, 6] != 0) | (st.farg[:, :, 7] != 0))).sum(1)
                if preset == "mscmrseg_aug2_device":
                    assert st.slots == 1 and set(np.unique(st.opcode)) <= {0, 1}
            else:
                assert isinstance(st, F7.PhotoProgram)
                st.validate(3)
                photo_ops |= set(np.unique(st.opcode))
                # (a Gaussian with sigma < 0.125 is encoded as NOP inside its slot: count the packed prefix instead)
                photo_slots += np.array([np.max(np.nonzero(row)[0]) + 1 if row.any() else 0 for row in st.opcode])
        assert np.all(photo_slots + warps <= 5), "SomeOf draws at most five entries"
        block_counts += list(photo_slots + warps)
        if preset == "mscmrseg_aug2_device":
            assert len(plan.stages) <= 2
    assert geo_ops == {0, 1, 2, 3} and photo_ops == set(range(12))
    assert max(nstages) >= 5 and min(nstages) <= 1 and max(block_counts) == 5
    a = Hv.sample_heavy_plan(9, "heavy_device", np.random.default_rng(11), h, w)
    b = Hv.sample_heavy_plan(9, "heavy_device", np.random.default_rng(11), h, w)
    assert len(a.stages) == len(b.stages)
    for x, y in zip(a.stages, b.stages):
        for k in ("opcode", "iarg", "farg", "seed"):
            assert np.array_equal(getattr(x, k), getattr(y, k)), k
    assert Hv.HeavyPlan(3).is_identity() and not a.is_identity()


def test_heavy_still_raises_and_presets_are_checked():
    from pointcloududa_amd.utils import augment as A
    rng = np.random.default_rng(0)
    assert A.sample_geo_program.__module__.endswith("utils.heavy") and A.HEAVY_DEVICE_PRESET == "heavy_device"
    for fn in (lambda: A.sample_geo_program(4, "heavy", rng, 64, 64), lambda: A.sample_heavy_plan(4, "heavy", rng, 64, 64),
               lambda: A.sample_params(4, "heavy", rng), lambda: A.sample_program(4, "heavy", rng)):
        with pytest.raises(NotImplementedError, match="heavy pipeline .* is out of scope"):
            fn()
    for kw in (dict(preset="heavy"), dict(preset=None, heavy_preset="heavy"), dict(preset="mmwhs_light", photometric_preset="heavy")):
        with pytest.raises(NotImplementedError, match="out of scope"):
            A.AugmentedBatches(iter(()), None, kw.pop("preset"), rng, **kw)
    with pytest.raises(ValueError, match="preset"):
        A.sample_geo_program(4, "mscmrseg_simple", rng, 64, 64)
    with pytest.raises(ValueError, match="preset"):
        A.sample_heavy_plan(4, "mscmrseg_aug2_photometric", rng, 64, 64)
    with pytest.raises(ValueError, match="heavy preset"):
        A.AugmentedBatches(iter(()), None, None, rng, rescale="div255", heavy_preset="aug2")
    with pytest.raises(ValueError, match="must be None"):
        A.AugmentedBatches(iter(()), None, "mscmrseg_simple", rng, rescale="div255", heavy_preset="heavy_device")
    with pytest.raises(ValueError, match="must be None"):
        A.AugmentedBatches(iter(()), None, None, rng, rescale="div255", heavy_preset="heavy_device",
                           photometric_preset="mscmrseg_aug2_photometric")
    with pytest.raises(ValueError, match="preset"):
        A.AugmentedBatches(iter(()), None, None, rng, rescale="div255")                    # None only with a heavy preset
    with pytest.raises(TypeError, match="uint8"):
        A.AugmentedBatches(iter(()), None, None, rng, heavy_preset="heavy_device")         # the default rescale is min-max


# ---------------------------------------------------------------------------------------------- C ABI, ISA
def test_header_declares_what_the_binding_binds():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p}
    for name, ret in (("pcuda_geometric", "int"), ("pcuda_geometric_workspace_size", "size_t")):
        assert name in _lib.EXPORTED_SYMBOLS
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (s.strip() for s in m.group(2).split(","))]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
    m = re.search(r"int pcuda_geometric\(([^;]*)\);", hdr)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "in", "out", "labels_in", "labels_out", "b", "h", "w", "c", "slots", "opcode", "iarg", "farg", "seed", "workspace",
        "workspace_bytes", "s"]
    from pointcloududa_amd.utils import geometric as P
    for n in P.OP_NAMES:
        assert re.search(r"#define PCUDA_GEO_%s %d\b" % (n, P.OP_NAMES.index(n)), hdr), n
    for n in P.MODE_NAMES:
        assert re.search(r"#define PCUDA_GEO_%s %d\b" % (n, P.MODE_NAMES.index(n)), hdr), n
    assert "geometric.hip" in open(os.path.join(CSRC, "Makefile")).read()
    from pointcloududa_amd import kernels as K
    assert callable(K.geometric)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_geometric_kernel_keeps_load_addresses_alive():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=geometric.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "geometric.s"]
    assert len(rows) >= 1, "expected the geometric kernel in the assembly"
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
    text = open(os.path.join(CSRC, "build", "isa", "geometric.s")).read()
    assert "v_div_scale_f64" in text, "the homography divides in float64"
    src = open(os.path.join(CSRC, "geometric.hip")).read()
    assert not re.search(r"\basm\b", src), "no inline assembly beyond PCUDA_KEEP"
