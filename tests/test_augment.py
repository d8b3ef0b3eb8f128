"""CPU checks of the device-side light augmentation (pointcloududa_amd/utils/augment.py, csrc/augment.hip): the scipy
restatement (scripts/make_augment_golden.py) against plain numpy, the fixture regenerating exactly, the parameter sampler,
the matrix composition against the helper's independent one, the C entry points rejecting bad arguments without a GPU, and
the new kernels' ISA.

scipy runs in a child process (see tests/test_eval_metrics.py)."""
import ctypes
import importlib.util
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import GOLD, ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
GEN = os.path.join(ROOT, "scripts", "make_augment_golden.py")
needs_scipy = pytest.mark.skipif(importlib.util.find_spec("scipy") is None, reason="the restatement needs scipy")


def _helper():
    spec = importlib.util.spec_from_file_location("make_augment_golden", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _in_child(body):
    code = "import sys, numpy as np\nsys.path.insert(0, %r)\nimport make_augment_golden as G\n" % os.path.dirname(GEN)
    r = subprocess.run([sys.executable, "-c", code + textwrap.dedent(body)], capture_output=True, text=True,
                       env=dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1"), timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


@needs_scipy
def test_scipy_restatement_matches_plain_numpy():
    """rounded values equal except at excusable pixels (one grey level there), excusable pixels <= 1e-5 of all pixels"""
    _in_child("""
        tot, exc, worst = G.check_restatement()
        assert tot > 2000000 and exc <= 1e-5 * tot and worst <= 1e-9, (tot, exc, worst)
    """)


@needs_scipy
def test_fixture_regenerates_exactly():
    _in_child("""
        g = np.load(G.OUT)
        new = G.build()
        assert sorted(g.files) == sorted(new)
        for k in new:
            a, b = np.asarray(new[k]), g[k]
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a, b), k
    """)
    assert os.path.getsize(os.path.join(GOLD, "augment.npz")) < 1024 * 1024


def test_fixture_case_set():
    """the case set the GPU tests run: orders 0 and 1, C = 1 and 3, 256x256 and a non-square odd size, B = 5, all six
    operation orders, the heavy corners, one case almost out of the frame; excusable pixels <= 1e-5 of all pixels"""
    G = _helper()
    cs = G.load_cases(np.load(os.path.join(GOLD, "augment.npz")))
    assert {c["op_order"] for c in cs} >= {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    assert {c["c"] for c in cs} == {1, 3} and any(c["b"] == 5 for c in cs)
    assert any((c["h"], c["w"]) == (256, 256) for c in cs) and any((c["h"], c["w"]) == (200, 231) for c in cs)
    on = [(int(o), bool(a)) for c in cs for o, a in zip(c["params"]["order"], c["params"]["affine_on"])]
    assert (0, True) in on and (1, True) in on
    assert any(np.any(np.abs(c["params"]["rotate"]) == 45) and np.any(np.abs(c["params"]["translate_x"]) == 0.2) for c in cs)
    oof = [c for c in cs if c["name"] == "out_of_frame"][0]
    assert np.all(oof["area"][:2] <= 50) and np.all(oof["area"][:2] > 0) and not oof["verts"][:2].any() and oof["verts"][2].any()
    pixels = sum(c["u8"].size + c["mask"].size for c in cs)
    assert sum(len(c["exc_img"]) + len(c["exc_mask"]) for c in cs) <= 1e-5 * pixels
    for c in cs:
        if "verts" in c:
            assert len(c["exc_mask"]) == 0
        x, q, mn, mx, lab = G.case_inputs(c)
        assert x.dtype == np.float32 and q.dtype == np.uint8 and q.min() == 0 and q.max() >= 254 and lab.max() == c["k"] - 1


# ---------------------------------------------------------------------------------------------- sample_params
@pytest.mark.parametrize("preset,p", [("mmwhs_light", (0.2, 0.2, 0.3)), ("mscmrseg_simple", (0.3, 0.3, 0.45))])
def test_sample_params_ranges_and_probabilities(preset, p):
    from pointcloududa_amd.utils.augment import sample_params
    n = 20000
    prm = sample_params(n, preset, np.random.default_rng(5))
    prm.validate()
    for got, want in zip((prm.flip_lr, prm.flip_ud, prm.affine_on), p):
        assert got.dtype == bool and abs(got.mean() - want) <= 4 * np.sqrt(want * (1 - want) / n), (got.mean(), want)
    for a, (lo, hi) in ((prm.scale_x, (0.8, 1.2)), (prm.scale_y, (0.8, 1.2)), (prm.translate_x, (-0.1, 0.05)),
                        (prm.translate_y, (-0.1, 0.1)), (prm.rotate, (-10, 10)), (prm.shear, (-12, 12))):
        assert a.dtype == np.float64 and lo <= a.min() < lo + 0.01 * (hi - lo) and hi - 0.01 * (hi - lo) < a.max() <= hi
    assert set(np.unique(prm.order)) == {0, 1} and prm.cval.min() == 0 and prm.cval.max() == 255
    assert abs(prm.order.mean() - 0.5) <= 4 * 0.5 / np.sqrt(n)


def test_sample_params_is_deterministic_and_draws_one_order_per_batch():
    from pointcloududa_amd.utils.augment import AugmentParams, sample_params
    a = sample_params(7, "mmwhs_light", np.random.default_rng(11))
    b = sample_params(7, "mmwhs_light", np.random.default_rng(11))
    for k in AugmentParams.__dataclass_fields__:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.batch == 7 and isinstance(a.op_order, tuple) and sorted(a.op_order) == [0, 1, 2]
    rng = np.random.default_rng(12)
    seen = {sample_params(3, "mscmrseg_simple", rng).op_order for _ in range(200)}
    assert len(seen) == 6                                      # every order occurs, one per batch
    with pytest.raises(NotImplementedError, match="heavy pipeline .* is out of scope"):
        sample_params(4, "heavy", np.random.default_rng(0))
    with pytest.raises(ValueError, match="preset"):
        sample_params(4, "medium", np.random.default_rng(0))


# ---------------------------------------------------------------------------------------------- inverse_matrices
def _params(case):
    from pointcloududa_amd.utils.augment import AugmentParams
    return AugmentParams(op_order=case["op_order"], **{k: np.asarray(v) for k, v in case["params"].items()})


def test_inverse_matrices_match_the_helpers_composition():
    from pointcloududa_amd.utils.augment import inverse_matrices
    G = _helper()
    cs = G.load_cases(np.load(os.path.join(GOLD, "augment.npz")))
    assert len(cs) >= 12
    for c in cs:
        got = inverse_matrices(_params(c), c["h"], c["w"])
        assert got.dtype == np.float64 and got.shape == (c["b"], 2, 3)
        assert np.abs(got - c["inv"]).max() <= 1e-12 * max(c["h"], c["w"]), c["name"]


def test_identity_and_flip_matrices_are_exact():
    from pointcloududa_amd.utils.augment import AugmentParams, inverse_matrices, kernel_params
    h, w = 200, 231
    ident = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    p = AugmentParams.identity(3)
    assert p.is_identity() and np.array_equal(inverse_matrices(p, h, w), np.stack([ident] * 3))
    # affine switched off: its parameters do not matter, and order / cval do not reach the kernel
    p.rotate[:] = 30.0; p.scale_x[:] = 0.5; p.order[:] = 1; p.cval[:] = 99
    inv, order, cval = kernel_params(p, h, w)
    assert np.array_equal(inv, np.stack([ident] * 3)) and not order.any() and not cval.any()
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    for lr in (False, True):
        for ud in (False, True):
            for oo in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
                p = AugmentParams.identity(1)
                p.flip_lr[:] = lr; p.flip_ud[:] = ud; p.op_order = oo
                m = inverse_matrices(p, h, w)[0]
                sx, sy = m[0, 0] * xs + m[0, 1] * ys + m[0, 2], m[1, 0] * xs + m[1, 1] * ys + m[1, 2]
                assert np.array_equal(sx, w - 1 - xs if lr else xs) and np.array_equal(sy, h - 1 - ys if ud else ys)


def test_parameters_are_validated_on_the_host():
    from pointcloududa_amd.utils.augment import AugmentParams, inverse_matrices, light_aug, simple_aug
    for field, bad, what in (("order", 2, "order"), ("order", -1, "order"), ("cval", 256, "cval"), ("cval", -1, "cval")):
        p = AugmentParams.identity(2)
        p.affine_on[:] = True
        getattr(p, field)[1] = bad
        with pytest.raises(ValueError, match=what):
            inverse_matrices(p, 8, 8)
    p = AugmentParams.identity(2)
    p.affine_on[:] = True
    p.scale_x[1] = 0.0
    with pytest.raises(ValueError, match="singular"):
        inverse_matrices(p, 8, 8)
    p = AugmentParams.identity(2)
    p.op_order = (0, 0, 2)
    with pytest.raises(ValueError, match="op_order"):
        inverse_matrices(p, 8, 8)
    import torch
    with pytest.raises(TypeError, match="params is required"):
        light_aug(torch.zeros(1, 4, 4, 1, dtype=torch.uint8))
    with pytest.raises(TypeError, match="params is required"):
        simple_aug(torch.zeros(4, 4, 1, dtype=torch.uint8), None)


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_points_reject_bad_arguments_without_a_gpu():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)                                  # never dereferenced: rejected before any launch
    ws = lib.pcuda_minmax_workspace_size()
    assert ws >= 8
    assert lib.pcuda_minmax(None, 16, fake, fake, ws, None) == -1 and b"minmax" in lib.pcuda_last_error()
    assert lib.pcuda_minmax(fake, 16, None, fake, ws, None) == -1
    assert lib.pcuda_minmax(fake, 16, fake, None, ws, None) == -1
    assert lib.pcuda_minmax(fake, 0, fake, fake, ws, None) == -1
    assert lib.pcuda_minmax(fake, 16, fake, fake, ws - 1, None) == -4 and b"workspace" in lib.pcuda_last_error()

    def call(img=fake, u8=0, lab=fake, b=2, h=16, w=16, c=3, crop=0, k=5, inv=fake, order=fake, cval=fake, rescale=0, mm=None,
             out=fake, onehot=fake, full=None, labels=None, out_u8=None):
        return lib.pcuda_augment_assemble(img, u8, lab, b, h, w, c, crop, k, inv, order, cval, rescale, mm, out, onehot, full,
                                          labels, out_u8, None)
    for kw, what in ((dict(img=None), b"null"), (dict(inv=None), b"null"), (dict(order=None), b"null"), (dict(cval=None), b"null"),
                     (dict(out=None, onehot=None), b"null"), (dict(lab=None), b"null"), (dict(lab=None, onehot=None, full=fake), b"null"),
                     (dict(crop=18), b"crop larger"), (dict(h=16, w=8, crop=10), b"crop larger"), (dict(k=1), b"num_classes"),
                     (dict(b=0), b"dims"), (dict(c=0), b"dims"), (dict(rescale=3), b"rescale"), (dict(rescale=1), b"min-max"),
                     (dict(rescale=1, u8=1, mm=fake), b"min-max"), (dict(rescale=2), b"uint8"), (dict(out_u8=fake), b"uint8")):
        assert call(**kw) == -1, kw
        assert what in lib.pcuda_last_error(), (kw, lib.pcuda_last_error())


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_augment_kernels_keep_load_addresses_alive():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=augment.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "augment.s"]
    assert len(rows) >= 6, "expected the min-max kernels and every augment_assemble instantiation in the assembly"
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
