"""CPU checks of the evaluation metrics: the scipy restatement (scripts/make_eval_golden.py) against brute force, the
fixture regenerating exactly, the C entry points rejecting bad arguments without a GPU, and the new kernels' ISA.

scipy runs in a child process: its import brings a BLAS with a thread pool of its own into the interpreter, which the
torch CPU tests that share this pytest process must not compete with."""
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
GEN = os.path.join(ROOT, "scripts", "make_eval_golden.py")
needs_scipy = pytest.mark.skipif(importlib.util.find_spec("scipy") is None, reason="the restatement needs scipy")


def _in_child(body):
    """run ``body`` in a fresh interpreter with scripts/make_eval_golden.py imported as G; it fails by raising"""
    code = "import sys, numpy as np\nsys.path.insert(0, %r)\nimport make_eval_golden as G\n" % os.path.dirname(GEN)
    r = subprocess.run([sys.executable, "-c", code + textwrap.dedent(body)], capture_output=True, text=True,
                       env=dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1"), timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


@needs_scipy
@pytest.mark.parametrize("conn", [1, 2, 3])
@pytest.mark.parametrize("spacing", [None, "aniso"])
def test_scipy_restatement_matches_brute_force(conn, spacing):
    _in_child("""
        rng = np.random.default_rng(3)
        n = 0
        for shape in ((5, 7, 6), (9, 8), (4, 5, 9)):
            for cls in ([1, 2], [2, 3]):
                p = rng.integers(0, 4, shape)
                t = G.blobs(shape, int(rng.integers(100)), [1, 2, 3], n=5)
                if %(conn)d > p.ndim:
                    continue
                sp = None if %(aniso)r is None else (2.5, 1.25, 0.7)[-p.ndim:]
                a, b = G.surface(p, t, cls, sp, %(conn)d), G.surface_brute(p, t, cls, sp, %(conn)d)
                assert np.allclose(a, b, rtol=1e-12, atol=0, equal_nan=True), (a, b)
                n += 1
        assert n >= 4
    """ % dict(conn=conn, aniso=spacing))


@needs_scipy
def test_scipy_largest_components_matches_flood_fill():
    _in_child("""
        for name, m in G.ccl_cases():
            assert np.array_equal(G.largest_components(m), G.largest_components_brute(m)), name
    """)


@needs_scipy
def test_scipy_matches_brute_force_on_the_edge_shapes():
    """the cases of tests/eval_shapes.py (what tests/test_eval_edges_gpu.py holds the kernels to): the brute force there
    is the reference, and here scipy agrees with it within the same bounds, without a GPU"""
    _in_child("""
        sys.path.insert(0, %r)
        import eval_shapes as S

        def same(a, b, unit, what):
            assert np.array_equal(a[:, [0, 4, 5, 6, 7]], b[:, [0, 4, 5, 6, 7]]), what
            ok = b[:, 7] == 0
            assert np.isnan(a[~ok, 1:4]).all() and np.isnan(b[~ok, 1:4]).all(), what
            if unit:
                assert np.array_equal(a[ok, 1], b[ok, 1]), (what, a, b)
            assert np.allclose(a[ok, 1:4], b[ok, 1:4], rtol=1e-12, atol=0), (what, a, b)

        n = 0
        for shape in S.DEGENERATE_SHAPES:
            p, t = S.degenerate_pair(G.blobs, shape)
            assert all((p == c).any() or (t == c).any() for c in (1, 2, 3)), shape
            for conn in range(1, len(shape) + 1):
                for sp in (None, S.ANISO[-len(shape):]):
                    same(G.surface(p, t, S.DEGENERATE_CLASSES, sp, conn),
                         G.surface_brute(p, t, S.DEGENERATE_CLASSES, sp, conn), sp is None, (shape, conn, sp))
                    n += 1
        assert n == 50
        for name, p, t, cls, sp, conn in S.surface_cases():
            same(G.surface(p, t, cls, sp, conn), G.surface_brute(p, t, cls, sp, conn), sp is None, name)
        far = G.surface_brute(*S.far_voxels((2, 3, 1030)), [1])[0]
        assert far[1] == far[2] == far[3] == np.sqrt(1.0 + 4.0 + 1029.0 ** 2)
        for name, m, kept in S.ccl_cases():
            ref = G.largest_components_brute(m)
            assert np.array_equal(G.largest_components(m), ref), name
            assert kept is None or int(np.count_nonzero(ref)) == kept, (name, int(np.count_nonzero(ref)))
            assert np.array_equal(G.largest_components(m.astype(bool)), G.largest_components_brute(m.astype(bool))), name
        assert S.snake(129, 131).sum() == 8579 and S.two_snakes().sum() == 1222 and S.rings(63).size == 3969
    """ % os.path.join(ROOT, "tests"))


def test_closed_forms_in_the_fixture():
    g = np.load(os.path.join(GOLD, "eval_metrics.npz"))
    names = {str(g[k]): k[:-5] for k in g.files if k.endswith("_name") and k.startswith("s")}
    cube = g[names["offset_cubes"] + "_out"][0]
    assert cube[1] == np.sqrt(8.0) and cube[7] == 0            # cubes offset by (2, 2, 0)
    single = g[names["single_voxels"] + "_out"][0]
    assert single[1] == single[2] == single[3] == np.sqrt(2 ** 2 + 4 ** 2 + 5 ** 2)
    assert g[names["blobs_12x64x64_empty"] + "_out"][1][7] == 3 and g[names["blobs_12x64x64_empty"] + "_out"][1][0] == 0
    ties = {str(g[k]): k[:-5] for k in g.files if k.endswith("_name") and k.startswith("c")}
    t = g[ties["tie_2d"] + "_out"]
    assert t[1, 1] == 1 and t[4, 5] == 0                        # equal sizes: the raster-first component wins


@needs_scipy
def test_fixture_regenerates_exactly():
    _in_child("""
        g = np.load(G.OUT)
        new = G.build()
        assert sorted(g.files) == sorted(new)
        for k in new:
            a, b = np.asarray(new[k]), g[k]
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
    """)
    assert os.path.getsize(os.path.join(GOLD, "eval_metrics.npz")) < 256 * 1024


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)                                  # never dereferenced: rejected before any launch
    cls = (ctypes.c_int * 9)(*range(1, 10))
    out = ctypes.c_void_p(8192)
    ws_ok = lib.pcuda_surface_metrics_workspace_size(3, 4, 5, 6, 2, None)
    assert ws_ok > 0
    assert lib.pcuda_surface_metrics_workspace_size(4, 4, 5, 6, 2, None) == 0
    assert lib.pcuda_surface_metrics_workspace_size(3, 4, 5, 6, 9, None) == 0
    sp = (ctypes.c_double * 3)(2.0, 1.0, 1.0)
    assert lib.pcuda_surface_metrics_workspace_size(3, 4, 5, 6, 2, sp) > ws_ok      # fp64 fields with spacing

    def call(ndim=3, z=4, h=5, w=6, ncls=2, conn=1, spacing=None, ws=ws_ok):
        return lib.pcuda_surface_metrics(fake, fake, 0, ndim, z, h, w, cls, ncls, conn, spacing, out, fake, ws, None)
    for kw, what in ((dict(ndim=1), b"ndim"), (dict(ndim=4), b"ndim"), (dict(ndim=2), b"dims"), (dict(conn=0), b"connectivity"),
                     (dict(conn=4), b"connectivity"), (dict(ndim=2, z=1, conn=3), b"connectivity"), (dict(ncls=9), b"classes"),
                     (dict(ncls=0), b"classes"), (dict(w=16385), b"dims"), (dict(z=16384, h=16384, w=16), b"2^31"),
                     (dict(spacing=(ctypes.c_double * 3)(1.0, 0.0, 1.0)), b"spacing")):
        assert call(**kw) == -1, kw
        assert what in lib.pcuda_last_error(), (kw, lib.pcuda_last_error())
    assert call(ws=ws_ok - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(spacing=sp) == -4                                 # the fp64 layout needs the larger workspace
    lw = lib.pcuda_largest_components_workspace_size(3, 4, 5, 6)
    assert lw >= 2 * 4 * 120 and lib.pcuda_largest_components_workspace_size(5, 4, 5, 6) == 0
    assert lib.pcuda_largest_components(fake, 0, 3, 4, 5, 6, 5, fake, fake, lw - 1, None) == -4
    assert lib.pcuda_largest_components(fake, 0, 2, 2, 5, 6, 5, fake, fake, lw, None) == -1
    assert lib.pcuda_largest_components(None, 0, 3, 4, 5, 6, 5, fake, fake, lw, None) == -1


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_eval_metric_kernels_keep_load_addresses_alive():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=eval_metrics.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "eval_metrics.s"]
    assert len(rows) >= 20, "expected every eval_metrics kernel instantiation in the assembly"
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
