"""CPU checks of the extended evaluation metrics (hd95, assd): the references of tests/eval_percentile_ref.py agree with
each other on every case the GPU tests run, the new entry points are declared and reject bad arguments without a GPU,
and the evaluate scripts' extended result lists follow their conventions.

scipy runs in a child process, as in tests/test_eval_metrics.py."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import eval_percentile_ref as R
from conftest import ROOT

needs_scipy = pytest.mark.skipif(importlib.util.find_spec("scipy") is None, reason="the restatement needs scipy")
E_BADARG, E_WORKSPACE = -1, -4               # include/pcuda_hip.h


@needs_scipy
def test_scipy_brute_force_and_numpy_percentile_agree_on_every_case():
    """G.sd (scipy), the all-pairs brute force and np.percentile of their distances: bit for bit at unit spacing, within
    1e-12 relative with spacing; hd95_ref / assd_ref are the same numbers"""
    code = """
        import sys, numpy as np
        sys.path.insert(0, %r)
        import eval_percentile_ref as R
        G = R.G
        n = 0
        for name, pred, gt, cls, sp, conn in R.cases():
            brute = R.case_sets(name)
            scipy_sets = R.class_sets(pred, gt, cls, sp, conn, sd=G.sd)
            for c, b, s in zip(cls, brute, scipy_sets):
                assert b[2:] == s[2:], (name, c)
                if b[4]:
                    continue
                for d_b, d_s in zip(b[:2], s[:2]):
                    if sp is None:
                        assert np.array_equal(d_b, d_s), (name, c)
                    else:
                        assert np.allclose(d_b, d_s, rtol=1e-12, atol=0), (name, c)
                for pooled in (np.hstack(b[:2]), np.hstack(s[:2])):
                    for q in R.QS:
                        mine, ref = R.percentile_linear(pooled, q), float(np.percentile(pooled, q))
                        assert mine == ref, (name, c, q, mine, ref)            # the restatement: bit for bit
                a, r = pred == c, gt == c
                for q in R.QS:
                    ref = R.hd95_ref(a, r, sp, conn, q)
                    assert ref == float(np.percentile(np.hstack(s[:2]), q))
                    got = R.ext_columns([b], q)[0, 0]
                    assert got == ref if sp is None else abs(got - ref) <= 1e-12 * ref, (name, c, q, got, ref)
                ref = R.assd_ref(a, r, sp, conn)
                got = R.ext_columns([b], 95.0)[0, 1]
                assert abs(got - ref) <= 1e-12 * ref, (name, c, got, ref)
                n += 1
        assert n >= 150, n
    """ % os.path.join(ROOT, "tests")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True,
                       env=dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1"), timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


def test_the_cases_are_what_their_names_say():
    """n = 2, n = 21 and n = 101 with t = 0, the straddle's ranks, and hd95 apart from hd"""
    def pooled(name):
        (ab, ba, na, nb, flags), = R.case_sets(name)[:1]
        assert flags == 0 and na + nb == ab.size + ba.size
        return np.sort(np.hstack((ab, ba)))
    assert pooled("far_voxels").tolist() == [np.sqrt(float(R.FAR_KEY))] * 2
    for name, n in (("n21", 21), ("n21_aniso", 21), ("n101", 101)):
        s = pooled(name)
        lo, hi, t = R.ranks(s.size, 95.0)
        assert s.size == n and t == 0.0 and lo == (n - 1) * 95 // 100 and hi == lo + 1
        assert R.percentile_linear(s, 95.0) == s[lo] and s[lo] < s[-1]
    for name, far in (("straddle", R.FAR_KEY), ("straddle_long", 5 + 5000 ** 2)):
        s = pooled(name)
        lo, hi, t = R.ranks(s.size, 95.0)
        assert (s.size, lo, hi, t) == (11, 9, 10, 0.5)
        assert (s ** 2).round().tolist() == [0.0] * 8 + [1.0, 1.0, float(far)]
        assert R.percentile_linear(s, 95.0) == s[10] - (s[10] - 1.0) * 0.5
    assert 5 + 5000 ** 2 >= 1 << 24 > R.FAR_KEY
    s = pooled("straddle_aniso")
    assert s[9] == 0.7 and s[10] > 700.0
    s = pooled("full_vs_voxel")
    assert abs(R.percentile_linear(s, 95.0) - 13.601) < 1e-3 and abs(s[-1] - 15.843) < 1e-3
    big = R.case_sets("big_8x96x96")
    assert all(f == 0 and na + nb > 2000 for _, _, na, nb, f in big)      # keys over many histogram workgroups


def test_new_symbols_are_exported_and_declared():
    from pointcloududa_amd import _lib
    header = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    for sym in ("pcuda_surface_metrics_ext_workspace_size", "pcuda_surface_metrics_ext"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\(" % sym, header), sym
        assert hasattr(_lib.lib(), sym)
    assert _lib.PCUDA_ABI_VERSION == 5 and _lib.lib().pcuda_version() == 5
    assert re.search(r"#define\s+PCUDA_ABI_VERSION\s+5\b", header)


def test_ext_entry_points_reject_bad_arguments_without_a_gpu():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)                                  # never dereferenced: rejected before any launch
    cls = (ctypes.c_int * 9)(*range(1, 10))
    out = ctypes.c_void_p(8192)
    size = lib.pcuda_surface_metrics_ext_workspace_size
    ws_ok = size(3, 4, 5, 6, 2, None)
    assert ws_ok > lib.pcuda_surface_metrics_workspace_size(3, 4, 5, 6, 2, None) > 0
    for bad in ((4, 4, 5, 6, 2), (1, 1, 5, 6, 2), (2, 2, 5, 6, 2), (3, 0, 5, 6, 2), (3, 4, 5, 16385, 2), (3, 16384, 16384, 16, 2),
                (3, 4, 5, 6, 9), (3, 4, 5, 6, 0)):
        assert size(*bad, None) == 0, bad
    assert size(2, 1, 5, 6, 2, None) > lib.pcuda_surface_metrics_workspace_size(2, 1, 5, 6, 2, None)
    sp = (ctypes.c_double * 3)(2.0, 1.0, 1.0)
    ws_sp = size(3, 4, 5, 6, 2, sp)
    assert ws_sp > ws_ok                                          # fp64 fields and keys with spacing
    assert size(3, 4, 5, 6, 2, (ctypes.c_double * 3)(1.0, 1.0, 1.0)) == ws_ok

    def call(ndim=3, z=4, h=5, w=6, ncls=2, conn=1, spacing=None, q=95.0, ws=ws_ok, pred=fake):
        return lib.pcuda_surface_metrics_ext(pred, fake, 0, ndim, z, h, w, cls, ncls, conn, spacing, q, out, fake, ws, None)
    for kw, what in ((dict(q=-1.0), b"percentile"), (dict(q=100.5), b"percentile"), (dict(q=float("nan")), b"percentile"),
                     (dict(q=float("inf")), b"percentile"), (dict(q=-1e-300), b"percentile"),
                     (dict(conn=0), b"connectivity"), (dict(conn=4), b"connectivity"),
                     (dict(ndim=2, z=1, conn=3), b"connectivity"), (dict(ncls=9), b"classes"), (dict(ncls=0), b"classes"),
                     (dict(spacing=(ctypes.c_double * 3)(1.0, 0.0, 1.0)), b"spacing"),
                     (dict(spacing=(ctypes.c_double * 3)(1.0, float("nan"), 1.0)), b"spacing"),
                     (dict(spacing=(ctypes.c_double * 3)(-1.0, 1.0, 1.0)), b"spacing"), (dict(ndim=4), b"ndim"),
                     (dict(ndim=2), b"dims"), (dict(w=16385), b"dims"), (dict(pred=None), b"null")):
        assert call(**kw) == E_BADARG, kw
        assert what in lib.pcuda_last_error(), (kw, lib.pcuda_last_error())
    assert call(ws=ws_ok - 1) == E_WORKSPACE and b"workspace" in lib.pcuda_last_error()
    assert call(spacing=sp) == E_WORKSPACE and call(spacing=sp, ws=ws_sp - 1) == E_WORKSPACE
    assert call(q=0.0, ws=ws_ok - 1) == E_WORKSPACE and call(q=100.0, ws=ws_ok - 1) == E_WORKSPACE     # the ends are valid


def _rows():
    nan = float("nan")
    #        dice hd   asd  asd' |A| |B| |AB| flags hd95 assd nbA nbB
    return [[0.5, 4.0, 1.5, 2.5, 10, 10, 5, 0, 3.0, 2.0, 6, 6],
            [0.0, nan, nan, nan, 0, 7, 0, 1, nan, nan, 0, 5],
            [0.25, 9.0, 3.0, 1.0, 8, 8, 2, 0, 7.0, 2.0, 4, 4],
            [0.0, nan, nan, nan, 3, 0, 0, 2, nan, nan, 3, 0]]


def test_metrics_from_rows_ext_follows_each_script():
    from pointcloududa_amd import evaluate_mmwhs as EW
    from pointcloududa_amd import evaluate_mscmrseg as EM
    rows = _rows()
    assert EW.CLASSES == [1, 2, 3, 4] and EM.CLASSES == [500, 600, 200]
    # MM-WHS: dice always, -1 for what is not asked for or what medpy would raise for; one row per class, in order
    assert EW.metrics_from_rows_ext(rows) == [0.5, 4.0, 1.5, 3.0, 2.0, 0.0, -1, -1, -1, -1, 0.25, 9.0, 3.0, 7.0, 2.0,
                                              0.0, -1, -1, -1, -1]
    assert EW.metrics_from_rows_ext(rows, ifhd=False) == [0.5, -1, 1.5, -1, 2.0, 0.0, -1, -1, -1, -1, 0.25, -1, 3.0, -1, 2.0,
                                                          0.0, -1, -1, -1, -1]
    assert EW.metrics_from_rows_ext(rows, ifasd=False)[:5] == [0.5, 4.0, -1, 3.0, -1]
    assert EW.metrics_from_rows_ext(rows, False, False) == [0.5, -1, -1, -1, -1, 0.0, -1, -1, -1, -1, 0.25, -1, -1, -1, -1,
                                                            0.0, -1, -1, -1, -1]
    # MS-CMRSeg: an empty class is five times -1 when hd or asd is asked for, and keeps its dice otherwise
    three = rows[:3]
    assert EM.metrics_from_rows_ext(three) == [0.5, 4.0, 1.5, 3.0, 2.0, -1, -1, -1, -1, -1, 0.25, 9.0, 3.0, 7.0, 2.0]
    assert EM.metrics_from_rows_ext(three, ifasd=False) == [0.5, 4.0, -1, 3.0, -1, -1, -1, -1, -1, -1, 0.25, 9.0, -1, 7.0, -1]
    assert EM.metrics_from_rows_ext(three, False, False) == [0.5, -1, -1, -1, -1, 0.0, -1, -1, -1, -1, 0.25, -1, -1, -1, -1]
    # the first three of every five are what the plain lists hold
    for mod, rs in ((EW, rows), (EM, three)):
        for ifhd in (True, False):
            for ifasd in (True, False):
                ext, plain = mod.metrics_from_rows_ext(rs, ifhd, ifasd), mod.metrics_from_rows([r[:8] for r in rs], ifhd, ifasd)
                assert [ext[5 * i + j] for i in range(len(rs)) for j in range(3)] == plain


def test_python_layers_exist_and_refuse_the_host():
    import torch
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd import validate as V
    from pointcloududa_amd.utils import metric as M
    import inspect
    assert list(inspect.signature(K.surface_metrics_ext).parameters) == ["pred", "gt", "classes", "spacing", "connectivity",
                                                                         "percentile"]
    assert inspect.signature(K.surface_metrics_ext).parameters["percentile"].default == 95.0
    for fn in (M.hd95, M.assd):
        assert list(inspect.signature(fn).parameters) == ["result", "reference", "voxelspacing", "connectivity"]
    assert list(inspect.signature(M.class_metrics_ext).parameters) == ["img_gt", "img_pred", "classes", "percentile"]
    assert inspect.signature(V.evaluate_volume).parameters["extended"].default is False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.surface_metrics_ext(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8), [1])
