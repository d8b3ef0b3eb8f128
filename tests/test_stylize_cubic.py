"""The cubic upscale of the noise-alpha slot without a GPU: tests/golden/stylize_cubic.npz regenerates
exactly (scripts/make_stylize_cubic_golden.py: a numpy restatement pinned by one in exact rational arithmetic), StyleProgram
accepts ``UPSCALE_CUBIC`` and keeps rejecting 2, and the encoder writes what the generator's own encoder writes."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT


def _load(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))


C = _load("make_stylize_cubic_golden")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLD, "stylize_cubic.npz"))


def test_fixture_regenerates_exactly(fixture):
    assert os.path.getsize(os.path.join(GOLD, "stylize_cubic.npz")) < 200000
    g = C.build()      # (asserts that the two restatements agree, the cap and a clipped value at each end)
    assert sorted(g) == sorted(fixture.files)
    for k in fixture.files:
        assert np.array_equal(g[k], fixture[k]), k
    lo, hi = fixture["upscaled_extremes"]
    assert lo < 0.0 and hi > 1.0, "an upscaled value is clipped at each end"
    tot, exc = (int(v) for v in fixture["counts"])
    assert exc <= 1e-5 * tot


def test_fixture_covers_the_grids_counts_aggregations_and_the_sigmoid(fixture):
    cases = C.load_cases(fixture)
    seen, sizes = set(), set()
    for c in cases:
        assert np.all(c["opcode"] == C.S.NOISE_ALPHA) and np.all(c["iarg"][:, 0, 1] == C.UPSCALE_CUBIC) and len(c["exc"]) == 0
        for ia in c["iarg"][:, 0]:
            seen.add((int(ia[0]), int(ia[2]), int(ia[3])))
            sizes |= {(int(ia[4 + 2 * k]), int(ia[5 + 2 * k])) for k in range(int(ia[0]))}
        x = C.S.case_inputs(c)
        got, _ = C.run_program(x, c["opcode"], c["iarg"], c["farg"], c["table"], c["seed_arr"], backend="numpy")
        assert np.array_equal(got, c["u8"]), c["name"]
        assert not np.array_equal(got, x)
    assert seen == {(n, agg, sig) for n in (1, 3) for agg in range(3) for sig in (0, 1)}
    assert sizes == {(2, 2), (3, 5), (16, 16)}


def test_an_upscale_to_the_grid_s_own_size_returns_the_grid_s_bits():
    g = np.random.default_rng(1).random((7, 16))
    assert np.array_equal(C.upscale_cubic_numpy(g, 7, 16), g)
    # and a 2x upscale of a 0 / 1 step leaves [0, 1] on both sides of the step
    step = np.repeat(np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0]]), 3, axis=0)
    v = C.upscale_cubic_numpy(step, 6, 12)
    assert v.min() < 0.0 and v.max() > 1.0


def test_validate_accepts_cubic_and_keeps_rejecting_2():
    from pointcloududa_amd.utils import stylize as St
    assert (St.UPSCALE_NEAREST, St.UPSCALE_BILINEAR, St.UPSCALE_CUBIC) == (0, 1, 3)
    rng = np.random.default_rng(2)
    want = C.S.Prog(2, 1)
    got = St.StyleProgram.identity(2, 1)
    for i, sizes in enumerate((((2, 2),), ((3, 5), (16, 16), (2, 2)))):
        grids = [C.snapped_grid(h2, w2, rng) for h2, w2 in sizes]
        wts = C.S.edge(0.7)
        C.put_cubic(want, i, 0, grids, i, bool(i), 1.5 * i, wts)
        got.set_noise_alpha(i, 0, wts, grids, upscale=St.UPSCALE_CUBIC, aggregation=i, sigmoid=bool(i), thresh=1.5 * i)
    got.validate(17, 33, 3)
    for k in ("opcode", "iarg", "farg", "table"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    for bad in (2, 4, -1):
        got.iarg[1, 0, 1] = bad
        with pytest.raises(ValueError, match="upscale"):
            got.validate(17, 33, 3)
    got.iarg[1, 0, 1] = St.UPSCALE_CUBIC
    assert got.kernel_arrays(17, 33, 3)[1][1, 0, 1] == 3
