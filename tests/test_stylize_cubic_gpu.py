"""The cubic upscale of the noise-alpha slot on the GPU, through ``stylize_aug``, against the NUMPY
restatement of scripts/make_stylize_cubic_golden.py.

Rule: bit for bit at every value, with no excused value.  The upscale, the clip, the aggregation, the correlation and the
blend are the same IEEE float64 operations in the same order on both sides; the sigmoid's ``exp`` may differ in its last
bits between the device and numpy, which moves the blend by about 1e-13 of a grey level -- the fixture and the cases below
hold no value within 1e-9 of a rounding boundary (the generator's exact restatement checks the fixture; the cases here
assert it on the float64 values), so no value can flip."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


def _load(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return m


C = _load("make_stylize_cubic_golden")
CASES = C.load_cases(np.load(os.path.join(GOLD, "stylize_cubic.npz")))
KEYS = ("opcode", "iarg", "farg", "table", "seed_arr")


def _run(dev, images, arrays):
    from pointcloududa_amd.utils.stylize import StyleProgram, stylize_aug
    x = torch.from_numpy(images).to(dev)
    keep = x.clone()
    out = stylize_aug(x, StyleProgram(*(np.ascontiguousarray(a) for a in arrays)))
    assert out.dtype == torch.uint8 and out.shape == x.shape and torch.equal(x, keep)
    return out.cpu().numpy()


def _same(got, want, name):
    diff = got != want
    print("%s: %d values, %d differ" % (name, got.size, int(diff.sum())))
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[diff][:5].tolist(), want[diff][:5].tolist())


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_fixture_case(dev, name):
    case = [c for c in CASES if c["name"] == name][0]
    assert len(case["exc"]) == 0
    got = _run(dev, C.S.case_inputs(case), [case[k] for k in KEYS])
    _same(got, case["u8"], name)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hw", [(17, 33), (64, 48)])
def test_small_and_large_grids_match_the_numpy_restatement(dev, hw, c):
    """2x2 and 16x16 grids (and one slot of three grids) on images that are no multiple of the workgroup"""
    h, w = hw
    rng = np.random.default_rng(10 * h + c)
    combos = [([(2, 2)], 2, False), ([(16, 16)], 0, False), ([(2, 2)], 1, True), ([(16, 16)], 2, True),
              ([(16, 16), (2, 2), (3, 5)], 1, False), ([(2, 2), (16, 16), (16, 16)], 0, True)]
    for attempt in range(20):      # (inputs without a value within 1e-9 of a rounding boundary: f9's rule on the restatement)
        x = rng.integers(0, 256, (len(combos), h, w, c), dtype=np.uint8)
        prog = C.S.Prog(len(combos), 1)
        for i, (sizes, agg, sig) in enumerate(combos):
            C.put_cubic(prog, i, 0, [C.snapped_grid(h2, w2, rng) for h2, w2 in sizes], agg, sig, float(rng.normal(0, 5)) if sig else 0.0,
                        C.S.edge(float(rng.uniform(0.5, 1.0))))
        arrays = (prog.opcode, prog.iarg, prog.farg, prog.table, prog.seed)
        want, exc = C.run_any_program(x, *arrays)
        if not exc.any():
            break
    assert not exc.any() and not np.array_equal(want, x)
    _same(_run(dev, x, arrays), want, "%dx%dx%d" % (h, w, c))
    # the other upscales of the same slots still are what f9 pinned: the cubic path changed nothing for them
    for up in (0, 1):
        other = prog.iarg.copy()
        other[:, 0, 1] = up
        w9, e9 = C.S.run_program(x, prog.opcode, other, prog.farg, prog.table, prog.seed, backend="numpy")
        got = _run(dev, x, (prog.opcode, other, prog.farg, prog.table, prog.seed))
        assert not ((got != w9) & ~e9).any() and not np.array_equal(got, want)


def test_the_cubic_upscale_adds_no_host_synchronisation(dev):
    from pointcloududa_amd.utils.stylize import StyleProgram, stylize_aug
    case = CASES[0]
    x = torch.from_numpy(C.S.case_inputs(case)).to(dev)
    prog = StyleProgram(*(np.ascontiguousarray(case[k]) for k in KEYS))
    ref = stylize_aug(x, prog)      # (warm: allocator, library load)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        got = stylize_aug(x, prog)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, ref)
