"""Superpixels at a working size (csrc/spx_scale.hip), the host side: the committed fixture
tests/golden/spx_scaled.npz against the vectorised restatement that wrote it (scripts/make_spx_scaled_golden.py), the working
size, the integer resize's anchors, ``StyleProgram.validate`` on the new field, the ``_scaled_`` presets' relation to their
``_connected_`` twins and the header.  The rule is this build's own (imgaug, cv2 and skimage are not installed: parity with
imgaug's max_size = 128 path is unpinned)."""
import importlib.util
import json
import os
import re
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
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return m


G = _load("make_spx_scaled_golden")
CASES = G.load_cases(np.load(os.path.join(GOLD, "spx_scaled.npz")))


def test_the_fixture_is_small_and_holds_the_four_shapes():
    assert os.path.getsize(os.path.join(GOLD, "spx_scaled.npz")) < 300000
    assert [(c["h"], c["w"], c["c"], int(c["iarg"][0, 0, 6]), c["working"]) for c in CASES] == [
        (40, 56, 3, 16, [11, 16]), (56, 40, 1, 16, [16, 11]), (33, 47, 4, 20, [14, 20]), (64, 64, 3, 32, [32, 32])]
    for c in CASES:
        r = c["replaced"].tolist()
        assert (c["iarg"][:, 0, 5] > 0).any() and not r[0] and not r[3] and r[2] and r[5]
    assert (CASES[2]["iarg"][:, 0, 5] > 0).all() and (CASES[0]["iarg"][:3, 0, 5] == 0).all()
    edges = json.load(open(os.path.join(GOLD, "spx_scaled_edges.json")))
    assert sorted(edges) == ["production_n20", "production_n200"]
    for d in edges.values():
        assert d["dims"][:4] == [2, 256, 256, 3] and d["working"] == [128, 128] and d["max_size"] == 128 and d["min_size"] > 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_vectorised_restatement_reproduces_the_fixture(case):
    x = G.case_inputs(case)
    got, exc = G.run_program(x, case["opcode"], case["iarg"], case["farg"], case["table"], case["seed_arr"], backend="numpy")
    assert not exc.any() and np.array_equal(got, case["u8"])
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[3], x[3]), "p_replace = 0 returns the input, not the round trip"


def test_the_sequential_restatement_agrees_on_one_case():
    case = CASES[0]
    rows = slice(1, 5)      # p between / 1 unconnected, p 0 / between connected
    got, _ = G.run_program(G.case_inputs(case)[rows], *(case[k][rows] for k in ("opcode", "iarg", "farg", "table", "seed_arr")),
                           backend="independent")
    assert np.array_equal(got, case["u8"][rows])


def test_working_size_table():
    from pointcloududa_amd.utils.stylize import SUPERPIXELS_MAX_SIZE, superpixel_working_size
    assert SUPERPIXELS_MAX_SIZE == 128
    for (h, w, m), want in (((256, 256, 128), (128, 128)), ((224, 224, 128), (128, 128)), ((200, 256, 128), (100, 128)),
                            ((40, 56, 16), (11, 16)), ((3, 500, 128), (1, 128)), ((56, 40, 16), (16, 11)),
                            ((128, 128, 128), (128, 128)), ((64, 100, 128), (64, 100)), ((64, 100, 100), (64, 100)),
                            ((300, 200, 0), (300, 200)), ((300, 200, -5), (300, 200))):
        assert superpixel_working_size(h, w, m) == want, (h, w, m)
        assert G.working_size(h, w, m) == want
    rng = np.random.default_rng(3)
    for h, w, m in rng.integers(1, 700, (200, 3)):
        hs, ws = superpixel_working_size(h, w, m)
        assert (hs, ws) == G.working_size(int(h), int(w), int(m))
        if max(h, w) > m:
            assert max(hs, ws) == m and min(hs, ws) >= 1, "the longer side is exactly max_size"


@pytest.mark.parametrize("fn", ["resize_numpy", "resize_python"])
def test_resize_anchors(fn):
    f = getattr(G, fn)
    rdiv = lambda a, b: (2 * a + b) // (2 * b)
    rng = np.random.default_rng(17)
    x = rng.integers(0, 256, (14, 10, 3), dtype=np.uint8)
    assert np.array_equal(f(x, 14, 10), x), "equal sizes return the input"
    assert np.array_equal(f(x, 7, 5), rdiv(x.astype(np.int64).reshape(7, 2, 5, 2, 3).sum((1, 3)), 4)), "exact 2x shrink"
    assert np.all(f(np.full((9, 4, 2), 131, dtype=np.uint8), 23, 17) == 131), "a constant image stays constant"
    for dh, dw in ((40, 56), (3, 2), (1, 1), (14, 37), (33, 10)):
        y = f(x, dh, dw)
        assert y.shape == (dh, dw, 3) and y.min() >= x.min() and y.max() <= x.max(), "every value lies in the input's range"
    one = rng.integers(0, 256, (1, 9, 1), dtype=np.uint8)      # a single source row: both taps are that row
    assert np.array_equal(f(one, 4, 9), np.repeat(one, 4, axis=0))


def test_the_two_resizes_agree_and_the_float_one_does_not():
    x = np.random.default_rng(23).integers(0, 256, (11, 16, 3), dtype=np.uint8)
    for dh, dw in ((40, 56), (5, 7), (11, 33)):
        assert np.array_equal(G.resize_numpy(x, dh, dw), G.resize_python(x, dh, dw))
    bad, total = G.float_mismatches()
    assert 0 < bad < total // 100, "ties decided by rounding error: the reason for the integer form"


def _scaled_program(h=40, w=56, gy=3, gx=4, min_size=0, max_size=16):
    from pointcloududa_amd.utils.stylize import StyleProgram
    prog = StyleProgram.identity(2, 2)
    prog.set_superpixels(1, 1, gy, gx, 0.5, 9, min_size=min_size, max_size=max_size)
    return prog


def test_set_superpixels_writes_iarg6_and_needs_scale():
    from pointcloududa_amd.utils.stylize import StyleProgram
    prog = _scaled_program(min_size=7)
    assert prog.iarg[1, 1, 6] == 16 and prog.iarg[1, 1, 5] == 7 and prog.iarg[0, 0, 6] == 0
    assert prog.needs_scale(40, 56) and prog.needs_scale(17, 3) and not prog.needs_scale(16, 16) and not prog.needs_scale(9, 16)
    plain = StyleProgram.identity(1, 1)
    plain.set_superpixels(0, 0, 3, 4, 0.5, 9, min_size=7)
    assert plain.iarg[0, 0, 6] == 0 and not plain.needs_scale(4000, 4000)
    hue = StyleProgram.identity(1, 1)
    hue.set_hue_saturation(0, 0, 3, 4)
    hue.iarg[0, 0, 6] = 5      # (another opcode's iarg[6] is not a max_size)
    assert not hue.needs_scale(40, 56)
    prog.set_superpixels(1, 1, 3, 4, 0.5, 9)
    assert prog.iarg[1, 1, 6] == 0 and not prog.needs_scale(40, 56)


def test_validate_measures_a_scaled_slot_against_its_working_size():
    _scaled_program().validate(40, 56, 3)
    _scaled_program(gy=11, gx=16, min_size=11 * 16).validate(40, 56, 3)
    with pytest.raises(ValueError, match=r"max_size \(iarg\[6\]\)"):
        _scaled_program(max_size=-1).validate(40, 56, 3)
    with pytest.raises(ValueError, match=r"max_size \(iarg\[6\]\)"):
        _scaled_program(max_size=-1).validate()
    with pytest.raises(ValueError, match=r"gy, gx \(iarg\[0:2\]\).*working size"):
        _scaled_program(gy=12).validate(40, 56, 3)      # h' = 11
    with pytest.raises(ValueError, match=r"gy, gx \(iarg\[0:2\]\).*working size"):
        _scaled_program(gx=17).validate(40, 56, 3)      # w' = 16
    with pytest.raises(ValueError, match=r"min_size \(iarg\[5\]\).*working size"):
        _scaled_program(min_size=11 * 16 + 1).validate(40, 56, 3)
    # the same values on a slot that is not scaled are measured against H, W as before
    _scaled_program(gy=12, gx=17, min_size=11 * 16 + 1, max_size=56).validate(40, 56, 3)
    _scaled_program(gy=12, gx=17, min_size=11 * 16 + 1, max_size=0).validate(40, 56, 3)
    with pytest.raises(ValueError, match=r"max_size \(iarg\[6\]\).*2\^24"):
        _scaled_program().validate(4097, 4096, 3)
    _scaled_program(max_size=5000).validate(4097, 4096, 3)
    assert len(_scaled_program().kernel_arrays(40, 56, 3)) == 5


@pytest.mark.parametrize("scaled,connected", [("heavy_scaled_device", "heavy_connected_device"),
                                              ("mscmrseg_aug2_scaled_device", "mscmrseg_aug2_connected_device")])
@pytest.mark.parametrize("h,w", [(256, 256), (200, 256), (64, 64)])
def test_a_scaled_preset_is_its_connected_twin_with_max_size(scaled, connected, h, w):
    from pointcloududa_amd.utils.augment import StyleProgram, sample_heavy_plan, sample_style_program
    from pointcloududa_amd.utils.stylize import (OP_SUPERPIXELS, superpixel_grid, superpixel_min_size, superpixel_working_size)
    hs, ws = superpixel_working_size(h, w, 128)
    slots = 0
    for seed in range(6):
        for interp in ("linear", "cubic"):
            ra, rb = np.random.default_rng(seed), np.random.default_rng(seed)
            a, b = sample_heavy_plan(8, scaled, ra, h, w, interp=interp), sample_heavy_plan(8, connected, rb, h, w, interp=interp)
            assert ra.bit_generator.state == rb.bit_generator.state, "the generator is consumed alike"
            assert [type(s) for s in a.stages] == [type(s) for s in b.stages]
            for sa, sb in zip(a.stages, b.stages):
                if not isinstance(sa, StyleProgram):
                    for f in sa.__dataclass_fields__:
                        assert np.array_equal(getattr(sa, f), getattr(sb, f)), f
                    continue
                spx = sa.opcode == OP_SUPERPIXELS
                assert np.array_equal(sa.opcode, sb.opcode) and np.array_equal(sa.farg, sb.farg)
                assert np.array_equal(sa.table, sb.table) and np.array_equal(sa.seed, sb.seed)
                ia, ib = sa.iarg.copy(), sb.iarg.copy()
                assert np.all(ia[spx][:, 6] == 128) and np.all(ib[..., 6][spx] == 0) and np.all(ia[~spx] == ib[~spx])
                for row in ia[spx]:
                    gy, gx = int(row[0]), int(row[1])
                    assert gy <= hs and gx <= ws and row[5] == superpixel_min_size(gy, gx, hs, ws)
                for q in (ia, ib):
                    q[spx, 0:2] = 0
                    q[spx, 5:7] = 0
                assert np.array_equal(ia, ib), "only iarg[0:2], iarg[5] and iarg[6] of the Superpixels slots differ"
                if (hs, ws) == (h, w):
                    assert np.array_equal(sa.iarg[..., :6], sb.iarg[..., :6])
                sa.validate(h, w, 3)
                assert sa.needs_scale(h, w) == (bool(spx.any()) and max(h, w) > 128)
                slots += int(spx.sum())
    assert slots > 0
    ra, rb = np.random.default_rng(77), np.random.default_rng(77)
    pa, pb = sample_style_program(8, scaled, ra, h, w), sample_style_program(8, connected, rb, h, w)
    assert ra.bit_generator.state == rb.bit_generator.state and np.array_equal(pa.opcode, pb.opcode)
    assert np.array_equal(pa.seed, pb.seed) and np.array_equal(pa.iarg[..., 2:5], pb.iarg[..., 2:5])
    for row in pa.iarg[pa.opcode == OP_SUPERPIXELS]:
        assert row[6] == 128 and (int(row[0]), int(row[1])) in {superpixel_grid(n, hs, ws) for n in range(20, 201)}


def test_augment_batches_accept_the_scaled_presets_and_unknown_ones_raise():
    from pointcloududa_amd.utils import augment as A
    assert A.HEAVY_SCALED_PRESET == "heavy_scaled_device" and A.AUG2_SCALED_PRESET == "mscmrseg_aug2_scaled_device"
    for preset in (A.HEAVY_SCALED_PRESET, A.AUG2_SCALED_PRESET):
        assert A._check_preset(preset)["scaled"] and A._check_preset(preset)["connected"]
    with pytest.raises(ValueError, match="heavy_scaled_device"):
        A._check_preset("heavy_scaled")      # (the message lists the presets there are)


def test_the_header_and_the_binding_declare_both_functions():
    from pointcloududa_amd import _lib
    text = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    assert re.search(r"size_t\s+pcuda_stylize_scaled_workspace_size\(int b, int h, int w, int c\);", text)
    m = re.search(r"int\s+pcuda_stylize_scaled\(([^;]*)\);", text)
    c = re.search(r"int\s+pcuda_stylize_connect\(([^;]*)\);", text)
    assert m and c and re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", c.group(1)), "pcuda_stylize_connect's argument list"
    src = open(_lib.__file__).read()
    assert '"pcuda_stylize_scaled_workspace_size"' in src and '"pcuda_stylize_scaled"' in src
    assert "spx_scale.hip" in open(os.path.join(ROOT, "pointcloududa_amd", "csrc", "Makefile")).read()
