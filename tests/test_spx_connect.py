"""CPU checks of the connected superpixels (pointcloududa_amd/utils/stylize.py ``min_size``, csrc/spx_connect.hip; DESIGN.md
section 6, f9b): the sequential restatement against the vectorised one (scripts/make_spx_connect_golden.py), the fixture and
the digests regenerating exactly, the connectedness and min-size properties, the encoders (``min_size`` is opt-in: without it
the arrays are f9's), the two ``_connected_`` presets against their ``_refpad_`` twins, validation, and the header against the
exports and the binding.  No GPU."""
import ctypes
import importlib.util
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT

GEN = os.path.join(ROOT, "scripts", "make_spx_connect_golden.py")


def _helper():
    sys.path.insert(0, os.path.dirname(GEN))
    try:
        spec = importlib.util.spec_from_file_location("make_spx_connect_golden", GEN)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(os.path.dirname(GEN))
    return m


@pytest.fixture(scope="module")
def G():
    return _helper()


# ---------------------------------------------------------------------------------------------- restatements, fixture
def test_fixture_and_digests_regenerate_from_the_restatement(G):
    """the committed files are what the generator builds (its build asserts connectedness and the min-size property of every
    connected slot, that min_size = H W leaves one segment painted with the image's rdiv mean, and that p = 0 copies)"""
    g = np.load(os.path.join(GOLD, "spx_connect.npz"))
    new = G.build()
    assert sorted(g.files) == sorted(new)
    for k in new:
        a, b = np.asarray(new[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert json.load(open(os.path.join(GOLD, "spx_connect_digests.json"))) == G.build_digests()
    assert os.path.getsize(os.path.join(GOLD, "spx_connect.npz")) <= os.path.getsize(os.path.join(GOLD, "stylize.npz"))


def test_sequential_restatement_equals_the_vectorised_one(G):
    """the raster-order flood fill in plain Python integers against scipy's labels with pointer jumping, bit for bit, on every
    small case (the production cases run when the generator writes the files)"""
    assert G.check_restatement(G.small_cases()) == sum(c["u8"].size for c in G.load_cases(np.load(G.OUT)))


def test_fixture_holds_the_cases_the_kernels_can_go_wrong_on(G):
    cases = {c["name"]: c for c in G.load_cases(np.load(G.OUT))}
    assert set(cases) == {"one_pixel_1x1x1", "row_1x40x1", "column_40x1x1", "tiny_5x7x1", "odd_50x70x1", "fragments_64x48x3",
                          "smooth_48x64x3", "tiles_c4_130x90x4"}
    for c in cases.values():
        h, w = c["h"], c["w"]
        ia, fa = c["iarg"][:, 0], c["farg"][:, 0]
        gy, gx = int(ia[0, 0]), int(ia[0, 1])
        assert c["b"] == 9 and np.all(c["opcode"] == 3)
        assert ia[:, 5].tolist() == [m for m in (1, max(1, (h * w) // (2 * gy * gx)), h * w) for _ in range(3)]
        assert fa[:, 0].tolist() == [0.0, G.P_BETWEEN, 1.0] * 3
        assert np.all(c["segments"][:3] == c["components"][:3]), "min_size = 1 merges nothing"
        assert np.all(c["segments"][6:] == 1), "min_size = H W drains everything into pixel 0's segment"
        assert np.all(c["segments"] <= c["components"])
        x = G.case_inputs(c)
        for i in (0, 3, 6):
            assert np.array_equal(c["u8"][i], x[i]), "p_replace = 0 copies"
        mean = G.rdiv(x[8].astype(np.int64).reshape(h * w, -1).sum(0), h * w)
        assert np.all(c["u8"][8].reshape(h * w, -1) == mean), "min_size = H W with p = 1 is the image's rdiv mean"
    f = cases["fragments_64x48x3"]
    assert f["iarg"][0, 0, :4].tolist() == [16, 16, 0, 0] and f["longest_chain"][3] >= 64 and f["components"][0] > 2000
    assert cases["odd_50x70x1"]["iarg"][0, 0, :3].tolist() == [10, 20, 5] and (50 * 70) % 64 != 0
    d = json.load(open(G.OUT_DIGESTS))
    assert sorted(d) == ["production_n20", "production_n200"]
    for v in d.values():
        assert v["dims"][:4] == [2, 256, 256, 3] and max(v["rounds"]) >= 9 and max(v["longest_chain"]) > 256


def test_the_properties_hold_and_the_checker_sees_a_violation(G):
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 6, (23, 31))
    for m in (1, 2, 5, 40, 23 * 31):
        fin, ids = G.final_ids_numpy(lab, m)
        G.check_properties(fin, ids, m)
        assert fin[0, 0] == 0                                                  # pixel 0 keeps its own id
    fin, ids = G.final_ids_numpy(lab, 5)
    with pytest.raises(AssertionError, match="min_size"):
        G.check_properties(ids, ids, 5)                                        # nothing merged: small segments remain
    # a hand case, W = 4: labels  0 0 1 1 / 2 0 1 3: components {0,1,5}, {2,3,6}, {4}, {7}
    lab = np.array([[0, 0, 1, 1], [2, 0, 1, 3]])
    fin, ids = G.final_ids_numpy(lab, 2)
    assert ids.ravel().tolist() == [0, 0, 2, 2, 4, 0, 2, 7]
    assert fin.ravel().tolist() == [0, 0, 2, 2, 0, 0, 2, 2]      # 4 (x = 0) goes up to pixel 0's, 7 goes left to 6's
    G.check_properties(fin, ids, 2)
    broken = fin.copy()
    broken[1, 3] = 0                                             # id 0's segment in two pieces
    with pytest.raises(AssertionError, match="in pieces"):
        G.check_properties(broken, ids, 2)
    out, f2 = G.connect_python(np.arange(8, dtype=np.uint8).reshape(2, 4, 1) * 10, lab.ravel().tolist(), 2, 2 ** 32 - 1, 3)
    assert np.array_equal(f2, fin)
    assert out.ravel().tolist() == [25, 25, 45, 45, 25, 25, 45, 45]      # rdiv(0 + 10 + 40 + 50, 4), rdiv(20 + 30 + 60 + 70, 4)


# ---------------------------------------------------------------------------------------------- encoders, presets
def test_min_size_is_opt_in_and_the_default_arrays_are_unchanged(G):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import stylize as S
    mine, gen = S.StyleProgram.identity(2, 2), G.Prog(2, 2)
    mine.set_superpixels(0, 1, 4, 5, 0.25, 77)
    gen.put(0, 1, 3, gy=4, gx=5, iters=5, p=0.25, seed=77)
    mine.set_superpixels(1, 0, 6, 7, 1.0, 2 ** 63 + 5, iters=0, compactness=0)
    gen.put(1, 0, 3, gy=6, gx=7, iters=0, p=1.0, seed=2 ** 63 + 5, compactness=0)
    for a, b in zip((mine.opcode, mine.iarg, mine.farg, mine.table, mine.seed), (gen.opcode, gen.iarg, gen.farg, gen.table, gen.seed)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert not mine.needs_connect()
    arrays = mine.kernel_arrays(32, 32, 3)
    assert len(arrays) == 5 and np.all(arrays[1][..., 5] == 0)
    mine.set_superpixels(0, 0, 4, 5, 0.25, 77, min_size=9)
    assert mine.iarg[0, 0, 5] == 9 and mine.needs_connect() and mine.kernel_arrays(32, 32, 3)[1][0, 0, 5] == 9
    mine.set_hue_saturation(0, 0, 3, 4)
    assert not mine.needs_connect() and mine.iarg[0, 0, 5] == 0
    hue = S.StyleProgram.identity(1, 1)
    hue.iarg[0, 0, 5] = 3                      # (another opcode's iarg[5] is not a min_size)
    assert not hue.needs_connect()
    assert S.superpixel_min_size(14, 14, 256, 256) == 167 and S.superpixel_min_size(16, 16, 8, 8) == 1
    assert S.superpixel_min_size(4, 5, 256, 256) == G.superpixel_min_size(4, 5, 256, 256) == 1638
    assert A.superpixel_min_size is S.superpixel_min_size
    assert (A.HEAVY_CONNECTED_PRESET, A.AUG2_CONNECTED_PRESET) == ("heavy_connected_device", "mscmrseg_aug2_connected_device")
    p = inspect.signature(K.stylize).parameters
    assert list(p) == ["images_u8", "opcode", "iarg", "farg", "table", "seed", "out", "connect"] and p["connect"].default is False
    assert inspect.signature(S.StyleProgram.set_superpixels).parameters["min_size"].default == 0


@pytest.mark.parametrize("preset,twin", [("heavy_connected_device", "heavy_refpad_device"),
                                         ("mscmrseg_aug2_connected_device", "mscmrseg_aug2_refpad_device")])
def test_a_connected_plan_is_the_refpad_plan_plus_min_size(preset, twin):
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import stylize as S
    seen = 0
    for seed in range(12):
        ra, rb = np.random.default_rng(seed), np.random.default_rng(seed)
        a, b = A.sample_heavy_plan(6, preset, ra, 64, 48), A.sample_heavy_plan(6, twin, rb, 64, 48)
        assert ra.bit_generator.state == rb.bit_generator.state, "the generator is consumed draw for draw"
        assert [type(s) for s in a.stages] == [type(s) for s in b.stages]
        for sa, sb in zip(a.stages, b.stages):
            if not isinstance(sa, S.StyleProgram):
                for f in ("opcode", "iarg", "farg", "seed"):
                    if hasattr(sa, f):
                        assert np.array_equal(getattr(sa, f), getattr(sb, f)), f
                continue
            for f in ("opcode", "farg", "table", "seed"):
                assert np.array_equal(getattr(sa, f), getattr(sb, f)), f
            spx = sa.opcode == S.OP_SUPERPIXELS
            keep = np.ones(sa.iarg.shape, dtype=bool)
            keep[..., 5] = ~spx
            assert np.array_equal(sa.iarg[keep], sb.iarg[keep]) and np.all(sb.iarg[spx][:, 5] == 0)
            for ia in sa.iarg[spx]:
                assert ia[5] == S.superpixel_min_size(ia[0], ia[1], 64, 48) >= 1
            assert sa.needs_connect() == bool(spx.any()) and not sb.needs_connect()
            seen += int(spx.sum())
        pa = A.sample_style_program(6, preset, np.random.default_rng(seed), 64, 48)
        pb = A.sample_style_program(6, twin, np.random.default_rng(seed), 64, 48)
        assert np.array_equal(pa.opcode, pb.opcode) and np.array_equal(pa.iarg[..., :5], pb.iarg[..., :5])
        assert pa.needs_connect() == bool((pa.opcode == S.OP_SUPERPIXELS).any())
    assert seen > 0


def test_validate_names_min_size():
    from pointcloududa_amd.utils.stylize import StyleProgram
    p = StyleProgram.identity(1, 1)
    p.set_superpixels(0, 0, 2, 2, 0.5, 1, min_size=-1)
    with pytest.raises(ValueError, match=r"min_size \(iarg\[5\]\) must be in 0\.\.H W"):
        p.validate(8, 8, 1)
    p.set_superpixels(0, 0, 2, 2, 0.5, 1, min_size=65)
    with pytest.raises(ValueError, match=r"min_size \(iarg\[5\]\) must be in 0\.\.H W"):
        p.validate(8, 8, 1)
    p.set_superpixels(0, 0, 2, 2, 0.5, 1, min_size=64)
    p.validate(8, 8, 1)
    p.validate()                                       # (without a shape only the sign is checked)
    with pytest.raises(ValueError, match=r"min_size \(iarg\[5\]\) > 0 takes images of at most 2\^24 pixels"):
        p.validate(4096, 4097, 1)
    p.validate(4096, 4096, 1)
    p.set_superpixels(0, 0, 2, 2, 0.5, 1)
    p.validate(4096, 4097, 1)                          # unconnected slots keep f9's limits


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_exports_and_prototypes_agree_on_the_new_entry_points():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret in (("pcuda_stylize_connect", "int"), ("pcuda_stylize_connect_workspace_size", "size_t")):
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (s.strip() for s in m.group(2).split(","))]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name)
    params = lambda n: [a.split()[-1].lstrip("*") for a in re.search(r"int %s\(([^;]*)\);" % n, hdr).group(1).split(",")]
    assert params("pcuda_stylize_connect") == params("pcuda_stylize")
    assert int(re.search(r"#define\s+PCUDA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _lib.PCUDA_ABI_VERSION
    mk = open(os.path.join(ROOT, "pointcloududa_amd", "csrc", "Makefile")).read()
    assert "spx_connect.hip" in mk.split("SRCS")[1].splitlines()[0]


def test_workspace_size_and_rejections_without_a_gpu():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    for b, h, w, c in ((1, 1, 1, 1), (2, 50, 70, 1), (5, 130, 90, 4), (32, 256, 256, 3), (3, 7, 5, 2)):
        need, base = lib.pcuda_stylize_connect_workspace_size(b, h, w, c), lib.pcuda_stylize_workspace_size(b, h, w, c)
        assert need >= base + 4 * b * h * w and need % 16 == 0
        assert need == base + 2 * (-(-4 * b * h * w // 16) * 16) + (-(-4 * b * h * w * (c + 1) // 16) * 16)      # the header's layout
    for dims in ((0, 8, 8, 3), (2, 0, 8, 3), (2, 8, -1, 3), (2, 8, 8, 0)):
        assert lib.pcuda_stylize_connect_workspace_size(*dims) == 0
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected before a launch
    other = ctypes.c_void_p(8192)
    call = lambda inp=fake, outp=other, b=1, h=8, w=8, c=3, slots=1, ws=fake, n=1 << 20: lib.pcuda_stylize_connect(
        inp, outp, b, h, w, c, slots, fake, fake, fake, fake, fake, ws, n, None)
    assert call(outp=fake) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(slots=9) == -1 and call(inp=None) == -1 and call(c=5) == -1 and call(b=0) == -1
    assert call(h=4096, w=4097, c=1, n=1 << 40) == -1 and b"2^24" in lib.pcuda_last_error()
    need = lib.pcuda_stylize_connect_workspace_size(1, 8, 8, 3)
    assert call(n=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(n=lib.pcuda_stylize_workspace_size(1, 8, 8, 3)) == -4 and call(ws=None) == -4
