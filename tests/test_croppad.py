"""CPU checks of the device-side CropAndPad with numpy's pad modes (pointcloududa_amd/utils/croppad.py, csrc/croppad.hip;
DESIGN.md section 6, f14): the fixture is numpy.pad's own output and its generator reproduces it, the plain restatement equals
numpy.pad live, the program validates, the C ABI agrees with its binding and refuses bad arguments before any launch, the two
new presets draw what they document, and the four older presets draw what they drew."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLD, ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _load("make_croppad_golden")


# ---------------------------------------------------------------------------------------------- fixture and restatement
def test_generator_reproduces_the_committed_fixture():
    path = os.path.join(GOLD, "croppad.npz")
    assert os.path.getsize(path) < 1000000
    old, new = np.load(path), G.build()
    assert sorted(old.files) == sorted(new)
    assert str(old["numpy_version"]) and tuple(old["mode_names"]) == G.MODES
    for k in new:
        if k != "numpy_version":
            assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), k
    # every mode at both channel counts and all four shapes; every mode meets every side set
    assert len(old["case_names"]) == 80 and len(old["checked"]) == 80 + 20 + 2 + 4
    seen = {(int(old["arg_" + n][4]), tuple(old["arg_" + n][:4])) for n in old["case_names"]}
    for mode in range(10):
        got = {s for m, s in seen if m == mode}
        assert {(3, 2, 0, 4), (0, 0, 0, 0), (-2, -1, -3, -2), (5, -2, -1, 6)} <= got, mode
        assert any(s[0] in (8, 11, 32, 63) and s[3] in (6, 9, 17, 47) for s in got), mode      # a pad of the size minus 1


def _random_sides(rng, h, w):
    while True:
        s = tuple(int(v) for v in rng.integers(-3, 7, 4))
        if G.sides_valid(h, w, *s):
            return s


@pytest.mark.parametrize("mode", range(10))
def test_restatement_equals_numpy_pad_live(mode):
    rng = np.random.default_rng(1000 + mode)
    for h, w, c in ((5, 4, 2), (6, 9, 1), (8, 8, 3), (11, 7, 4), (12, 13, 3)):
        for _ in range(6):
            x = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
            if rng.random() < 0.5:
                x[rng.integers(0, h), :] = rng.integers(0, 256)      # flat lines: zero steps, tied medians
            sides = _random_sides(rng, h, w)
            cval = int(rng.choice([0, 255, int(x[0, 0, 0]), int(rng.integers(0, 256))]))
            pt, pb, pl, pr = G.split_sides(h, w, *sides)[4:]
            xc = G.crop(x, *sides)
            want = G.numpy_pad(xc, pt, pb, pl, pr, mode, cval)
            got = G.pad_restated(xc, pt, pb, pl, pr, mode, cval)
            assert got.dtype == want.dtype and np.array_equal(got, want), (G.MODES[mode], (h, w, c), sides, cval)
            assert np.array_equal(G.resize_restated(want, h, w), G.resize_loops(want, h, w))


def test_restatement_separates_the_two_forms_of_the_ramp():
    """width 10, end 0, edge 90: k = 7 is 63 by floor(end + k step) and 62 once another edge value of the side equals end"""
    a, b = G.ramp_pair()
    for img, at7 in ((a, 63), (b, 62)):
        xc = G.crop(img, 0, -10, 0, 10)
        want = G.numpy_pad(xc, 0, 0, 10, 0, 2, 0)
        assert np.array_equal(G.pad_restated(xc, 0, 0, 10, 0, 2, 0), want)
        assert want[0, 7, 0] == at7 and want[0, 10, 0] == 90
    assert (a[:, 0] != 0).all() and (b[:, 0] == 0).sum() == 1


def test_net_zero_geometry_returns_the_padded_array():
    x = G.test_image(22, 22, 3, 5)
    for mode in range(10):
        big, res = G.crop_pad_restated(x, 10, -10, -10, 10, mode, 9)
        assert big.shape == x.shape and np.array_equal(big, res)


# ---------------------------------------------------------------------------------------------- the program
def test_validate_refuses_each_clause():
    from pointcloududa_amd.utils.croppad import CropPadProgram

    def prog(**kw):
        p = CropPadProgram.identity(2)
        p.set_crop_and_pad(1, *kw.get("sides", (2, 0, -1, 3)), kw.get("mode", 4), kw.get("cval", 7))
        return p
    prog().validate(16, 12)
    assert CropPadProgram.identity(3).is_identity() and not prog().is_identity() and prog().batch == 2
    bad = []
    p = prog(); p.opcode = p.opcode.astype(np.int64); bad.append((p, "opcode must be int32"))
    p = prog(); p.opcode = p.opcode.reshape(2, 1); bad.append((p, "opcode must be int32"))
    p = prog(); p.iarg = p.iarg[:, :5]; bad.append((p, "iarg must be int32"))
    p = prog(); p.iarg = p.iarg.astype(np.int64); bad.append((p, "iarg must be int32"))
    p = prog(); p.opcode[0] = 2; bad.append((p, "unknown opcode"))
    p = prog(); p.opcode[0] = -1; bad.append((p, "unknown opcode"))
    bad += [(prog(mode=10), "mode must be in 0..9"), (prog(mode=-1), "mode must be in 0..9"),
            (prog(cval=256), "cval must be in 0..255"), (prog(cval=-1), "cval must be in 0..255"),
            (prog(sides=(-8, 0, -7, 0)), "at least 2 pixels"), (prog(sides=(0, -5, 0, -6)), "at least 2 pixels"),
            (prog(sides=(16, 0, 0, 0)), "a pad must be at most"), (prog(sides=(0, 0, 0, 12)), "a pad must be at most"),
            (prog(sides=(-4, 0, 12, 0)), "a pad must be at most")]
    for p, msg in bad:
        with pytest.raises(ValueError, match=msg):
            p.validate(16, 12)
    prog(sides=(15, 11, 15, 11)).validate(16, 12)      # the cropped size minus 1 is allowed
    big = CropPadProgram.identity(1)
    big.set_crop_and_pad(0, 65, 0, 0, 0)
    with pytest.raises(ValueError, match="a pad must be at most"):
        big.validate(256, 256)
    big.set_crop_and_pad(0, 64, 64, 64, 64, 9, 255)
    big.validate(256, 256)
    for h, w in ((1, 12), (16, 1)):
        with pytest.raises(ValueError, match="at least 2"):
            CropPadProgram.identity(1).validate(h, w)
    # a dead sample's arguments are not read
    p = CropPadProgram.identity(1); p.iarg[0] = (99, 99, 99, 99, 99, 999); p.validate(8, 8)


def test_crop_pad_aug_requires_a_program_and_uint8_images():
    import torch
    from pointcloududa_amd.utils import augment as A
    from pointcloududa_amd.utils import croppad as Cp
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="program is required"):
        A.crop_pad_aug(x, None)
    with pytest.raises(TypeError, match="uint8"):
        A.crop_pad_aug(x.float(), None, A.CropPadProgram.identity(2))
    with pytest.raises(ValueError, match="batch of 2"):
        A.crop_pad_aug(x, None, A.CropPadProgram.identity(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.crop_pad_aug(x, None, A.CropPadProgram.identity(2))
    assert A.CropPadProgram is Cp.CropPadProgram and A.crop_pad_aug is Cp.crop_pad_aug and A.MODE_NAMES is Cp.MODE_NAMES
    assert tuple(n.lower() for n in Cp.MODE_NAMES) == G.MODES == tuple(sorted(G.MODES))
    assert (A.HEAVY_REFPAD_PRESET, A.AUG2_REFPAD_PRESET) == ("heavy_refpad_device", "mscmrseg_aug2_refpad_device")


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_declares_what_the_binding_binds():
    from pointcloududa_amd import _lib
    from pointcloududa_amd.utils import croppad as Cp
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p}
    for name, ret in (("pcuda_crop_pad", "int"), ("pcuda_crop_pad_workspace_size", "size_t")):
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (s.strip() for s in m.group(2).split(","))]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
    m = re.search(r"int pcuda_crop_pad\(([^;]*)\);", hdr)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "in", "out", "labels_in", "labels_out", "b", "h", "w", "c", "opcode", "iarg", "workspace", "workspace_bytes", "s"]
    for k, n in enumerate(Cp.MODE_NAMES):
        assert re.search(r"#define PCUDA_PAD_%s %d\b" % (n, k), hdr), n
    assert len(re.findall(r"#define PCUDA_PAD_\w+ \d+", hdr)) == 10
    assert int(re.search(r"#define\s+PCUDA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _lib.PCUDA_ABI_VERSION
    csrc = os.path.join(ROOT, "pointcloududa_amd", "csrc")
    assert "croppad.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "croppad.hip")).read()
    assert "kIArgs = %d" % Cp.IARGS in src and "kMaxPad = %d" % Cp.MAX_PAD in src


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """fake pointers: every call below must return before it touches the device"""
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    size = lib.pcuda_crop_pad_workspace_size
    need = size(4, 32, 48, 3)
    assert need % 16 == 0 and need >= 4 * 3 * (48 + 32 + 128) + 4 * 4
    for bad in ((0, 32, 48, 3), (-1, 32, 48, 3), (65536, 32, 48, 3), (4, 1, 48, 3), (4, 32, 1, 3), (4, 32, 48, 0), (4, 32, 48, 5),
                (1, 40000, 40000, 2)):
        assert size(*bad) == 0, bad
    fake = [0x10000 * k for k in range(1, 8)]

    def call(inp=fake[0], outp=fake[1], li=None, lo=None, b=4, h=32, w=48, c=3, op=fake[4], ia=fake[5], ws=fake[6], nbytes=need):
        return lib.pcuda_crop_pad(inp, outp, li, lo, b, h, w, c, op, ia, ws, nbytes, None)
    for kw in (dict(inp=None), dict(outp=None), dict(op=None), dict(ia=None)):
        assert call(**kw) == -1 and b"null pointer" in lib.pcuda_last_error(), kw
    assert call(outp=fake[0]) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(li=fake[2], lo=fake[2]) == -1 and b"in == out" in lib.pcuda_last_error()
    assert call(li=fake[2]) == -1 and b"labels" in lib.pcuda_last_error()
    assert call(lo=fake[3]) == -1 and b"labels" in lib.pcuda_last_error()
    for kw in (dict(b=0), dict(b=65536), dict(h=1), dict(w=1), dict(c=0), dict(c=5), dict(h=40000, w=40000)):
        assert call(**kw) == -1 and b"bad dims" in lib.pcuda_last_error(), kw
    assert call(nbytes=need - 1) == -4 and b"workspace" in lib.pcuda_last_error()
    assert call(ws=None) == -4 and call(nbytes=0) == -4


# ---------------------------------------------------------------------------------------------- the presets
REFPAD = ("heavy_refpad_device", "mscmrseg_aug2_refpad_device")


def _crop_stages(plan):
    from pointcloududa_amd.utils.augment import CropPadProgram
    return [s for s in plan.stages if isinstance(s, CropPadProgram)]


@pytest.mark.parametrize("preset", REFPAD)
def test_refpad_presets_draw_all_ten_modes_within_the_documented_ranges(preset):
    from pointcloududa_amd.utils import geometric as Geo
    from pointcloududa_amd.utils.augment import GeoProgram, sample_geo_program, sample_heavy_plan
    h, w, b = 64, 48, 500
    lo_h, hi_h = int(np.floor(-0.05 * h + 0.5)), int(np.floor(0.1 * h + 0.5))
    lo_w, hi_w = int(np.floor(-0.05 * w + 0.5)), int(np.floor(0.1 * w + 0.5))
    modes, samples = [], 0
    for seed in range(8):
        plan = sample_heavy_plan(b, preset, np.random.default_rng(seed), h, w)
        kinds = [type(s) for s in plan.stages]
        assert all(a is not b2 for a, b2 in zip(kinds, kinds[1:])), "two neighbours of one kind"
        crop = _crop_stages(plan)
        assert len(crop) == 1
        for st in plan.stages:
            # CropAndPad lives in the CropPadProgram alone: the geometric stages hold no resize-and-translate homography
            if isinstance(st, GeoProgram):
                f = st.farg[st.opcode == Geo.OP_HOMOGRAPHY]
                is_scale = (f[:, 1] == 0) & (f[:, 3] == 0) & (f[:, 6] == 0) & (f[:, 7] == 0) & (f[:, 0] > 0) & (f[:, 4] > 0)
                assert not np.any(is_scale & ((f[:, 0] != 1) | (f[:, 4] != 1)))
        st = crop[0]
        st.validate(h, w)
        live = st.opcode == 1
        a = st.iarg[live]
        assert np.all(st.iarg[~live] == 0)
        assert a[:, [0, 2]].min() >= lo_h and a[:, [0, 2]].max() <= hi_h and a[:, [1, 3]].min() >= lo_w and a[:, [1, 3]].max() <= hi_w
        assert a[:, 5].min() >= 0 and a[:, 5].max() <= 255
        modes.append(a[:, 4])
        samples += b
    assert samples == 4000
    modes = np.concatenate(modes)
    n = len(modes)
    assert abs(n - 2000) <= 4 * np.sqrt(4000 * 0.25)                     # sometimes(0.5)
    sd = np.sqrt(n * 0.1 * 0.9)
    counts = np.bincount(modes, minlength=10)
    assert len(counts) == 10 and np.all(np.abs(counts - n / 10.0) <= 4 * sd), counts
    geo = sample_geo_program(8, preset, np.random.default_rng(0), h, w)
    assert geo.slots == (6 if preset == REFPAD[0] else 0)


@pytest.mark.parametrize("preset", REFPAD)
def test_refpad_presets_consume_the_generator_as_documented(preset):
    """everything the _full_ twin draws, in the same order, then one integers(0, 10, batch); sides and cval are _draw_geo's"""
    from pointcloududa_amd.utils import geometric as Geo
    from pointcloududa_amd.utils import heavy as Hv
    from pointcloududa_amd.utils import stylize as St
    from pointcloududa_amd.utils.augment import sample_heavy_plan
    full = {"heavy_refpad_device": "heavy_full_device", "mscmrseg_aug2_refpad_device": "mscmrseg_aug2_full_device"}[preset]
    b, h, w = 16, 64, 48
    for seed in range(10):
        rng, twin, rng_full = (np.random.default_rng(seed) for _ in range(3))
        plan = sample_heavy_plan(b, preset, rng, h, w)
        spec = Hv._PRESETS[preset]
        assert [e if e == "block" else e[1] for e in spec["outer"]] == [e if e == "block" else e[1] for e in Hv._PRESETS[full]["outer"]]
        assert spec["block"] == Hv._PRESETS[full]["block"]
        twin.permutation(len(spec["outer"])); twin.permutation(len(spec["block"]))
        twin.integers(0, 6, b); twin.random((b, len(spec["block"])))
        for e in spec["block"]:
            if e in Hv._SOMETIMES:
                twin.random(b)
        coins = [twin.random(b) for e in spec["outer"] if e != "block"]
        dg = Geo._draw_geo(b, twin, h, w); Hv._draw_photo(b, twin); St.draw_style(b, twin)
        mode = twin.integers(0, 10, b)
        nxt = twin.integers(0, 2 ** 62)
        assert rng.integers(0, 2 ** 62) == nxt, (preset, seed)
        sample_heavy_plan(b, full, rng_full, h, w)
        rng_full.integers(0, 10, b)
        assert rng_full.integers(0, 2 ** 62) == nxt, (preset, seed)
        on = coins[[e for e in spec["outer"] if e != "block"].index(("c", Geo.ENTRY_CROP_AND_PAD))] < 0.5
        crop = _crop_stages(plan)
        if not on.any():
            assert not crop
            continue
        st = crop[0]
        assert np.array_equal(st.opcode == 1, on)
        for i in np.nonzero(on)[0]:
            t, r, bt, l = dg["crop"][i]
            want = (Geo.crop_pad_pixels(t, h), Geo.crop_pad_pixels(r, w), Geo.crop_pad_pixels(bt, h), Geo.crop_pad_pixels(l, w),
                    int(mode[i]), int(dg["crop_cval"][i]))
            assert tuple(st.iarg[i]) == want, (seed, i)


def test_the_four_older_presets_draw_what_they_drew():
    """sha256 of every stage's arrays for seeds 0..19, recorded on the commit before f14 (tests/golden/heavy_plan_digests.json)"""
    want = json.load(open(os.path.join(GOLD, "heavy_plan_digests.json")))
    assert sorted(want) == sorted(G.DIGEST_PRESETS) and all(len(v) == 20 for v in want.values())
    assert G.digests() == want


def test_augmented_batches_know_the_new_presets():
    import torch
    from pointcloududa_amd.utils import augment as A
    rng, cpu = np.random.default_rng(0), torch.device("cpu")
    for preset in REFPAD:
        assert A.AugmentedBatches(iter(()), cpu, None, rng, num_classes=5, rescale="div255", heavy_preset=preset).heavy_preset == preset
    with pytest.raises(ValueError, match="unknown heavy preset"):
        A.AugmentedBatches(iter(()), cpu, None, rng, num_classes=5, rescale="div255", heavy_preset="heavy_refpad")
    with pytest.raises(NotImplementedError) as e:
        A.sample_heavy_plan(2, "heavy", rng, 32, 32)
    assert str(e.value) == A.HEAVY_MESSAGE
