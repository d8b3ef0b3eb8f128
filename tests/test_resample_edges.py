"""CPU checks of the second fixture of the device-side spacing resample, tests/golden/resample_edges.npz (csrc/resample.hip;
DESIGN.md section 6, f12): it loads, stays under the size limit, its digests match the restatement on the stored or
regenerated inputs, and every case reaches the branch of the kernels it is there for -- the tie counts, the bit lengths of the
variance's integers, the workgroup counts derived from the constants of the source text.  No GPU."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLD, ROOT

GEN = os.path.join(ROOT, "scripts", "make_resample_golden.py")
_spec = importlib.util.spec_from_file_location("make_resample_golden", GEN)
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
PATH = os.path.join(GOLD, "resample_edges.npz")
FILE = np.load(PATH)
ZOOM, LABELS, STATS = G.load_edge_cases(FILE)
ZBY, LBY, SBY = ({c["name"]: c for c in cases} for cases in (ZOOM, LABELS, STATS))
SRC = open(os.path.join(ROOT, "pointcloududa_amd", "csrc", "resample.hip")).read()


def _constant(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, SRC).group(1))


def _have_scipy():
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except ImportError:
        return False


def _window(c):
    return G.crop_window(c["zh"], c["zw"], c["crop"])[2:]


def test_the_file_loads_names_its_versions_and_stays_small():
    assert len(ZOOM) == 19 and len(LABELS) == 8 and len(STATS) == 6
    assert str(FILE["scipy_version"]) and str(FILE["numpy_version"])
    assert os.path.getsize(PATH) < 1000 * 1000
    assert G.EDGES_PATH == PATH
    first = np.load(os.path.join(GOLD, "resample.npz"))
    assert not {str(n) for n in first["zoom_cases"]} & set(ZBY) and not {str(n) for n in first["stat_cases"]} & set(SBY)


def test_the_restatement_equals_the_stored_scipy_arrays_and_digests():
    for c in ZOOM:
        assert c["scipy"].dtype == c["vol"].dtype and c["scipy"].shape == (c["vol"].shape[0],) + _window(c), c["name"]
        assert G.bit_equal(G.zoom_rule(c["vol"], c["zh"], c["zw"], c["crop"]), c["scipy"]), c["name"]
    for c in LABELS:
        lab, stray = G.label_rule(c["raw"], c["zh"], c["zw"], c["num_classes"], c["remap"], c["crop"])
        assert G.bit_equal(lab, c["scipy"]) and stray == 0 and c["scipy"].shape == (c["raw"].shape[0],) + _window(c), c["name"]
    for c in STATS:
        z, numpy_out = G.expected_stat_arrays(c)                        # (raises where the digest differs)
        assert z.dtype == c["vol"].dtype and z.shape == (c["vol"].shape[0],) + _window(c) == numpy_out.shape, c["name"]
        assert re.fullmatch(r"[0-9a-f]{64}", c["sha256"]), c["name"]
        ref_mean, ref_std = (float(v) for v in c["numpy_stats"])
        mean, std = (float(v) for v in c["rule_stats"])
        if z.dtype == np.float32:
            assert (mean, std) == G.f32_stats(z), c["name"]
        else:
            assert (mean, std) == G.int_stats(z) and mean == ref_mean == float(np.mean(z)), c["name"]
            assert z.flags["C_CONTIGUOUS"] and abs(ref_std - float(np.std(z))) <= z.size * 2.0 ** -53 * ref_std, c["name"]
        assert abs(std - ref_std) <= z.size * 2.0 ** -53 * ref_std, c["name"]
        differ = int(np.count_nonzero(G.standardize_rule(z, mean, std).view(np.uint32) != numpy_out.view(np.uint32)))
        assert differ == c["differ"] and differ * 100 <= z.size, c["name"]
    wrong = dict(SBY["u8_many_520x3x3_to_33x4"], sha256="0" * 64)
    with pytest.raises(AssertionError, match="not the ones scipy gave"):
        G.expected_stat_arrays(wrong)


def test_the_zoom_cases_reach_the_ties_the_second_trip_and_the_one_sample_axes():
    for tag, dt in G.DTYPES:
        for stem, n, src, dst in (("9x5_to_17x17", 2, (9, 5), (17, 17)), ("3x300_to_5x1030", 1, (3, 300), (5, 1030)),
                                  ("3x300_to_5x1028", 1, (3, 300), (5, 1028)), ("6x1_to_9x4", 2, (6, 1), (9, 4)),
                                  ("1x6_to_4x9", 2, (1, 6), (4, 9)), ("6x7_to_40x1", 2, (6, 7), (40, 1))):
            c = ZBY["%s_%s" % (tag, stem)]
            assert c["vol"].dtype == dt and c["vol"].shape == (n,) + src and c["scipy"].shape == (n,) + dst and c["crop"] == 0, c["name"]
    # weights of exactly 0.5 and 0.25: z = 8 / 16 and 4 / 16
    ty, tx = G.axis_terms(9, 17)[1], G.axis_terms(5, 17)[1]
    assert set(ty.tolist()) == {0.0, 0.5} and set(tx.tolist()) == {0.0, 0.25, 0.5, 0.75}
    for tag in ("i16", "u8"):
        c = ZBY["%s_9x5_to_17x17" % tag]
        half, negative = G.half_ties(c["vol"], 17, 17)
        assert [half, negative] == c["ties"].tolist() and half >= 100, c["name"]
        if tag == "i16":
            assert negative >= 20 and c["vol"].min() < 0 < c["vol"].max()
            # half away from zero, decided on the ties themselves: -2.5 -> -3, 2.5 -> 3
            acc = G.accumulator(c["vol"], 17, 17)
            tie = np.abs(acc - np.trunc(acc)) == 0.5
            assert np.array_equal(c["scipy"][tie], (acc[tie] + np.where(acc[tie] > 0, 0.5, -0.5)).astype(np.int16))
            assert np.count_nonzero(c["scipy"][tie] != np.rint(acc[tie])) >= 20, "round half to even would give other values"
    assert ZBY["f32_9x5_to_17x17"]["ties"] is None
    # the lane-to-column edges, from the kernel's own constants: a lane owns four columns, a workgroup has kThreads lanes
    threads, band = _constant("kThreads"), _constant("kBandRows")
    assert (threads, band) == (256, 32)
    groups = lambda ow: ((ow + 3) // 4 * 4) // 4
    assert groups(1030) == 258 > threads and groups(1028) == 257 > threads and 1028 % 4 == 0 and 1030 % 4 != 0
    assert max(groups(c["scipy"].shape[2]) for c in G.load_cases(np.load(os.path.join(GOLD, "resample.npz")))[0]) <= threads
    assert groups(1) == 1 and threads // groups(1) == 256 and (40 + band - 1) // band == 2
    # an input axis with one sample: every right / lower tap is beyond the slice; scipy repeats the one sample
    for tag, _ in G.DTYPES:
        a, b = ZBY["%s_6x1_to_9x4" % tag], ZBY["%s_1x6_to_4x9" % tag]
        assert all(np.array_equal(a["scipy"][:, :, k], a["scipy"][:, :, 0]) for k in range(4))
        assert all(np.array_equal(b["scipy"][:, k, :], b["scipy"][:, 0, :]) for k in range(4))
        assert np.array_equal(a["scipy"][:, ::8, 0], a["vol"][:, ::5, 0]) and np.array_equal(b["scipy"][:, 0, ::8], b["vol"][:, 0, ::5])
    lim = ZBY["i16_2x2_to_9x9_limits"]
    assert sorted(np.unique(lim["vol"]).tolist()) == [-32768, 32767] and lim["scipy"].min() == -32768 and lim["scipy"].max() == 32767
    acc = G.accumulator(lim["vol"], 9, 9)
    assert acc.min() - 0.5 < -32768.0 and acc.max() + 0.5 > 32767.0, "the clamp of round_int decides these values"


def test_the_label_cases_reach_the_bands_the_ties_and_the_limits_of_eight():
    band = _constant("kBandRows")
    assert _constant("kMaxClasses") == 8 == _constant("kMaxRemap")
    bands = lambda c: (_window(c)[0] + band - 1) // band
    want = {"u8_blocks8_to_267x267_crop224": (7, 224), "u8_noise8_to_70x76_crop64": (2, 64), "u8_noise8_to_70x75": (3, 75),
            "i16_noise_remap8_to_70x76_crop64": (2, 64), "u8_noise8_9x11_to_17x21": (1, 21), "u8_noise8_1x9_to_3x17": (1, 17),
            "u8_noise8_9x1_to_17x3": (1, 3), "u8_noise8_3x300_to_5x1030": (1, 1030)}
    assert sorted(want) == sorted(LBY)
    for name, (nb, ow) in want.items():
        c = LBY[name]
        assert bands(c) == nb and _window(c)[1] == ow and c["num_classes"] == 8, name
        assert c["counts"].tolist() == list(G.channel_counts(c["raw"], c["zh"], c["zw"], 8, c["remap"], c["crop"])), name
    first = G.load_cases(np.load(os.path.join(GOLD, "resample.npz")))[1]
    assert all((c["scipy"].shape[1] + band - 1) // band == 1 for c in first), "the first file never has a second band"
    blocks = LBY["u8_blocks8_to_267x267_crop224"]
    assert blocks["raw"].shape == (3, 40, 44) and blocks["raw"].dtype == np.uint8 and G.bit_equal(blocks["raw"], G.blocks8())
    assert all(len(np.unique(blocks["raw"][k, y:y + 4, x:x + 4])) == 1 for k in range(3) for y in range(0, 40, 4) for x in range(0, 44, 4))
    assert np.unique(blocks["raw"]).tolist() == list(range(8))
    assert blocks["counts"][0] >= 100 and blocks["counts"][1] >= 100
    ties = LBY["u8_noise8_9x11_to_17x21"]
    assert ties["counts"][0] >= 20 and ties["counts"][1] >= 100, "the first class whose channel rounds to 1"
    assert set(G.axis_terms(9, 17)[1].tolist()) == {0.0, 0.5} and set(G.axis_terms(11, 21)[1].tolist()) == {0.0, 0.5}
    for name in ("u8_noise8_to_70x76_crop64", "u8_noise8_to_70x75"):
        raw = LBY[name]["raw"]
        assert raw.shape == (2, 40, 44) and np.unique(raw).tolist() == list(range(8))
        quads = np.stack([raw[:, :-1, :-1], raw[:, :-1, 1:], raw[:, 1:, :-1], raw[:, 1:, 1:]], -1).reshape(-1, 4)
        distinct = np.array([len(set(q)) for q in quads.tolist()])
        # uniform classes: four distinct under 8 7 6 5 / 8^4 = 41 % of the tap squares, three or more under 90 %
        assert np.mean(distinct == 4) > 0.35 and np.mean(distinct >= 3) > 0.85, name
    # eight pairs with a chained one, negative and large raw codes, on the same noise
    r8 = LBY["i16_noise_remap8_to_70x76_crop64"]
    assert r8["raw"].dtype == np.int16 and r8["remap"] == G.REMAP8 and len(r8["remap"]) == 8
    (a, b), (b2, c2) = r8["remap"][:2]
    assert b == b2 and (a, b, c2) == (7, 200, 1) and np.count_nonzero(r8["raw"] == 7) >= 100 and np.count_nonzero(r8["raw"] == 200) >= 100
    assert np.array_equal(G.remap_rule(r8["raw"], r8["remap"]), LBY["u8_noise8_to_70x76_crop64"]["raw"])
    assert G.bit_equal(r8["scipy"], LBY["u8_noise8_to_70x76_crop64"]["scipy"]) and r8["raw"].min() < 0
    # vector stores need ow % 4 == 0
    assert [n for n, (_, ow) in sorted(want.items()) if ow % 4 == 0] == ["i16_noise_remap8_to_70x76_crop64", "u8_blocks8_to_267x267_crop224",
                                                                        "u8_noise8_to_70x76_crop64"]


def test_the_statistics_cases_reach_the_looping_reduce_the_128_bit_numerator_and_the_capped_second_pass():
    band, reduce_blocks, threads = _constant("kBandRows"), _constant("kReduceBlocks"), _constant("kThreads")
    assert (band, reduce_blocks, threads) == (32, 1024, 256)
    assert "(total + kThreads * 8 - 1) / (kThreads * 8)" in SRC and "blocks > kReduceBlocks ? blocks : kReduceBlocks" in SRC
    blocks = lambda c: c["vol"].shape[0] * ((_window(c)[0] + band - 1) // band)
    for tag, dt in G.DTYPES:
        c = SBY["%s_many_520x3x3_to_33x4" % tag]
        assert c["vol"].dtype == dt and c["vol"].shape == (520, 3, 3) and _window(c) == (33, 4) and 33 * 4 == 132
        assert blocks(c) == 1040 > reduce_blocks, "past the floor of partial_bytes"
        assert sorted({len(range(t, 1040, threads)) for t in range(threads)}) == [4, 5], "partials per lane of stats_finalize_kernel"
    first = G.load_cases(np.load(os.path.join(GOLD, "resample.npz")))[2]
    assert max(blocks(c) for c in first) == 14, "the first file: no lane of the reduce ever takes a second partial"
    full = SBY["i16_fullscale_3x32x32_to_267x267_crop224"]
    assert G.bit_equal(full["vol"], G.fullscale_volume())
    assert np.abs(full["vol"].astype(np.int64)).min() >= 28000 and (full["vol"][:, :, :14] > 0).all() and (full["vol"][:, :, 14:] < 0).all()
    n, s1, s2 = G.int_sums(G.expected_stat_arrays(full)[0])
    assert n == 3 * 224 * 224 and n * s2 - s1 * s1 >= 2 ** 64 and s1 < 0
    assert ((n * s2).bit_length(), (n * s2 - s1 * s1).bit_length(), -1) == tuple(full["bits"].tolist()) == (65, 65, -1)
    near = SBY["i16_nearconstant_4x32x32_to_267x267_crop224"]
    assert G.bit_equal(near["vol"], G.nearconstant_volume()) and np.count_nonzero(near["vol"] != 30000) == 1 and near["vol"].min() == 29999
    n, s1, s2 = G.int_sums(G.expected_stat_arrays(near)[0])
    assert n * s2 >= 2 ** 64 and ((n * s2).bit_length(), (n * s2 - s1 * s1).bit_length(), 1) == tuple(near["bits"].tolist()) == (65, 24, 1)
    assert abs(float(near["rule_stats"][1]) - 0.01497) < 1e-5
    for c in first:
        if c["vol"].dtype != np.float32:
            n1, _, q = G.int_sums(G.zoom_rule(c["vol"], c["zh"], c["zw"], c["crop"]))
            assert n1 * q < 2 ** 64, "the first file stays inside the hi == 0 shortcut of u128_to_double: %s" % c["name"]
    # the exact statistics follow the stated arithmetic on the wide numerator too: one conversion, ties to even
    num = n * s2 - s1 * s1
    assert float(near["rule_stats"][1]) == math.sqrt(float(num) / (float(n) * float(n)))
    exact = SBY["f32_exact_42x64x64_to_267x267_crop224"]
    assert "stats/%s/in" % exact["name"] not in FILE.files and exact["vol"].dtype == np.float32 and exact["vol"].shape == (42, 64, 64)
    q = exact["vol"].astype(np.float64) * 1024.0
    assert np.all(q == np.floor(q)) and q.min() >= 64 * 1024 and q.max() < 256 * 1024, "multiples of 2^-10 in [64, 256)"
    z = G.expected_stat_arrays(exact)[0]
    total = z.size
    assert total == 2107392 and (total + threads * 8 - 1) // (threads * 8) == 1029 > reduce_blocks and blocks(exact) == 294
    assert 2097152 == reduce_blocks * threads * 8 < total
    s = G.exact_sum_scaled(z)                                             # integers: the float64 sum is exact in any order
    assert float(exact["rule_stats"][0]) == float(exact["numpy_stats"][0]) == float(s) / 2.0 ** 17 / total


@pytest.mark.skipif(not _have_scipy(), reason="scipy is not installed")
def test_scipy_reproduces_the_second_file():
    assert G.check_edges_file() == len(FILE.files) - 2
    for c in STATS:
        z = G.zoom_scipy(c["vol"], c["zh"], c["zw"], c["crop"])
        assert G.sha256_hex(z) == c["sha256"], c["name"]


def test_the_design_names_the_second_fixture():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert "tests/golden/resample_edges.npz" in text and "tests/golden/resample.npz" in text
