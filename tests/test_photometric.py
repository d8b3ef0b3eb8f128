"""CPU checks of the device-side photometric augmentation (pointcloududa_amd/utils/photometric.py, csrc/photometric.hip;
DESIGN.md section 6, f7): the scipy restatement against the plain-numpy one (scripts/make_photometric_golden.py), the
fixture regenerating exactly, its case set and excusable share, the generator's Philox4x32-10 against a scalar one written
here, the package's encoders against the generator's, the program sampler, validation, the C declaration against the
binding, and the new kernels' ISA.  No GPU and no library load.

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
GEN = os.path.join(ROOT, "scripts", "make_photometric_golden.py")
needs_scipy = pytest.mark.skipif(importlib.util.find_spec("scipy") is None, reason="the restatement needs scipy")


def _helper():
    sys.path.insert(0, os.path.dirname(GEN))
    try:
        spec = importlib.util.spec_from_file_location("make_photometric_golden", GEN)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(os.path.dirname(GEN))
    return m


def _in_child(body):
    code = "import sys, numpy as np\nsys.path.insert(0, %r)\nimport make_photometric_golden as G\n" % os.path.dirname(GEN)
    r = subprocess.run([sys.executable, "-c", code + textwrap.dedent(body)], capture_output=True, text=True,
                       env=dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1"), timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


@needs_scipy
def test_scipy_restatement_matches_plain_numpy():
    """0 rounded mismatches on the whole case set; excusable pixels <= 1e-5 of all pixels"""
    _in_child("""
        tot, exc = G.check_restatement()
        assert tot > 1000000 and exc <= 1e-5 * tot, (tot, exc)
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
    assert os.path.getsize(os.path.join(GOLD, "photometric.npz")) < 1000 * 1000


def test_fixture_case_set():
    """every opcode alone on 64x48 and 96x80 with C = 1 and 3, its parameter corners, the three input kinds, chains of five
    slots in several orders with per_channel on and off; excusable pixels <= 1e-5 of all pixels, none for integer operators
    and none in the chains; the numpy restatement reproduces the stored images without scipy"""
    G = _helper()
    cs = G.load_cases(np.load(os.path.join(GOLD, "photometric.npz")))
    single = [c for c in cs if not c["chain"]]
    for op in range(1, 12):
        got = {(c["h"], c["w"], c["c"]) for c in single if set(np.unique(c["opcode"])) == {op}}
        assert got == {(64, 48, 1), (64, 48, 3), (96, 80, 1), (96, 80, 3)}, (op, got)
    assert {c["kind"] for c in cs} == {"random", "smooth", "grey3"}

    def params(op, what):
        return np.concatenate([what(c)[c["opcode"] == op] for c in single])
    assert set(params(G.AVERAGE_BLUR, lambda c: c["iarg"][..., 0])) >= {2, 7}
    assert set(params(G.MEDIAN_BLUR, lambda c: c["iarg"][..., 0])) >= {3, 11}
    assert set(params(G.GAUSSIAN_BLUR, lambda c: c["iarg"][..., 0])) >= {1, 12}
    assert set(params(G.ADD, lambda c: c["iarg"][..., 0])) >= {-10, 10}
    for op in (G.GAUSSIAN_NOISE, G.DROPOUT, G.COARSE_DROPOUT):
        assert set(params(op, lambda c: c["iarg"][..., 0])) == {0, 1}, op
        assert len(set(params(op, lambda c: c["seed_arr"]))) > 4
    for op, lo, hi in ((G.GAUSSIAN_NOISE, 0.0, 12.75), (G.DROPOUT, 0.01, 0.1), (G.COARSE_DROPOUT, 0.03, 0.15),
                       (G.MULTIPLY, 0.5, 1.5), (G.GRAYSCALE, 0.0, 1.0)):
        v = params(op, lambda c: c["farg"][..., 0])
        assert lo <= v.min() <= lo + 0.02 * (hi - lo) and hi - 0.02 * (hi - lo) <= v.max() <= hi, (op, v.min(), v.max())
        assert not np.any(v == np.round(v, 3)), "continuous parameters come from seeded ranges, not round values"
    chains = [c for c in cs if c["chain"]]
    assert len(chains) >= 3 and all(c["opcode"].shape[1] == 5 and np.all(c["opcode"] != 0) for c in chains)
    orders = {tuple(row) for c in chains for row in c["opcode"]}
    assert len(orders) >= 10 and set(np.concatenate([c["opcode"].ravel() for c in chains])) == set(range(1, 12))
    pc = np.concatenate([c["iarg"][..., 0][np.isin(c["opcode"], (5, 6, 7))] for c in chains])
    assert set(pc) == {0, 1}
    pixels = sum(c["u8"].size for c in cs)
    assert pixels > 1000000 and sum(len(c["exc"]) for c in cs) <= 1e-5 * pixels
    for c in cs:
        if c["chain"] or np.all(np.isin(c["opcode"], G.INTEGER_OPS)):
            assert len(c["exc"]) == 0, c["name"]
    for c in cs[::5] + chains:
        out, exc = G.run_program(G.case_inputs(c), c["opcode"], c["iarg"], c["farg"], c["seed_arr"], backend="numpy")
        keep = ~exc
        assert np.array_equal(out[keep], c["u8"][keep]) and np.abs(out.astype(int) - c["u8"]).max() <= 1, c["name"]


# ---------------------------------------------------------------------------------------------- Philox4x32-10
def _philox_scalar(key, counter):
    """Philox4x32-10 on plain Python integers: written from the round description, not from the generator's code"""
    mask = (1 << 32) - 1
    k = [key & mask, key >> 32]
    c = [counter, 0, 0, 0]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + 0x9E3779B9) & mask, (k[1] + 0xBB67AE85) & mask]
        prod0, prod1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(prod1 >> 32) ^ c[1] ^ k[0], prod1 & mask, (prod0 >> 32) ^ c[3] ^ k[1], prod0 & mask]
    return c


def test_vectorised_philox_matches_a_scalar_implementation():
    G = _helper()
    rng = np.random.default_rng(3)
    keys = [0, 1, (1 << 64) - 1, 0xFFFFFFFF, 1 << 32] + [int(v) for v in rng.integers(0, 2 ** 64, 15, dtype=np.uint64)]
    counters = np.concatenate([[0, 1, 2, 2 ** 32 - 1, 2 ** 31], rng.integers(0, 2 ** 32, 15)]).astype(np.uint32)
    n = 0
    for key in keys:
        got = G.philox4x32_10(key, counters)
        assert all(g.dtype == np.uint32 for g in got)
        for j, ctr in enumerate(counters):
            assert [int(g[j]) for g in got] == _philox_scalar(key, int(ctr)), (key, int(ctr))
            n += 1
    assert n >= 400
    # the words look uniform and the normal draws standard (a transcription error in a constant shows here)
    x0, x1, x2, x3 = G.philox4x32_10(keys[7], np.arange(200000, dtype=np.uint32))
    for x in (x0, x1, x2, x3):
        assert abs(x.astype(np.float64).mean() / 2 ** 32 - 0.5) < 4 / np.sqrt(12 * 200000)
    z = G.normal_draws(keys[8], np.arange(200000, dtype=np.uint32))
    assert abs(z.mean()) < 4 / np.sqrt(200000) and abs(z.std() - 1) < 0.01 and np.all(np.isfinite(z))


# ---------------------------------------------------------------------------------------------- the package's encoders
def test_package_encoders_match_the_generators():
    from pointcloududa_amd.utils import photometric as P
    G = _helper()
    assert [getattr(P, "OP_" + n.upper()) for n in G.NAMES] == list(range(12))
    for sigma in (0.125, 0.3, 1.0, 2.2, 3.0):
        assert np.array_equal(P.gaussian_weights(sigma), G.gaussian_weights(sigma))
    assert len(P.gaussian_weights(3.0)) == 13 and len(P.gaussian_weights(0.1249)) == 1
    assert np.array_equal(P.sharpen_weights(0.3, 1.2), G.sharpen(0.3, 1.2)) and np.array_equal(P.emboss_weights(0.7, 1.9), G.emboss(0.7, 1.9))
    assert np.array_equal(P.sharpen_weights(1, 1), [[-1, -1, -1], [-1, 9, -1], [-1, -1, -1]])
    assert np.array_equal(P.emboss_weights(1, 1), [[-2, -1, 0], [-1, 1, 1], [0, 1, 2]])
    assert np.array_equal(P.sharpen_weights(0, 1.3), [[0, 0, 0], [0, 1, 0], [0, 0, 0]])
    rng = np.random.default_rng(8)
    setters = {G.GAUSSIAN_BLUR: "set_gaussian_blur", G.AVERAGE_BLUR: "set_average_blur", G.MEDIAN_BLUR: "set_median_blur",
               G.CONV3X3: "set_conv3x3", G.GAUSSIAN_NOISE: "set_gaussian_noise", G.DROPOUT: "set_dropout",
               G.COARSE_DROPOUT: "set_coarse_dropout", G.INVERT: "set_invert", G.ADD: "set_add", G.MULTIPLY: "set_multiply",
               G.GRAYSCALE: "set_grayscale"}
    for op, name in setters.items():
        slots = G.corner_slots(op, rng) + [G.random_slot(op, rng) for _ in range(3)]
        want, got = G.Prog(len(slots), 1), P.PhotoProgram.identity(len(slots), 1)
        for i, kw in enumerate(slots):
            want.put(i, 0, op, **kw)
            getattr(got, name)(i, 0, **kw)
        got.validate(3)
        for f in ("opcode", "iarg", "farg", "seed"):
            a, b = getattr(got, f), getattr(want, f)
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, f)
    # sigma below the threshold is a NOP; the kernel's view: thresholds and coarse grids
    p = P.PhotoProgram.identity(3, 1)
    p.set_gaussian_blur(0, 0, 0.12)
    assert p.is_identity()
    p.set_dropout(1, 0, 0.1, True, 5)
    p.set_coarse_dropout(2, 0, 0.15, 0.05, False, (1 << 64) - 1)
    assert not p.is_identity()
    op, ia, fa, sd = p.kernel_arrays(96, 80, 3)
    assert ia.dtype == np.int32 and sd.dtype == np.int64 and sd[2, 0] == -1 and op is p.opcode
    assert ia[1, 0, 1] == int(np.floor(0.1 * 2.0 ** 32)) and ia[2, 0, 1] == int(np.floor(0.15 * 2.0 ** 32))
    assert tuple(ia[2, 0, 2:]) == (5, 4) and tuple(p.iarg[2, 0, 1:]) == (0, 0, 0)
    assert P.dropout_threshold(1.0) == 2 ** 32 - 1 and P.dropout_threshold(0.0) == 0 and P.coarse_grid(0.02, 20, 256) == (1, 5)


# ---------------------------------------------------------------------------------------------- sample_program
def test_sample_program_slots_ranges_and_frequencies():
    from pointcloududa_amd.utils import photometric as P
    n = 20000
    prog = P.sample_program(n, "mscmrseg_aug2_photometric", np.random.default_rng(5))
    prog.validate(3)
    op, ia, fa = prog.opcode, prog.iarg, prog.farg
    assert op.shape == (n, 5) and prog.seed.dtype == np.uint64
    active = (op != 0).sum(1)
    assert active.max() == 5 and active.min() == 0
    p = 2.5 / 9                                   # a uniform count 0..5 of nine entries
    tol = lambda q, m=1: 4 * np.sqrt(m * q * (1 - q / m) / n)
    sig_nop = 0.125 / 3.0                         # sigma below the threshold is encoded as NOP
    freq = {c: (op == c).sum() / n for c in range(12)}
    for code, want in ((P.OP_GAUSSIAN_BLUR, p / 3 * (1 - sig_nop)), (P.OP_AVERAGE_BLUR, p / 3), (P.OP_MEDIAN_BLUR, p / 3),
                       (P.OP_GAUSSIAN_NOISE, p), (P.OP_DROPOUT, p / 2), (P.OP_COARSE_DROPOUT, p / 2), (P.OP_INVERT, p),
                       (P.OP_ADD, p), (P.OP_MULTIPLY, p), (P.OP_GRAYSCALE, p)):
        assert abs(freq[code] - want) <= tol(want), (P.OP_NAMES[code], freq[code], want)
    assert abs(freq[P.OP_CONV3X3] - 2 * p) <= tol(2 * p, 2)
    # the slot count is uniform up to the Gaussians that became NOPs
    cnt = np.bincount(active, minlength=6) / n
    assert np.all(np.abs(cnt - 1 / 6) < 0.02)

    def sel(code):
        m = op == code
        return ia[m], fa[m]
    i, f = sel(P.OP_GAUSSIAN_BLUR)
    assert i[:, 0].min() == 1 and i[:, 0].max() == 12 and 0.125 <= f[:, 15].min() < 0.2 and 2.95 < f[:, 15].max() <= 3.0
    assert np.array_equal(i[:, 0], (4 * f[:, 15] + 0.5).astype(int))
    i, f = sel(P.OP_AVERAGE_BLUR)
    assert set(i[:, 0]) == {2, 3, 4, 5, 6, 7}
    i, f = sel(P.OP_MEDIAN_BLUR)
    assert set(i[:, 0]) == {3, 5, 7, 9, 11}
    i, f = sel(P.OP_GAUSSIAN_NOISE)
    assert 0 <= f[:, 0].min() < 0.2 and 12.6 < f[:, 0].max() <= 12.75 and abs(i[:, 0].mean() - 0.5) < 4 * 0.5 / np.sqrt(len(i))
    i, f = sel(P.OP_DROPOUT)
    assert 0.01 <= f[:, 0].min() < 0.012 and 0.098 < f[:, 0].max() <= 0.1 and abs(i[:, 0].mean() - 0.5) < 4 * 0.5 / np.sqrt(len(i))
    i, f = sel(P.OP_COARSE_DROPOUT)
    assert 0.03 <= f[:, 0].min() < 0.033 and 0.147 < f[:, 0].max() <= 0.15 and 0.02 <= f[:, 1].min() and f[:, 1].max() <= 0.05
    assert abs(i[:, 0].mean() - 0.2) < 4 * 0.4 / np.sqrt(len(i))
    i, f = sel(P.OP_INVERT)
    bits = np.array([(i[:, 0] >> ch) & 1 for ch in range(4)])
    assert np.all(np.abs(bits.mean(1) - 0.05) < 4 * np.sqrt(0.05 * 0.95 / len(i)))
    i, f = sel(P.OP_ADD)
    assert i.min() == -10 and i.max() == 10 and abs(np.all(i == i[:, :1], axis=1).mean() - (0.5 + 0.5 / 21 ** 3)) < 0.03
    i, f = sel(P.OP_MULTIPLY)
    assert 0.5 <= f[:, :4].min() < 0.51 and 1.49 < f[:, :4].max() <= 1.5 and abs(np.all(f[:, :4] == f[:, :1], axis=1).mean() - 0.5) < 0.03
    i, f = sel(P.OP_GRAYSCALE)
    assert 0 <= f[:, 0].min() < 0.01 and 0.99 < f[:, 0].max() <= 1
    i, f = sel(P.OP_CONV3X3)
    sharp = f[:, 0] == f[:, 8]                    # sharpen is symmetric, emboss is not
    assert abs(sharp.mean() - 0.5) < 0.03 and np.all(f[:, 9:] == 0)
    rnd = np.isin(op, (P.OP_GAUSSIAN_NOISE, P.OP_DROPOUT, P.OP_COARSE_DROPOUT))
    assert len(np.unique(prog.seed[rnd])) == rnd.sum() and not prog.seed[~rnd].any()


def test_sample_program_is_deterministic_and_draws_one_order_per_batch():
    from pointcloududa_amd.utils import photometric as P
    from pointcloududa_amd.utils.augment import AugmentedBatches, sample_params, sample_program
    assert sample_program is P.sample_program
    a = sample_program(9, P.PHOTOMETRIC_PRESET, np.random.default_rng(11))
    b = sample_program(9, P.PHOTOMETRIC_PRESET, np.random.default_rng(11))
    for k in ("opcode", "iarg", "farg", "seed"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.batch == 9 and a.slots == 5

    def entry(code, farg):                         # opcode -> which of the nine entries it came from
        return {1: 0, 2: 0, 3: 0, 5: 3, 6: 4, 7: 4, 8: 5, 9: 6, 10: 7, 11: 8}.get(code, 1 if farg[0] == farg[8] else 2)
    rng = np.random.default_rng(12)
    for _ in range(20):                            # within a batch, two entries always come in the same relative order
        prog = sample_program(64, P.PHOTOMETRIC_PRESET, rng)
        before = set()
        for i in range(64):
            e = [entry(int(c), prog.farg[i, s]) for s, c in enumerate(prog.opcode[i]) if c]
            before |= {(x, y) for j, x in enumerate(e) for y in e[j + 1:]}
        assert not any((y, x) in before for x, y in before)
    with pytest.raises(NotImplementedError, match="heavy pipeline .* is out of scope"):
        sample_program(4, "heavy", np.random.default_rng(0))
    with pytest.raises(NotImplementedError, match="heavy pipeline .* is out of scope"):
        sample_params(4, "heavy", np.random.default_rng(0))
    with pytest.raises(NotImplementedError, match="out of scope"):
        AugmentedBatches(iter(()), None, "heavy", np.random.default_rng(0))
    with pytest.raises(ValueError, match="preset"):
        sample_program(4, "mscmrseg_simple", np.random.default_rng(0))
    with pytest.raises(ValueError, match="photometric preset"):
        AugmentedBatches(iter(()), None, "mscmrseg_simple", np.random.default_rng(0), rescale="div255", photometric_preset="aug2")
    with pytest.raises(TypeError, match="uint8"):
        AugmentedBatches(iter(()), None, "mscmrseg_simple", np.random.default_rng(0), photometric_preset=P.PHOTOMETRIC_PRESET)


# ---------------------------------------------------------------------------------------------- validate
def test_programs_are_validated_on_the_host():
    import torch
    from pointcloududa_amd.utils import photometric as P

    def one(setter, *args):
        p = P.PhotoProgram.identity(2, 2)
        getattr(p, setter)(1, 1, *args)
        return p
    assert P.PhotoProgram.identity(3, 0).is_identity() and P.PhotoProgram.identity(3).slots == 5
    P.PhotoProgram.identity(3, 8).validate()
    good = one("set_grayscale", 0.5)
    good.validate(); good.validate(3); good.validate(1)
    for c in (2, 4):
        with pytest.raises(ValueError, match="GRAYSCALE takes 3 channels"):
            good.validate(c)
    with pytest.raises(ValueError, match="channels"):
        P.PhotoProgram.identity(1).validate(5)
    bad = []
    p = one("set_average_blur", 4); p.opcode[0, 0] = 12; bad.append((p, "unknown opcode"))
    p = one("set_average_blur", 4); p.opcode[0, 0] = -1; bad.append((p, "unknown opcode"))
    bad += [(one("set_average_blur", k), "AVERAGE_BLUR k") for k in (1, 8)]
    bad += [(one("set_median_blur", k), "MEDIAN_BLUR k") for k in (1, 4, 13)]
    p = one("set_gaussian_blur", 2.0); p.iarg[1, 1, 0] = 13; bad.append((p, "radius"))
    p = one("set_gaussian_blur", 2.0); p.iarg[1, 1, 0] = 0; bad.append((p, "radius"))
    p = one("set_gaussian_blur", 2.0); p.farg[1, 1, 1] *= 1.5; bad.append((p, "weights"))
    p = one("set_conv3x3", np.ones(9)); p.farg[1, 1, 4] = np.nan; bad.append((p, "finite"))
    bad += [(one("set_gaussian_noise", s, True, 1), "scale") for s in (-1.0, 300.0)]
    p = one("set_gaussian_noise", 3.0, True, 1); p.iarg[1, 1, 0] = 2; bad.append((p, "per_channel"))
    bad += [(one("set_dropout", q, False, 1), "DROPOUT p") for q in (-0.1, 1.5)]
    bad += [(one("set_coarse_dropout", 0.1, sp, False, 1), "size_percent") for sp in (0.0, 1.5)]
    p = one("set_invert", (1, 1, 1, 1)); p.iarg[1, 1, 0] = 16; bad.append((p, "INVERT"))
    bad += [(one("set_add", v), "ADD") for v in (256, -300)]
    bad += [(one("set_multiply", v), "MULTIPLY") for v in (-0.5, 1000.0)]
    bad += [(one("set_grayscale", v), "alpha") for v in (-0.1, 1.1)]
    p = P.PhotoProgram.identity(2, 9); bad.append((p, "slots"))
    p = P.PhotoProgram.identity(2, 2); p.iarg = p.iarg.astype(np.int64); bad.append((p, "iarg"))
    p = P.PhotoProgram.identity(2, 2); p.farg = p.farg[:, :, :9]; bad.append((p, "farg"))
    p = P.PhotoProgram.identity(2, 2); p.seed = p.seed.astype(np.int64); bad.append((p, "seed"))
    p = P.PhotoProgram.identity(2, 2); p.opcode = p.opcode.astype(np.int64); bad.append((p, "opcode"))
    for p, what in bad:
        with pytest.raises(ValueError, match=what):
            p.validate(3)
    with pytest.raises(TypeError, match="program is required"):
        P.photometric_aug(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match="uint8"):
        P.photometric_aug(torch.zeros(1, 4, 4, 3), P.PhotoProgram.identity(1))
    with pytest.raises(ValueError, match="batch"):
        P.upload_program(P.PhotoProgram.identity(2), 3, 8, 8, 3, torch.device("cpu"))


# ---------------------------------------------------------------------------------------------- C ABI, ISA
def test_header_declares_what_the_binding_binds():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p}
    for name, ret in (("pcuda_photometric", "int"), ("pcuda_photometric_workspace_size", "size_t")):
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (s.strip() for s in m.group(2).split(","))]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
    m = re.search(r"int pcuda_photometric\(([^;]*)\);", hdr)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "in", "out", "b", "h", "w", "c", "slots", "opcode", "iarg", "farg", "seed", "workspace", "workspace_bytes", "s"]
    from pointcloududa_amd.utils import photometric as P
    for n in P.OP_NAMES:
        assert re.search(r"#define PCUDA_PHOTO_%s %d\b" % (n, getattr(P, "OP_" + n)), hdr), n
    assert "photometric.hip" in open(os.path.join(CSRC, "Makefile")).read()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_photometric_kernels_keep_load_addresses_alive():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=photometric.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "photometric.s"]
    assert len(rows) >= 2, "expected the pointwise and the neighbourhood kernel in the assembly"
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
    text = open(os.path.join(CSRC, "build", "isa", "photometric.s")).read()
    assert "global_store_dwordx4" in text, "the 16-byte stores are gone"
