"""The case table of the photometric edge tests (tests/test_photometric_edges.py, tests/test_photometric_edges_gpu.py) and of
``scripts/make_photometric_golden.py --edges``: plain data plus seeded input builders, numpy and the generator's restatement only.

tests/golden/photometric.npz stops at 96 x 80 and C in {1, 3}, all of its rows and samples multiples of 16 bytes;
csrc/photometric.hip picks its path from the shape and the channel count (the tile is 16 rows x ``twpx`` pixels, twpx = 64 at
C = 3 and 256 / C otherwise; 16-byte stores of the neighbourhood kernel iff W C % 16 == 0, of the pointwise kernel iff
H W C % 16 == 0; halo up to 12).  Every shape below is the smallest at which one of those paths is first reached:

  c1_two_tiles_tail   17 x 257 x 1   C = 1 tiles_x = 2 with a one-pixel second tile, a one-row second y tile, byte stores, a
                                     second pointwise block (4369 elements = 274 lanes) whose last lane holds one element
  c1_two_tiles_vec    16 x 272 x 1   a partial second x tile (16 pixels = one chunk) on the 16-byte store path
  c2_tail             18 x 129 x 2   C = 2 (twpx = 128, 304-byte staged rows), two x tiles, ragged rows, byte stores
  c2_vec              16 x 136 x 2   C = 2, 16-byte stores
  c3_tail             17 x 65 x 3    C = 3 with a one-pixel second tile, ragged rows, byte stores (195-byte rows); the pointwise
                                     tail's last lane ends inside the last pixel (GRAYSCALE's pixel clamp)
  c3_three_y_tiles    33 x 70 x 3    a middle y tile (rows 16..31) whose halo is all interior along y for r = 1 (the 3x3, k = 2
                                     and 3, the narrow Gaussian) and reflects off the bottom alone for r > 1; a one-row last tile
  c4_tail             19 x 65 x 4    C = 4 (352-byte staged rows), 260-byte rows: byte stores
  c4_vec              16 x 68 x 4    C = 4, 16-byte stores
  flags_disagree      2 x 40 x 3     H W C % 16 == 0 with W C % 16 == 8: pointwise vectorised, neighbourhood byte-wise
  tiny_c1 .. tiny_c4  5 x 7 x C      H and W below the halo: reflect101 wraps more than once, the replicate clamp with k = 11
  one_row, one_col    1 x 9 x 1, 9 x 1 x 3   the n == 1 branch of reflect101 on either axis
  three_by_three_c4, one_pixel   3 x 3 x 4, 1 x 1 x 1   a window larger than the image on both axes
  production_grey     224 x 224 x 1  the MS-CMRSeg crop size at C = 1: fourteen y tiles, one x tile

A case of kind "ops" is a batch of single-slot programs, one sample per (opcode, parameter corner of ``G.corner_slots``), opcodes
1..11 in order (GRAYSCALE left out at C = 2 and 4, where the host rejects it): 33 or 30 samples.  With H W C % 16 != 0 the
samples behind the first also start on misaligned addresses.  Every sample has random uint8 content of its own, every channel
from a seed of its own; the last corner of each of the four blur opcodes runs on a smooth field instead, so each blur sees both.

A case of kind "chain" is B = 4 samples of five slots, every sample with its own operator order, two neighbourhood operators
adjacent at slots (i, i + 1) of sample i (the second reads what the first stored: workspace -> output or output -> workspace,
and in sample 3 the neighbourhood kernel stores the final result), the other three slots distinct pointwise operators.  One per
C at that C's ``*_tail`` shape, and the same programs at the ``*_vec`` shapes of C = 1, 2, 4 for the misaligned-pointer tests.

Every case is BAND-FREE: no pre-rounding value of the restatement lies within ``G.EPS`` of a rounding boundary (the generator
refuses to record digests otherwise), so the expected bytes do not depend on the last bit of log / cos / sqrt and the GPU test
demands equality."""
import hashlib
import importlib.util
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _load("make_photometric_golden")
JSON_PATH = os.path.join(ROOT, "tests", "golden", "photometric_edges.json")
LOOPS_AT_MOST = 64                     # the Python-loop twin of the neighbourhood operators runs where H W is at most this
BLURS = (G.GAUSSIAN_BLUR, G.AVERAGE_BLUR, G.MEDIAN_BLUR, G.CONV3X3)

# name, kind ("ops" / "chain"), H, W, C, seed, prog: a G.Prog, rows: per sample the tuple of its opcodes,
# smooth: the samples whose input is a smooth field
Case = namedtuple("Case", "name kind h w c seed prog rows smooth")

SHAPES = (("c1_two_tiles_tail", 17, 257, 1), ("c1_two_tiles_vec", 16, 272, 1), ("c2_tail", 18, 129, 2), ("c2_vec", 16, 136, 2),
          ("c3_tail", 17, 65, 3), ("c3_three_y_tiles", 33, 70, 3), ("c4_tail", 19, 65, 4), ("c4_vec", 16, 68, 4),
          ("flags_disagree", 2, 40, 3), ("tiny_c1", 5, 7, 1), ("tiny_c2", 5, 7, 2), ("tiny_c3", 5, 7, 3), ("tiny_c4", 5, 7, 4),
          ("one_row", 1, 9, 1), ("one_col", 9, 1, 3), ("three_by_three_c4", 3, 3, 4), ("one_pixel", 1, 1, 1),
          ("production_grey", 224, 224, 1))
CHAIN_SHAPES = (("chain_c1", "c1_two_tiles_tail"), ("chain_c2", "c2_tail"), ("chain_c3", "c3_tail"), ("chain_c4", "c4_tail"),
                ("chain_c1_vec", "c1_two_tiles_vec"), ("chain_c2_vec", "c2_vec"), ("chain_c4_vec", "c4_vec"))
SMALL = ("tiny_c1", "tiny_c2", "tiny_c3", "tiny_c4", "one_row", "one_col", "three_by_three_c4", "one_pixel")
TAILS = ("c1_two_tiles_tail", "c2_tail", "c3_tail", "c4_tail")


def digest(a):
    """sha256 of an array's bytes (C order)"""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def opcodes_for(c):
    """1..11; GRAYSCALE only where the host takes it"""
    return [op for op in range(G.GAUSSIAN_BLUR, G.GRAYSCALE + 1) if op != G.GRAYSCALE or c in (1, 3)]


# ---------------------------------------------------------------------------------------------- input builders
def random_images(b, h, w, c, seed):
    """uint8 [B,H,W,C]: every channel from a generator of its own (seed, channel), so no two channels hold the same bytes"""
    return np.stack([np.random.default_rng([seed, ch]).integers(0, 256, (b, h, w), dtype=np.uint8) for ch in range(c)], axis=-1)


def build_images(case):
    x = random_images(len(case.rows), case.h, case.w, case.c, case.seed)
    if case.smooth:
        x[list(case.smooth)] = G.make_images("smooth", len(case.smooth), case.h, case.w, case.c, case.seed + 500)
    return x


# ---------------------------------------------------------------------------------------------- the table
def _ops_case(name, h, w, c, seed):
    rng = np.random.default_rng(seed)
    slots = [(op, kw) for op in opcodes_for(c) for kw in G.corner_slots(op, rng)]
    prog = G.Prog(len(slots), 1)
    for i, (op, kw) in enumerate(slots):
        prog.put(i, 0, op, **kw)
    rows = [(op,) for op, _ in slots]
    assert [int(v) for v in prog.opcode[:, 0]] == [op for op, _ in slots], "no corner is encoded as a NOP"
    smooth = tuple(max(i for i, (op, _) in enumerate(slots) if op == blur) for blur in BLURS)
    return Case(name, "ops", h, w, c, seed, prog, rows, smooth)


def _chain_prog(c, seed):
    """B = 4, five slots: sample i holds two distinct neighbourhood operators at slots i and i + 1 and three distinct pointwise
    operators around them, drawn per sample; parameters from the reference's ranges (G.random_slot)"""
    rng = np.random.default_rng(seed)
    pointwise = [op for op in opcodes_for(c) if op not in BLURS]
    prog, rows = G.Prog(4, G.SLOTS), []
    for i in range(4):
        pair = [int(v) for v in rng.permutation(BLURS)[:2]]
        rest = [int(v) for v in rng.permutation(pointwise)[:3]]
        ops = rest[:i] + pair + rest[i:]
        for s, op in enumerate(ops):
            prog.put(i, s, op, **G.random_slot(op, rng))
        rows.append(tuple(ops))
    assert np.array_equal(prog.opcode, np.array(rows)), "no slot is encoded as a NOP"
    return prog, rows


def _cases():
    out = [_ops_case(name, h, w, c, 700 + n) for n, (name, h, w, c) in enumerate(SHAPES)]
    by = {cs.name: cs for cs in out}
    progs = {c: _chain_prog(c, 800 + c) for c in (1, 2, 3, 4)}
    for n, (name, shape) in enumerate(CHAIN_SHAPES):
        cs = by[shape]
        prog, rows = progs[cs.c]
        out.append(Case(name, "chain", cs.h, cs.w, cs.c, 900 + n, prog, rows, ()))
    return out


CASES = _cases()
BY_NAME = {cs.name: cs for cs in CASES}
assert len(BY_NAME) == len(CASES)
OPS_CASES = [cs for cs in CASES if cs.kind == "ops"]
CHAIN_CASES = [cs for cs in CASES if cs.kind == "chain"]


# ---------------------------------------------------------------------------------------------- expected values (computed once)
_CACHE = {}


def images_of(case):
    key = ("img", case.name)
    if key not in _CACHE:
        x = build_images(case)
        assert x.dtype == np.uint8 and x.shape == (len(case.rows), case.h, case.w, case.c), case.name
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def arrays_of(case):
    """(opcode, iarg, farg, seed) as G.run_program and PhotoProgram take them"""
    p = case.prog
    return p.opcode, p.iarg, p.farg, p.seed


def expected(case, backend="numpy"):
    """``G.run_program(.., backend=backend)``: (uint8 [B,H,W,C], excusable bool [B,H,W,C]), read-only and shared by all tests"""
    key = ("exp", case.name, backend)
    if key not in _CACHE:
        out, exc = G.run_program(images_of(case), *arrays_of(case), backend=backend)
        out.setflags(write=False)
        exc.setflags(write=False)
        _CACHE[key] = (out, exc)
    return _CACHE[key]


def digests_of(case):
    """what tests/golden/photometric_edges.json records of a case"""
    return {"shape": [case.h, case.w, case.c], "batch": len(case.rows), "expected": digest(expected(case)[0])}
