"""Device-side photometric augmentation (csrc/photometric.hip) at the shapes where the kernels leave the
paths that tests/golden/photometric.npz reaches: more than one x tile at every C, C = 2 and 4, heights that are no multiple of
the tile, the byte-wise store of the neighbourhood kernel and the ragged tail of the pointwise one with real operators, the
two kernels disagreeing on vectorisation, misaligned `in` and `out`, images below the halo, and 224 x 224 x 1
(tests/photometric_edge_cases.py).

Expected arrays are the plain-numpy restatement of scripts/make_photometric_golden.py, computed here; before anything is
compared with one, its sha256 is compared with tests/golden/photometric_edges.json, which was written only after the scipy
backend had equalled it and no case had an excusable pixel.  The table is band-free, so every comparison is bit for bit: no
excused set and no allowance of one grey level.  Every output is a view into a buffer prefilled with 0xA5 whose bytes around
the view must stay untouched."""
import json

import numpy as np
import pytest
import torch

import photometric_edge_cases as T

pytestmark = pytest.mark.gpu

G = T.G
RECORDED = json.load(open(T.JSON_PATH))["cases"]
GUARD, FILL = 64, 0xA5
_CHECKED = set()


def _case(name):
    """the case, its recorded digest asserted once against the restatement as this machine's numpy computes it"""
    cs = T.BY_NAME[name]
    if name not in _CHECKED:
        assert T.digests_of(cs) == RECORDED[name], "the restatement here is not the one that was checked against scipy: " + name
        assert not T.expected(cs)[1].any(), name
        _CHECKED.add(name)
    return cs


def _upload(dev, cs, rows=None, slots=None):
    from pointcloududa_amd.utils.photometric import PhotoProgram, upload_program
    rows = slice(None) if rows is None else rows
    slots = slice(None) if slots is None else slots
    prog = PhotoProgram(*(np.ascontiguousarray(a[rows][:, slots]) for a in T.arrays_of(cs)))
    return upload_program(prog, prog.batch, cs.h, cs.w, cs.c, dev)


def _run(dev, images, up, out_offset=GUARD, in_offset=None):
    """K.photometric into a view at byte `out_offset` of a flat 0xA5 buffer (GUARD: 16-byte aligned); with `in_offset` the input
    is a contiguous view at that byte offset of a larger buffer.  The guard bytes stay 0xA5 and the input stays what it was"""
    from pointcloududa_amd import kernels as K
    shape, n = tuple(images.shape), images.size
    flat = torch.from_numpy(np.array(images).reshape(-1)).to(dev)            # (a copy: the table's arrays are read-only)
    if in_offset is None:
        x = flat.view(shape)
    else:
        ibuf = torch.full((n + 2 * GUARD,), 0x3C, dtype=torch.uint8, device=dev)
        ibuf[in_offset:in_offset + n] = flat
        x = ibuf[in_offset:in_offset + n].view(shape)
        assert x.is_contiguous() and x.data_ptr() == ibuf.data_ptr() + in_offset
    keep = x.clone()
    buf = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=dev)
    out = buf[out_offset:out_offset + n].view(shape)
    assert out_offset >= GUARD and buf.data_ptr() % 16 == 0 and out.is_contiguous() and out.data_ptr() % 16 == out_offset % 16
    res = K.photometric(x, *up, out=out)
    assert res.data_ptr() == out.data_ptr() and x.data_ptr() == (flat.data_ptr() if in_offset is None else ibuf.data_ptr() + in_offset)
    got = out.cpu().numpy()
    lo, hi = buf[:out_offset].cpu().numpy(), buf[out_offset + n:].cpu().numpy()
    assert len(lo) >= GUARD and len(hi) >= GUARD
    assert (lo == FILL).all() and (hi == FILL).all(), ("guard bytes written", np.flatnonzero(lo != FILL)[:5].tolist(),
                                                        np.flatnonzero(hi != FILL)[:5].tolist())
    assert torch.equal(x, keep), "the input is never written"
    return got


def _same(got, want, cs, what):
    """bit for bit; a failure names the first differing (sample, y, x, channel) with that sample's operators"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        first = np.argwhere(bad)[:6]
        where = [(tuple(int(v) for v in p), "/".join(G.NAMES[op] for op in cs.rows[p[0]]), int(got[tuple(p)]), int(want[tuple(p)]))
                 for p in first]
        per_sample = {i: int(bad[i].sum()) for i in range(len(bad)) if bad[i].any()}
        raise AssertionError("%s %s: %d bytes differ; (sample, y, x, ch), operator, got, want: %r; per sample: %r" % (
            cs.name, what, int(bad.sum()), where, per_sample))


# ---------------------------------------------------------------------------------------------- every case, exact
@pytest.mark.parametrize("name", [cs.name for cs in T.CASES])
def test_every_case_equals_the_restatement_bit_for_bit(dev, name):
    cs = _case(name)
    got = _run(dev, T.images_of(cs), _upload(dev, cs))
    _same(got, T.expected(cs)[0], cs, "aligned")


# ---------------------------------------------------------------------------------------------- misaligned pointers
@pytest.mark.parametrize("name", ("c1_two_tiles_vec", "c2_vec", "c4_vec"))
def test_misaligned_pointers_give_the_same_bytes(dev, name):
    """rows and samples are multiples of 16 here, so the pointer alone decides between the 16-byte and the byte-wise path:
    `out` one byte off, `in` a contiguous view four bytes into a larger buffer, and both; single-slot programs (the store goes
    straight to `out`) and the five-slot chain (the first slot reads the misaligned input, the last stores to `out`)"""
    for cs in (_case(name), _case("chain_" + name[:2] + "_vec")):
        assert (cs.w * cs.c) % 16 == 0 and (cs.h * cs.w * cs.c) % 16 == 0
        x, want = T.images_of(cs), T.expected(cs)[0]
        up = _upload(dev, cs)
        ref = _run(dev, x, up)
        _same(ref, want, cs, "aligned")
        for out_offset, in_offset in ((GUARD + 1, None), (GUARD, 4), (GUARD + 1, 4), (GUARD + 8, 1)):
            got = _run(dev, x, up, out_offset=out_offset, in_offset=in_offset)
            _same(got, ref, cs, "out at +%d, in at %r, against the aligned run" % (out_offset - GUARD, in_offset))


# ---------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("name", ("chain_c1", "chain_c2", "chain_c3", "chain_c4"))
def test_a_chain_equals_the_restatement_and_its_slots_one_call_at_a_time(dev, name):
    cs = _case(name)
    x, want = T.images_of(cs), T.expected(cs)[0]
    whole = _run(dev, x, _upload(dev, cs))
    _same(whole, want, cs, "five slots in one call")
    step = x
    for s in range(cs.prog.opcode.shape[1]):
        step = _run(dev, step, _upload(dev, cs, slots=slice(s, s + 1)))
    _same(step, whole, cs, "one call per slot")


# ---------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ("c3_tail", "c2_tail"))
def test_two_calls_give_identical_bytes(dev, name):
    cs = _case(name)
    up = _upload(dev, cs)
    a = _run(dev, T.images_of(cs), up)
    b = _run(dev, T.images_of(cs), up)
    assert np.array_equal(a, b)
    _same(a, T.expected(cs)[0], cs, "first call")
