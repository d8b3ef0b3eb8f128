"""Pins the host-side decisions of the 2-D convolution dispatch (csrc/conv_igemm.hip): packed buffer sizes, tile counts
and the job records of the batched repack, for a fixed list of geometries, both precisions, with and without the small-map
knobs the kernel tests set.  Writes tests/golden/conv_host_plan.json; tests/test_conv_host_plan.py compares a build to it.

Run it on the build whose behaviour is to be kept (the PARENT of a refactor), never on the commit under test:

    python scripts/make_conv_host_golden.py

Everything recorded is pure host code: nothing is launched and no device is needed.  Without a device the compute-unit
count the map thresholds use falls back to 256, which is the MI355X's own count, so the fixture holds on both kinds of
machine.  The pointers handed to pcuda_conv2d_pack_jobs_fill are fixed fake addresses; they are only stored."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "conv_host_plan.json")

IG_MAX_TAPS = 36
W_PTR, FWD_PTR, DGRAD_PTR = 0x100000000000, 0x200000000000, 0x300000000000
MAX_JOBS = 64
KNOBS = {"default": {}, "small_maps": {"PCUDA_AP_MIN_ITEMS": "0", "PCUDA_RS_MIN_ROWS": "2", "PCUDA_RS_MIN_ITEMS": "0"}}
JOB_FIELDS = ("w", "out", "rec", "rows", "red", "s_row", "s_red", "ntaps", "tap_src", "pair", "co_tile", "nchunks", "n_co_tiles")


class PackParams(C.Structure):      # struct PackParams, csrc/conv_igemm.h
    _fields_ = [("w", C.c_void_p), ("out", C.c_void_p), ("rec", C.c_int), ("rows", C.c_int), ("red", C.c_int),
                ("s_row", C.c_longlong), ("s_red", C.c_longlong), ("ntaps", C.c_int), ("tap_src", C.c_byte * IG_MAX_TAPS),
                ("pair", C.c_int), ("co_tile", C.c_int), ("nchunks", C.c_int), ("n_co_tiles", C.c_int)]


def _g(n, cin, cout, h, w, k, s=1, p=None, d=1, up=0):
    """(n, cin, cout, in_h, in_w, k, stride, pad, dil, in_up); pad defaults to 'same' for stride 1"""
    return (n, cin, cout, h, w, k, s, d * (k - 1) // 2 if p is None else p, d, up)


GEOMS = [
    # 1-channel 3x3: the direct layer, and maps it does not take (row length not 4k)
    _g(4, 1, 32, 64, 64, 3), _g(2, 1, 64, 16, 16, 3), _g(2, 1, 32, 29, 29, 3), _g(32, 1, 32, 256, 256, 3),
    # 1x1: cout <= 8 (direct), above, cin > 64, h * w not 4k
    _g(4, 32, 4, 64, 64, 1), _g(4, 32, 5, 64, 64, 1), _g(2, 64, 8, 16, 16, 1), _g(4, 32, 16, 64, 64, 1),
    _g(2, 96, 8, 16, 16, 1), _g(2, 32, 4, 5, 5, 1), _g(1, 16, 8, 16, 16, 1),
    # k4 / s2 / p2, cin <= 5: the four-class image and the d1 / d5 kernels, odd and even maps
    _g(4, 4, 64, 129, 129, 4, 2, 2), _g(4, 5, 64, 128, 128, 4, 2, 2), _g(4, 1, 64, 65, 65, 4, 2, 2), _g(4, 4, 32, 33, 33, 4, 2, 2),
    _g(2, 5, 16, 17, 17, 4, 2, 2), _g(2, 4, 8, 11, 14, 4, 2, 2), _g(1, 3, 8, 5, 1, 4, 2, 2), _g(16, 4, 64, 256, 256, 4, 2, 2),
    _g(4, 2, 62, 64, 64, 4, 2, 2),
    # k4 / s2 / p2, cin > 5: the paired column classes
    _g(4, 64, 128, 65, 65, 4, 2, 2), _g(4, 128, 256, 33, 33, 4, 2, 2), _g(4, 256, 512, 17, 17, 4, 2, 2), _g(2, 24, 40, 11, 14, 4, 2, 2),
    _g(1, 8, 8, 5, 1, 4, 2, 2), _g(4, 64, 128, 64, 64, 4, 2, 2), _g(16, 64, 128, 129, 129, 4, 2, 2), _g(2, 6, 16, 16, 16, 4, 2, 2),
    # other strides: k3 / s2 / p1, stride 3 (the one-launch-per-layout repack), classes without taps
    _g(2, 16, 32, 32, 32, 3, 2, 1), _g(2, 16, 32, 33, 33, 3, 2, 1), _g(2, 8, 8, 16, 16, 3, 3, 1), _g(1, 8, 16, 20, 52, 3, 3, 1),
    _g(2, 16, 16, 16, 16, 1, 2, 0), _g(2, 8, 8, 17, 17, 2, 3, 0),
    # anti-phase layers on maps the kernel takes and on maps it does not; an odd tile count; channel counts it does not take
    _g(32, 64, 64, 32, 32, 3), _g(1, 64, 64, 32, 32, 3), _g(32, 128, 64, 32, 32, 3), _g(1, 128, 64, 32, 32, 3),
    _g(32, 256, 256, 32, 32, 3), _g(1, 256, 256, 32, 32, 3), _g(1, 64, 64, 24, 32, 3), _g(3, 64, 64, 8, 32, 3),
    _g(32, 64, 64, 20, 52, 3), _g(32, 64, 64, 29, 29, 3), _g(16, 64, 128, 128, 128, 3), _g(8, 128, 128, 64, 64, 3),
    _g(32, 64, 32, 256, 256, 3), _g(4, 24, 64, 32, 32, 3), _g(4, 64, 96, 32, 32, 3), _g(2, 1024, 64, 8, 32, 3),
    _g(16, 512, 512, 16, 16, 3), _g(16, 256, 512, 16, 32, 3),
    # 32 -> 32 3x3: row-streaming at 256 x 256 with n = 32, not at 64 x 64 with n = 1
    _g(32, 32, 32, 256, 256, 3), _g(1, 32, 32, 64, 64, 3), _g(32, 32, 32, 64, 64, 3), _g(8, 32, 32, 128, 128, 3),
    _g(4, 32, 32, 256, 250, 3),
    # layers behind the nearest-x2 fold
    _g(8, 32, 32, 64, 64, 3, up=1), _g(8, 128, 64, 64, 64, 3, up=1), _g(32, 128, 64, 32, 32, 3, up=1),
    _g(8, 64, 32, 128, 128, 3, up=1), _g(2, 96, 32, 256, 256, 3, up=1),
    # dilation, large kernels (6 x 6 = IG_MAX_TAPS taps; 7 x 7 is refused)
    _g(4, 16, 16, 32, 32, 3, d=2), _g(4, 64, 64, 32, 32, 3, d=4), _g(2, 32, 32, 64, 64, 3, d=2),
    _g(2, 8, 8, 16, 16, 6, 1, 2), _g(2, 8, 16, 16, 16, 6, 2, 2), _g(2, 16, 16, 20, 20, 5), _g(2, 8, 8, 16, 16, 7),
    # ragged maps, ordinary layers
    _g(4, 32, 32, 20, 52, 3), _g(4, 32, 64, 29, 29, 3), _g(4, 16, 32, 20, 52, 3), _g(2, 48, 48, 29, 29, 3),
    _g(8, 16, 32, 64, 64, 3), _g(8, 32, 16, 128, 128, 3), _g(2, 8, 16, 16, 16, 3), _g(2, 3, 32, 64, 64, 3),
    # inconsistent geometry
    (0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
]
assert len(GEOMS) >= 60 and len(set(GEOMS)) == len(GEOMS)


def geom_struct(t):
    from pointcloududa_amd._lib import ConvGeom
    n, cin, cout, h, w, k, s, p, d, up = t
    oh = (h + 2 * p - d * (k - 1) - 1) // s + 1 if s > 0 else 0
    ow = (w + 2 * p - d * (k - 1) - 1) // s + 1 if s > 0 else 0
    return ConvGeom(n, cin, cout, h, w, oh, ow, k, s, p, d, up)


def _jobs(lib, g, prec, dgrad_ptr):
    assert C.sizeof(PackParams) == lib.pcuda_conv2d_pack_job_bytes(), "the ctypes mirror of PackParams is out of date"
    jobs = (PackParams * MAX_JOBS)()
    blocks = (C.c_int * MAX_JOBS)()
    nj = lib.pcuda_conv2d_pack_jobs_fill(C.byref(g), prec, W_PTR, FWD_PTR, dgrad_ptr, jobs, MAX_JOBS, blocks)
    rec = {"n": nj, "blocks": [blocks[i] for i in range(max(nj, 0))], "jobs": []}
    for i in range(max(nj, 0)):
        j = jobs[i]
        row = []
        for f in JOB_FIELDS:      # (tap_src past ntaps * (1 + pair) is not part of the record: no kernel reads it)
            row.append([j.tap_src[t] for t in range(j.ntaps * (1 + j.pair))] if f == "tap_src" else (getattr(j, f) or 0))
        rec["jobs"].append(row)
    return rec


def record(lib):
    """the whole record of one build, as the fixture stores it"""
    out = {}
    saved = {k: os.environ.get(k) for kn in KNOBS.values() for k in kn}
    try:
        for kname, kn in KNOBS.items():
            for k in saved:
                os.environ.pop(k, None)
            os.environ.update(kn)
            for prec in (0, 1):
                rows = []
                for t in GEOMS:
                    g = geom_struct(t)
                    rows.append({
                        "fwd_bytes": lib.pcuda_conv2d_packed_fwd_bytes(C.byref(g), prec),
                        "dgrad_bytes": lib.pcuda_conv2d_packed_dgrad_bytes(C.byref(g), prec),
                        "fwd_tiles": lib.pcuda_conv2d_fwd_tiles(C.byref(g), prec),
                        "dgrad_tiles": lib.pcuda_conv2d_dgrad_tiles(C.byref(g), prec),
                        "jobs_fwd": _jobs(lib, g, prec, None),
                        "jobs_all": _jobs(lib, g, prec, DGRAD_PTR),
                    })
                out["%s/prec%d" % (kname, prec)] = rows
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


def main():
    sys.path.insert(0, ROOT)
    from pointcloududa_amd import _lib
    doc = {"note": "host decisions of csrc/conv_igemm.hip on the parent of the host-dispatch refactor "
                   "(scripts/make_conv_host_golden.py); no device: the compute-unit count falls back to 256 = the MI355X's",
           "job_fields": list(JOB_FIELDS), "geoms": [list(t) for t in GEOMS], "records": record(_lib.lib())}
    with open(OUT, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s: %d geometries, %d bytes" % (OUT, len(GEOMS), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
