"""The weight-gradient pin, child process: ``python conv_wgrad_child.py <table> <records.jsonl>``.

Runs every case of CASES that belongs to one table straight through the C ABI, once as ``pcuda_conv2d_wgrad`` (the one-by-one
reduce) and once as ``pcuda_conv2d_wgrad_partial`` + ``pcuda_wgrad_reduce_batch``, for both precisions, with and without the
bias gradient, plain and accumulating, and writes one JSON line per run: the launch tag, the ``fallback_count()`` delta, the
reduce job (byte offsets of its slabs from the workspace) and the sha256 of dw / db of both forms.  Nothing is compared here:
scripts/make_conv_wgrad_golden.py records the lines on the parent of a refactor, tests/test_conv_wgrad_pin_gpu.py compares a
build to them.  The weight-gradient switches are read once per process, hence one process per table.  Stops at the first HIP
error and exits non-zero.

Inputs are integers from a counter hash scaled to multiples of 2^-8 (no library sampler takes part).
"""
import ctypes as C
import hashlib
import json
import os
import re
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TABLES = {
    "default": {},
    "w3r2": {"PCUDA_WGRAD3R": "2"},
    "generic": {"PCUDA_WGRAD3R": "0", "PCUDA_NO_WGRAD1": "1", "PCUDA_NO_WGRAD3": "1"},
}


def _c(name, n, cin, cout, h, w, k, s=1, p=None, d=1, up=0, db=(0, 1), split=0, tables=None):
    """geometry as scripts/make_conv_host_golden._g writes it (pad defaults to 'same' for stride 1) + db: the bias-gradient
    settings to run, split: channels of the first of two sources (0: one source), tables: where it runs (None: everywhere)"""
    return dict(name=name, geom=(n, cin, cout, h, w, k, s, d * (k - 1) // 2 if p is None else p, d, up), db=db, split=split,
                tables=tables)


CASES = [
    _c("c1", 2, 1, 32, 16, 16, 3),
    _c("d1", 2, 4, 8, 12, 16, 4, 2, 2),                   # (without db: the direct kernel; with db: the generic plan)
    _c("w3r", 1, 16, 32, 64, 32, 3),                      # unequal channels, 64 rows, rsplit 2
    _c("w3r_up", 1, 32, 16, 8, 32, 3, up=1),
    _c("w3", 1, 32, 128, 4, 32, 3),
    _c("w1_co1_ci1", 2, 16, 8, 4, 4, 1),
    _c("w1_co2_ci2", 2, 48, 40, 8, 8, 1),
    _c("w1_co2_ci3", 1, 96, 64, 4, 8, 1),
    _c("g_1tap", 2, 32, 8, 5, 5, 1),
    _c("g_9tap", 2, 8, 16, 10, 12, 3),
    _c("g_aligned4", 2, 8, 16, 32, 32, 3),
    _c("g_16tap", 2, 24, 40, 11, 14, 4, 2, 2),            # 16 taps in one group, eight-wave request
    _c("g_25tap", 2, 16, 16, 20, 20, 5),                  # three tap groups
    _c("g_36tap", 2, 8, 16, 16, 16, 6, 2, 2),
    _c("g_dil4", 4, 64, 64, 32, 32, 3, d=4),              # one-per-CU footprint
    _c("g_split24", 2, 48, 48, 29, 29, 3, split=24),      # second source off a 32-channel boundary: no prefetch
    _c("g_xcd", 8, 32, 16, 128, 128, 3, tables=("generic",)),   # ksplit a multiple of 8
]
assert len({c["name"] for c in CASES}) == len(CASES)

JOB_FIELDS = ("numel", "ksplit", "nkg", "ntaps", "nb", "accumulate", "partial_off", "db_partial_off")


def tag_int(tag, name):
    m = re.search(r" %s(\d+)" % name, tag)
    return int(m.group(1)) if m else None


def _is(table, case, start):
    return lambda r: r["table"] == table and r["case"] == case and r["last_kernel"].startswith(start)


# the branches the cases were chosen for: (name, predicate over one record); every one must hold for some record
REACH = [
    ("direct c1", _is("default", "c1", "direct c1 wgrad ")),
    ("direct d1 without db", lambda r: _is("default", "d1", "direct d1 wgrad ")(r) and not r["db"]),
    ("d1 geometry with db on the generic plan", lambda r: _is("default", "d1", "wgrad ")(r) and r["db"]),
    ("wgrad3r default mode, rsplit 2", lambda r: _is("default", "w3r", "wgrad3r ")(r) and " up0 " in r["last_kernel"]),
    ("wgrad3r up-convolution", lambda r: _is("default", "w3r_up", "wgrad3r ")(r) and " up1 " in r["last_kernel"]),
    ("wgrad3", _is("default", "w3", "wgrad3 ")),
    ("wgrad3r mode 2 takes the wgrad3 layer", _is("w3r2", "w3", "wgrad3r ")),
    ("wgrad1 co 1 / ci 1", lambda r: _is("default", "w1_co1_ci1", "wgrad1 ")(r) and r["last_kernel"].split(" | ")[0].endswith(" tile32x32")),
    ("wgrad1 co 2 / ci 2", lambda r: _is("default", "w1_co2_ci2", "wgrad1 ")(r) and r["last_kernel"].split(" | ")[0].endswith(" tile64x64")),
    ("wgrad1 co 2 / ci 3", lambda r: _is("default", "w1_co2_ci3", "wgrad1 ")(r) and r["last_kernel"].split(" | ")[0].endswith(" tile64x96")),
    ("third table: the wgrad3r / wgrad3 / wgrad1 layers on the generic plan",
     lambda r: r["table"] == "generic" and r["case"] in ("w3r", "w3", "w1_co2_ci2") and r["last_kernel"].startswith("wgrad ")),
] + [("generic plan: %s" % c, _is("default", c, "wgrad ")) for c in
     ("g_1tap", "g_9tap", "g_aligned4", "g_16tap", "g_25tap", "g_36tap", "g_dil4", "g_split24")] + [
    ("generic one tap", lambda r: r["case"] == "g_1tap" and r["job"]["ntaps"] == 1 and r["last_kernel"].startswith("wgrad ")),
    ("generic 36 taps", lambda r: r["case"] == "g_36tap" and r["job"]["ntaps"] == 36),
    ("generic clamp0", lambda r: r["last_kernel"].startswith("wgrad ") and " clamp0 " in r["last_kernel"]),
    ("generic clamp1", lambda r: r["last_kernel"].startswith("wgrad ") and " clamp1 " in r["last_kernel"]),
    ("generic pf 0", lambda r: r["last_kernel"].startswith("wgrad ") and tag_int(r["last_kernel"], "pf") == 0),
    ("generic pf 1", lambda r: r["last_kernel"].startswith("wgrad ") and tag_int(r["last_kernel"], "pf") == 1),
    ("generic pf 3", lambda r: r["last_kernel"].startswith("wgrad ") and tag_int(r["last_kernel"], "pf") == 3),
    ("generic eight-wave request", lambda r: r["last_kernel"].startswith("wgrad ") and (tag_int(r["last_kernel"], "pf") or 0) >= 100),
    ("no prefetch behind a split off a 32-channel boundary",
     lambda r: _is("default", "g_split24", "wgrad ")(r) and tag_int(r["last_kernel"], "pf") == 0),
    ("ksplit a multiple of 8", lambda r: _is("generic", "g_xcd", "wgrad ")(r) and tag_int(r["last_kernel"], "ksplit") >= 8 and
     tag_int(r["last_kernel"], "ksplit") % 8 == 0),
    ("a reduce with one k-group", lambda r: r["job"]["ksplit"] >= 1 and r["job"]["nkg"] == 1),
    ("a reduce with sixteen k-groups", lambda r: r["job"]["nkg"] == 16),
    ("both precisions", lambda r: r["prec"] == 1),
    ("accumulate", lambda r: r["acc"] == 1 and r["job"]["ksplit"] > 0 and r["job"]["accumulate"] == 1),
    ("no bias gradient", lambda r: not r["db"] and r["job"]["ksplit"] > 0 and r["job"]["nb"] == 0 and r["hash"]["db"] is None),
]


def missing_branches(records):
    return [name for name, pred in REACH if not any(pred(r) for r in records)]


def geom_struct(t):
    from pointcloududa_amd._lib import ConvGeom
    n, cin, cout, h, w, k, s, p, d, up = t
    return ConvGeom(n, cin, cout, h, w, (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1, k, s, p, d, up)


def cases_of(table):
    return [c for c in CASES if c["tables"] is None or table in c["tables"]]


def ints(seed, shape):
    """float32 multiples of 2^-8 in [-1, 1] from a splitmix64-style hash of (seed, index)"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    v = (z >> np.uint64(40)) % np.uint64(513)
    return ((v.astype(np.int64) - 256).astype(np.float32) / np.float32(256.0)).reshape(shape)


def _sha(t):
    return None if t is None else hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def main(table, out_path):
    import torch
    from pointcloududa_amd import _lib as L
    from pointcloududa_amd import kernels as K
    lib = L.lib()
    dev = torch.device("cuda", 0)
    with open(out_path, "w") as out:
        for ci, case in enumerate(cases_of(table)):
            n, cin, cout, h, w, k, s, p, d, up = case["geom"]
            g = geom_struct(case["geom"])
            sh, sw = (h // 2, w // 2) if up else (h, w)
            xh = ints(1000 + ci, (n, cin, sh, sw))
            c1 = case["split"] or cin
            x1 = torch.from_numpy(np.ascontiguousarray(xh[:, :c1])).to(dev)
            x2 = torch.from_numpy(np.ascontiguousarray(xh[:, c1:])).to(dev) if c1 < cin else None
            dy = torch.from_numpy(ints(2000 + ci, (n, cout, g.out_h, g.out_w))).to(dev)
            dw0 = torch.from_numpy(ints(3000 + ci, (cout, cin, k, k))).to(dev)
            db0 = torch.from_numpy(ints(4000 + ci, (cout,))).to(dev)
            src = K.make_src(x1, x2)
            sn, sc = dy.stride(0), dy.stride(1)
            ws_bytes = lib.pcuda_conv2d_wgrad_workspace_size(C.byref(g))
            for prec in (0, 1):
                for with_db in case["db"]:
                    for acc in (0, 1):
                        res = {}
                        fb = K.fallback_count()
                        for form in ("one", "batch"):
                            ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
                            dw = dw0.clone()
                            db = db0.clone() if with_db else None
                            stream = torch.cuda.current_stream().cuda_stream
                            if form == "one":
                                K.check(lib.pcuda_conv2d_wgrad(C.byref(g), prec, C.byref(src), dy.data_ptr(), sn, sc, dw.data_ptr(),
                                                               K._ptr(db), acc, ws.data_ptr(), ws_bytes, stream), "conv2d_wgrad")
                            else:
                                job = L.ReduceJob()
                                K.check(lib.pcuda_conv2d_wgrad_partial(C.byref(g), prec, C.byref(src), dy.data_ptr(), sn, sc,
                                                                       dw.data_ptr(), K._ptr(db), acc, ws.data_ptr(), ws_bytes,
                                                                       C.byref(job), stream), "conv2d_wgrad_partial")
                            tag = K.last_kernel()
                            if form == "batch":
                                K.check(lib.pcuda_wgrad_reduce_batch(C.byref(job), 1, stream), "wgrad_reduce_batch")
                            torch.cuda.synchronize()      # a HIP error of this run surfaces here: nothing runs after it
                            res[form] = (tag, _sha(dw), _sha(db))
                        off = lambda q: None if not q else q - ws.data_ptr()
                        rec = dict(table=table, case=case["name"], prec=prec, db=int(with_db), acc=acc, last_kernel=res["one"][0],
                                   last_kernel_partial=res["batch"][0], fallbacks=K.fallback_count() - fb,
                                   job=dict(numel=job.numel, ksplit=job.ksplit, nkg=job.nkg, ntaps=job.ntaps, nb=job.nb,
                                            accumulate=job.accumulate, partial_off=off(job.partial), db_partial_off=off(job.db_partial)),
                                   hash=dict(dw=res["one"][1], db=res["one"][2], dw_batch=res["batch"][1], db_batch=res["batch"][2]))
                        out.write(json.dumps(rec) + "\n")
                        out.flush()
        out.write(json.dumps(dict(table=table, done=True)) + "\n")


if __name__ == "__main__":
    try:
        main(sys.argv[1], sys.argv[2])
    except BaseException:      # a HIP error (or anything else): report and stop, non-zero
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(3)
