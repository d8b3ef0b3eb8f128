"""What the bit-pin recorders (scripts/make_*_pin_golden.py) and their tests (tests/test_*_pin_gpu.py) share: seeds, hashes,
the launch counter, the toolchain line, the fixture's writer and the comparison.  A record is
``{"case": key, "launches": {call: count}, "in": {name: sha256}, "hash": {name: sha256}}``."""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import subprocess
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pointcloududa_amd import kernels as K  # noqa: E402


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _counted(launches, name, fn):
    before = K.launch_count()
    out = fn()
    launches[name] = K.launch_count() - before
    return out


def toolchain():
    """what the records depend on besides the sources: the HIP runtime torch was built for and the compiler's version line"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    try:
        text = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout
        line = next((ln.strip() for ln in text.splitlines() if "HIP version" in ln), text.strip().splitlines()[0])
    except Exception as e:      # no compiler on this machine: said, not hidden
        line = "hipcc --version failed: %s" % type(e).__name__
    return {"torch_hip": str(torch.version.hip), "hipcc": line}


def unique_cases(records):
    keys = [r["case"] for r in records]
    assert len(set(keys)) == len(keys), "case keys repeat"
    return records


def write_golden(out_path, note, records):
    """the fixture: the note, the hash of the loaded library's sources, the toolchain, the records"""
    from pointcloududa_amd import _lib
    doc = {"note": note, "build": _lib.csrc_hash(), "toolchain": toolchain(), "records": records}
    with open(out_path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s: %d records, %d bytes" % (out_path, len(doc["records"]), os.path.getsize(out_path)))


def recorder_main(tool, argv, default_out, note, record):
    if not torch.cuda.is_available():
        raise SystemExit("%s: needs a HIP device" % tool)
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else default_out
    write_golden(out_path, note, record(torch.device("cuda", 0)))


def load_golden(path):
    with open(path) as fh:
        return json.load(fh)


def _toolchains(golden):
    now = toolchain()
    if now == golden["toolchain"]:
        return "same toolchain as recorded (%r)" % (now,)
    return "the toolchain differs: recorded %r, running %r" % (golden["toolchain"], now)


def assert_case_list(records, golden):
    assert [r["case"] for r in records] == [r["case"] for r in golden["records"]], "fixture and case list disagree"


def assert_no_differences(records, golden):
    """every input hash, launch count and output hash of ``records`` against the fixture's: no tolerance"""
    want = {r["case"]: r for r in golden["records"]}
    diffs = []
    for r in records:
        w = want[r["case"]]
        for field in ("in", "launches", "hash"):
            assert sorted(r[field]) == sorted(w[field]), (r["case"], field)
            diffs += [(r["case"], field, k, r[field][k], w[field][k]) for k in w[field] if r[field][k] != w[field][k]]
    assert not diffs, "%d differences (%s), the first: %r" % (len(diffs), _toolchains(golden), diffs[:3])
