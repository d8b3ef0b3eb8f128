"""Pins the weight-gradient host side (csrc/conv_wgrad*.hip, the wgrad routes of csrc/conv_direct*.hip) in
tests/golden/conv_wgrad_plan.json; tests/test_conv_wgrad_plan.py and tests/test_conv_wgrad_pin_gpu.py compare a build to it.

Run it on the build whose behaviour is to be kept (the PARENT of a refactor), never on the commit under test:

    python scripts/make_conv_wgrad_golden.py             # both pins (the device pin needs the MI355X)
    python scripts/make_conv_wgrad_golden.py --host      # the host pin only: keeps the file's device records

Host pin: ``pcuda_conv2d_wgrad_workspace_size`` for every geometry of make_conv_host_golden.GEOMS, the geometries of the device
pin and one that hits the 64 MB slab cap, under four sets of the route switches.  The switches are cached per process, so
every set is a child process (this file with ``--sizes``) that loads the library and prints the sizes; it launches nothing.

Device pin: tests/conv_wgrad_child.py, one child per table, one after the other, each under its own timeout; a child that
fails ends the run.  The generator asserts that every branch the cases were chosen for is reached (conv_wgrad_child.REACH)."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "conv_wgrad_plan.json")
for _p in (os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import conv_wgrad_child as child  # noqa: E402
from make_conv_host_golden import GEOMS, _g, geom_struct  # noqa: E402

HOST_KNOBS = {
    "default": {},
    "w3r0": {"PCUDA_WGRAD3R": "0"},
    "w3r2": {"PCUDA_WGRAD3R": "2"},
    "w3r0_nowgrad1": {"PCUDA_WGRAD3R": "0", "PCUDA_NO_WGRAD1": "1"},
}
SLAB_CAP = _g(8, 512, 512, 4, 4, 3)          # 1024 wanted slices of 9.4 MB: halved down to the 64 MB cap
# Where a special route asks for MORE than the generic plan, so that its switch shows in the size (the maximum over the
# routes): twelve one-tile images -- the generic plan rounds its 12 slices down to 8, wgrad3r (an up-convolution by default,
# any layer in mode 2) and wgrad1 keep 12.
ROUTE_DOMINATES = [_g(12, 16, 32, 4, 32, 3, up=1), _g(12, 16, 32, 4, 32, 3), _g(12, 16, 8, 4, 4, 1)]
CHILD_TIMEOUT = 300                          # seconds; a hang guard, not a budget


def geom_slab_bytes(t, slices):
    """the split-K layout of csrc/conv_host.h: [slices][weights] + [slices][cout] floats + 256 bytes"""
    _n, cin, cout, _h, _w, k = t[:6]
    return (slices * cout * cin * k * k + slices * cout) * 4 + 256


def host_geoms():
    out = list(GEOMS)
    for t in [c["geom"] for c in child.CASES] + [SLAB_CAP] + ROUTE_DOMINATES:
        if t not in out:
            out.append(t)
    return out


def _switches():
    return sorted({k for kn in list(HOST_KNOBS.values()) + list(child.TABLES.values()) for k in kn})


def _env(knobs):
    env = {k: v for k, v in os.environ.items() if k not in _switches()}
    env.update(knobs)
    return env


def print_sizes():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    print(json.dumps([lib.pcuda_conv2d_wgrad_workspace_size(C.byref(geom_struct(t))) for t in host_geoms()]))


def record_host():
    """{knob set: [workspace bytes per geometry of host_geoms()]} of the library pointcloududa_amd._lib loads"""
    out = {}
    for name, knobs in HOST_KNOBS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sizes"], capture_output=True, text=True, env=_env(knobs),
                           timeout=CHILD_TIMEOUT)
        if r.returncode != 0:
            raise RuntimeError("size child %r exited with %s\n%s" % (name, r.returncode, r.stderr[-2000:]))
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
        assert len(out[name]) == len(host_geoms())
    return out


def record_device(tmp_dir):
    """the records of every table (conv_wgrad_child.py), or RuntimeError at the first child that does not finish"""
    records = []
    for table, knobs in child.TABLES.items():
        path = os.path.join(tmp_dir, "wgrad_pin_%s.jsonl" % table)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_wgrad_child.py"), table, path], capture_output=True,
                           text=True, env=_env(knobs), timeout=CHILD_TIMEOUT)
        if r.returncode != 0:
            raise RuntimeError("device child %r exited with %s\n%s" % (table, r.returncode, r.stderr[-3000:]))
        recs = [json.loads(ln) for ln in open(path)]
        if not recs or not recs[-1].get("done"):
            raise RuntimeError("device child %r did not finish its table" % table)
        records += recs[:-1]
    return records


def check_host(host):
    names = list(host)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert host[a] != host[b], "knob sets %s and %s give the same sizes everywhere: they pin nothing" % (a, b)


def check_device(records):
    missing = child.missing_branches(records)
    assert not missing, "branches no case reaches: %s" % missing
    for r in records:
        h = r["hash"]
        assert h["dw"] == h["dw_batch"] and h["db"] == h["db_batch"], "one-by-one and batched reduce differ on the parent: %r" % r


def main(argv):
    if "--sizes" in argv:
        return print_sizes()
    import tempfile
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else OUT
    doc = {"note": "workspace sizes and launch records of the weight-gradient routes on the parent of the route-table refactor "
                   "(scripts/make_conv_wgrad_golden.py)"}
    if os.path.exists(OUT):
        with open(OUT) as fh:
            doc.update(json.load(fh))
    doc["host_geoms"] = [list(t) for t in host_geoms()]
    doc["host"] = record_host()
    check_host(doc["host"])
    if "--host" not in argv:
        with tempfile.TemporaryDirectory() as tmp:
            doc["device"] = record_device(tmp)
    with open(out_path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    if "--host" not in argv:
        check_device(doc["device"])      # (after the write: a missed branch is read from the file)
    print("wrote %s: %d geometries x %d knob sets, %d device records, %d bytes" %
          (out_path, len(doc["host_geoms"]), len(doc["host"]), len(doc.get("device", [])), os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1:])
