"""The device assembly of csrc/area_resize.hip under the VMEM address rule of common.h: no vector-memory
load whose destination registers overlap the registers that hold its address; and nothing spills to scratch.  A CPU-side check:
hipcc cross-compiles without a GPU."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_area_resize_kernels_keep_load_addresses_alive_and_do_not_spill():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=area_resize.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "area_resize.s"]
    names = " ".join(k for _, k, _, _ in rows)
    # the plain resize and the fused form of the one template
    assert len(re.findall(r"::area_resize_kernel<", names)) == 2 and len(rows) == 2, names
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
    text = open(os.path.join(CSRC, "build", "isa", "area_resize.s")).read()
    assert text.count(".private_segment_fixed_size: 0") == 2, "a kernel spills to scratch"
