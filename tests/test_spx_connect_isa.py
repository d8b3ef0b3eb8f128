"""The device assembly of csrc/spx_connect.hip under the VMEM address rule of common.h: no
vector-memory load whose destination registers overlap the registers that hold its address, and no kernel that spills to
scratch.  A CPU-side check: hipcc cross-compiles without a GPU."""
import importlib.util
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_spx_connect_kernels_keep_load_addresses_alive():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=spx_connect.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "spx_connect.s"]
    assert len(rows) == 7, "expected init, merge, compress, size, link, sum and write in the assembly"
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
    text = open(os.path.join(CSRC, "build", "isa", "spx_connect.s")).read()
    assert text.count(".private_segment_fixed_size: 0") == 7, "a kernel spills to scratch"
