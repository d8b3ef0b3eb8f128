"""The device assembly of csrc/stylize.hip under the VMEM address rule of common.h: no vector-memory
load whose destination registers overlap the registers that hold its address -- the claim f7 makes for photometric.hip.
A CPU-side check: hipcc cross-compiles without a GPU."""
import importlib.util
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_stylize_kernels_keep_load_addresses_alive():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=stylize.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "stylize.s"]
    assert len(rows) == 3, "expected the pointwise, the noise-alpha and the superpixel kernel in the assembly"
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
    text = open(os.path.join(CSRC, "build", "isa", "stylize.s")).read()
    assert "global_store_dwordx4" in text, "the copy's 16-byte stores are gone"
    assert "ds_add_u64" in text, "the superpixel sums are LDS integer atomics"
    assert text.count(".private_segment_fixed_size: 0") == 3, "a kernel spills to scratch"
