"""The device assembly of csrc/pointnet_small.hip under the VMEM address rule of common.h: no vector-memory load whose
destination registers overlap the registers that hold its address (the file is not on the allow-list of
tests/test_isa_rules.py: its count is 0).  Its kernels are bit-identical restatements of the general ones, which multiply and
add in two roundings (-ffp-contract=off): no fp32 fma may appear; nothing spills.  A CPU-side check: hipcc cross-compiles
without a GPU."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_pointnet_small_kernels_keep_load_addresses_alive_and_contract_nothing():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=pointnet_small.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "pointnet_small.s"]
    assert len(rows) == 5, "expected bn1d_fwd, bn1d_bwd, the gather and the two apply kernels in the assembly"
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
    text = open(os.path.join(CSRC, "build", "isa", "pointnet_small.s")).read()
    fused = re.findall(r"^\s*(v_(?:pk_)?(?:fma|fmac|mad)_f32\w*)", text, re.M)
    assert not fused, "fp32 multiply-adds were contracted: %s" % sorted(set(fused))
    assert text.count(".private_segment_fixed_size: 0") == 5, "a kernel spills to scratch"
