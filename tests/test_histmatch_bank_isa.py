"""The device assembly of csrc/histmatch_bank.hip under the VMEM address rule of common.h: no
vector-memory load whose destination registers overlap the registers that hold its address; the histograms are LDS integer
atomics, the interpolation is not contracted, nothing spills.  The counterpart of tests/test_histmatch_isa.py.  A CPU-side
check: hipcc cross-compiles without a GPU."""
import importlib.util
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
KERNELS = 5      # the reference sort, the image sort, the lookup, the uint8 count and the uint8 match


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_histmatch_bank_kernels_keep_load_addresses_alive():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=histmatch_bank.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "histmatch_bank.s"]
    assert len(rows) == KERNELS, "expected %d kernels in the assembly, got %r" % (KERNELS, [k for _, k, _, _ in rows])
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
    text = open(os.path.join(CSRC, "build", "isa", "histmatch_bank.s")).read()
    assert "ds_add_u32" in text, "the histograms are LDS integer atomics"
    assert "v_div_fixup_f64" in text, "the quantiles are true float64 divisions"
    assert "v_fma_f64" not in _outside_divisions(text), "the interpolation must not be contracted"
    assert text.count(".private_segment_fixed_size: 0") == KERNELS, "a kernel spills to scratch"


def _outside_divisions(text):
    """the assembly without the float64 division expansions (v_div_scale .. v_div_fixup: Newton steps made of fmas)"""
    out, inside = [], False
    for line in text.splitlines():
        if "v_div_scale_f64" in line:
            inside = True
        if not inside:
            out.append(line)
        if "v_div_fixup_f64" in line:
            inside = False
    return "\n".join(out)
