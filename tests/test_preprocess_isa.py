"""The device assembly of csrc/preprocess.hip under the VMEM address rule of common.h: no
vector-memory load whose destination registers overlap the registers that hold its address; the tile histogram is an LDS
integer atomic, the minimum / maximum are integer atomics, the blend of the interpolation kernel is not contracted, nothing
spills.  A CPU-side check: hipcc cross-compiles without a GPU."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
FUSED = ("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32", "v_fma_mix", "v_mad_mix")


def _kernels(text):
    """{mangled name: body} of every kernel of an assembly listing"""
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_Z[^\n:]+):.*?s_endpgm", text, re.S | re.M)}


def _fused(lines):
    return [l.strip() for l in lines if any(op in l for op in FUSED)]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_preprocess_kernels_keep_load_addresses_alive_and_do_not_contract_the_blend():
    r = subprocess.run(["make", "-C", CSRC, "isa", "ISA_SRCS=preprocess.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("vmem_overlap_scan", os.path.join(ROOT, "scripts", "vmem_overlap_scan.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rows = [r for r in V.scan(os.path.join(CSRC, "build", "isa")) if r[0] == "preprocess.s"]
    names = " ".join(k for _, k, _, _ in rows)
    # the LUT kernel, four forms of the apply kernel (dword / scalar accesses x uint8 / fp32 out), the reduction cells'
    # initialisation, the min / max reduce of three dtypes and the map kernel of four (dword / byte stores)
    assert len(rows) == 17, names
    for want, count in (("clahe_lut_kernel", 1), ("clahe_apply_kernel", 4), ("rescale_init_kernel", 1), ("rescale_minmax_kernel", 3),
                        ("rescale_map_kernel", 8)):
        assert names.count(want) == count, (want, names)
    bad = [(k, n, ex) for _, k, n, ex in rows if n]
    assert not bad, "loads whose destination overlaps their address: %s" % bad[:4]
    text = open(os.path.join(CSRC, "build", "isa", "preprocess.s")).read()
    assert text.count(".private_segment_fixed_size: 0") == 17, "a kernel spills to scratch"
    kernels = _kernels(text)
    assert len(kernels) == 17
    lut = [b for k, b in kernels.items() if "clahe_lut_kernel" in k]
    assert len(lut) == 1 and "ds_add_u32" in lut[0], "the tile histogram is an LDS integer atomic"
    assert "v_rndne_f32" in lut[0], "rint of the scaled cumulative sum"
    for k, b in kernels.items():
        if "rescale_minmax_kernel" in k:
            assert "global_atomic_umin" in b and "global_atomic_umax" in b and "global_load_dwordx4" in b, k
        if "rescale_map_kernel" in k and "ILi3E" not in k:
            assert "v_div_fixup_f64" in b and "v_trunc_f64" in b, "a true float64 division, truncation toward zero: %s" % k
            assert "v_fma_f64" not in _outside_divisions(b, "f64"), "the rescale must not be contracted: %s" % k
    # the interpolation kernel: sixteen LUT bytes per lane and row, rint, and no fused multiply-add anywhere in the uint8 forms;
    # the fp32 forms divide by 255 (v_div_scale .. v_div_fixup: Newton steps made of fmas) and hold none outside of that
    apply = {k: b for k, b in kernels.items() if "clahe_apply_kernel" in k}
    for k, b in apply.items():
        assert b.count("ds_read_u8") == 16 and "v_rndne_f32" in b, k
        if k.endswith("ELi0EEEvNS_9ClaheArgsEi"):
            assert "v_div_scale_f32" not in b and not _fused(b.splitlines()), (k, _fused(b.splitlines())[:4])
        else:
            assert b.count("v_div_fixup_f32") == 4, k
            lines = b.splitlines()
            first = min(i for i, l in enumerate(lines) if "v_div_scale_f32" in l)
            last = max(i for i, l in enumerate(lines) if "v_div_fixup_f32" in l)
            stray = _fused(lines[:first] + lines[last + 1:])
            assert not stray, "a fused multiply-add outside the division by 255: %s %s" % (k, stray[:4])
    assert sum(k.endswith("ELi0EEEvNS_9ClaheArgsEi") for k in apply) == 2
    # the blend's own multiplications are all there in the fp32 forms too (12 per pixel, four pixels per lane and row)
    muls = {k: len(re.findall(r"\bv_mul_f32", b)) + 2 * len(re.findall(r"\bv_pk_mul_f32", b)) for k, b in apply.items()}
    assert min(muls.values()) >= 24, muls


def _outside_divisions(text, kind):
    """the assembly without the division expansions (v_div_scale .. v_div_fixup: Newton steps made of fmas)"""
    out, inside = [], False
    for line in text.splitlines():
        if "v_div_scale_" + kind in line:
            inside = True
        if not inside:
            out.append(line)
        if "v_div_fixup_" + kind in line:
            inside = False
    return "\n".join(out)
