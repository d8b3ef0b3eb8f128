"""CPU checks of the test-volume reader of the evaluate scripts (pointcloududa_amd/utils/volume.py, csrc/evalprep.hip; DESIGN.md
section 6, f13): the C declarations against the binding and the exported symbols, the entry points' argument checks with fake
pointers, the host-side validation of the Python wrappers, and the table arithmetic of evaluate_mmwhs.evaluate_segmentation fed
rows directly.  No GPU."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pointcloududa_amd", "csrc")
ENTRIES = ("pcuda_volume_slices", "pcuda_volume_labels", "pcuda_volume_restore")


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_binding_and_exported_symbols_agree():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "pcuda_stream_t": ctypes.c_void_p, "long long": ctypes.c_longlong}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret in tuple((e, "int") for e in ENTRIES) + (("pcuda_volume_labels_workspace_size", "size_t"),):
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m and m.group(1) == ret, name
        params = [re.sub(r"\s+", " ", s).strip() for s in m.group(2).split(",") if s.strip() != "void"]
        want = [ctypes.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0]] for a in params]
        res, args = _lib._PROTOS[name]
        assert res is kinds[ret] and list(args) == want, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert int(re.search(r"#define\s+PCUDA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _lib.PCUDA_ABI_VERSION == _lib.lib().pcuda_version()
    codes = {k: int(v) for k, v in re.findall(r"#define\s+PCUDA_VOL_(\w+)\s+(\d+)", hdr)}
    assert codes == {"F32": 0, "I16": 1, "U8": 2, "F64": 4, "I32": 5}
    import torch
    from pointcloududa_amd import kernels as K
    assert K._VOL_DTYPES == {torch.float32: 0, torch.int16: 1, torch.uint8: 2, torch.float64: 4, torch.int32: 5}
    assert "evalprep.hip" in open(os.path.join(CSRC, "Makefile")).read()
    src = open(os.path.join(CSRC, "evalprep.hip")).read()
    for entry in ENTRIES:
        assert 'extern "C" int %s(' % entry in src, entry
    assert 'extern "C" size_t pcuda_volume_labels_workspace_size(' in src
    assert _lib.lib().pcuda_volume_labels_workspace_size() == 16


def test_bad_arguments_are_rejected_without_a_gpu():
    """fake pointers: every call below must return before any launch"""
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    IN, OUT, HOT, WS, LUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    remap = (ctypes.c_int * 18)(*range(18))
    rm = ctypes.cast(remap, ctypes.c_void_p)

    def slices(inp=IN, dt=1, base=0, sz=64, sr=8, sc=1, z=4, r=8, c=8, fr=1, fc=1, window=3, out=OUT):
        return lib.pcuda_volume_slices(inp, dt, base, sz, sr, sc, z, r, c, fr, fc, window, out, None)

    def labels(inp=IN, dt=2, base=0, sz=64, sr=8, sc=1, z=4, r=8, c=8, fr=1, fc=1, ncls=5, remap=rm, nrm=3, raw=0, out=OUT, hot=HOT, ws=WS,
               nbytes=16):
        return lib.pcuda_volume_labels(inp, dt, base, sz, sr, sc, z, r, c, fr, fc, ncls, remap, nrm, raw, out, hot, ws, nbytes, None)

    def restore(inp=IN, z=4, r=8, c=8, out=OUT, dt=1, base=0, sz=64, sr=8, sc=1, fr=1, fc=1, lut=LUT):
        return lib.pcuda_volume_restore(inp, z, r, c, out, dt, base, sz, sr, sc, fr, fc, lut, None)

    shared = (dict(z=-1), dict(r=-1), dict(c=-3), dict(sz=0), dict(sr=0), dict(sc=0), dict(sz=-64), dict(sc=-1), dict(base=-1),
              dict(inp=None), dict(out=None), dict(out=IN), dict(dt=3), dict(dt=6), dict(dt=-1))
    for call, tag in ((slices, b"volume_slices"), (labels, b"volume_labels"), (restore, b"volume_restore")):
        for kw in shared:
            assert call(**kw) == -1 and lib.pcuda_last_error().startswith(tag), (tag, kw, lib.pcuda_last_error())
        # a zero stride is refused only on an axis longer than 1; an empty volume is a no-op, whatever its strides
        assert call(z=-1, sz=0) == -1
        for kw in (dict(z=0), dict(r=0), dict(c=0), dict(z=0, sz=0, sr=0, sc=0)):
            assert call(**kw) == 0, (tag, kw, lib.pcuda_last_error())
    # (an axis of length 1 with stride 0 passes the checks: it would launch, so it is left to the GPU tests)
    for kw in (dict(dt=5), dict(window=0), dict(window=2), dict(window=5), dict(window=-3)):      # int32 is no image dtype
        assert slices(**kw) == -1 and lib.pcuda_last_error().startswith(b"volume_slices"), kw
    for kw in (dict(nrm=9), dict(nrm=-1), dict(remap=None), dict(ncls=1), dict(ncls=256), dict(ncls=0), dict(raw=1), dict(hot=IN)):
        assert labels(**kw) == -1 and lib.pcuda_last_error().startswith(b"volume_labels"), kw      # (raw with a one-hot output)
    for kw in (dict(ws=None), dict(nbytes=8), dict(ws=WS + 4)):
        assert labels(**kw) == -4 and lib.pcuda_last_error().startswith(b"volume_labels"), kw
    for kw in (dict(dt=0), dict(dt=4), dict(dt=5), dict(lut=LUT + 1)):                               # uint8 or int16 only
        assert restore(**kw) == -1 and lib.pcuda_last_error().startswith(b"volume_restore"), kw


# ---------------------------------------------------------------------------------------------- the host side of the package
def test_argument_validation_raises_before_touching_the_device():
    import torch
    from pointcloududa_amd import evaluate_mmwhs as EW
    from pointcloududa_amd import evaluate_mscmrseg as EM
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils import volume as VOL
    v = torch.zeros((8, 8, 4), dtype=torch.int16)
    for bad in (torch.zeros((8, 8, 4), dtype=torch.int32), torch.zeros((8, 8, 4), dtype=torch.int64), np.zeros((8, 8, 4), np.int64)):
        with pytest.raises(TypeError, match="float32 / float64 / int16 / uint8"):
            VOL.volume_slices(bad)
    for bad in (torch.zeros((8, 8, 4), dtype=torch.int64), np.zeros((8, 8, 4), np.float16)):
        with pytest.raises(TypeError, match="uint8 / int16 / int32 / float32 / float64"):
            VOL.volume_labels(bad)
    with pytest.raises(TypeError, match="device tensor or a numpy array"):
        VOL.volume_slices([[[1.0]]])
    for fn in (VOL.volume_slices, VOL.volume_labels):
        for bad in (torch.zeros((8, 8), dtype=torch.int16), np.zeros((1, 8, 8, 4), np.int16)):
            with pytest.raises(ValueError, match="3-D"):
                fn(bad)
        for axis in (3, -4, 1.0, True):
            with pytest.raises(ValueError, match="slice_axis"):
                fn(v, slice_axis=axis)
        with pytest.raises(TypeError, match="flip is a pair"):
            fn(v, flip=True)
    for window in (0, 2, 5, "3"):
        with pytest.raises(ValueError, match="window is 1 or 3"):
            VOL.volume_slices(v, window=window)
    for ncls in (1, 256, 5.0, True):
        with pytest.raises(ValueError, match="classes"):
            VOL.volume_labels(v, num_classes=ncls)
    with pytest.raises(ValueError, match="at most 8"):
        VOL.volume_labels(v, remap=tuple((k, 1) for k in range(9)))
    with pytest.raises(TypeError, match="pairs"):
        VOL.volume_labels(v, remap=(200, 1))
    for kw in (dict(onehot=True), dict(remap=((200, 1),))):
        with pytest.raises(ValueError, match="raw output"):
            VOL.volume_labels(v, raw=True, **kw)
    p = torch.zeros((4, 8, 8), dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8 or torch.int16"):
        VOL.restore_volume(p, (8, 8, 4), dtype=torch.int32)
    with pytest.raises(TypeError, match="uint8 .D,H,W. device tensor"):
        VOL.restore_volume(p.to(torch.int16), (8, 8, 4))
    for shape in ((8, 8), (8, 8, 4, 1), (8, -1, 4)):
        with pytest.raises(ValueError, match="3-D shape"):
            VOL.restore_volume(p, shape)
    with pytest.raises(ValueError, match="does not fit"):
        VOL.restore_volume(p, (8, 4, 8))
    with pytest.raises(ValueError, match="does not fit"):
        VOL.restore_volume(p, (8, 4, 4), transpose=True)                 # (the transpose of an [8,8,4] volume is [4,8,8]: p would fit that)
    for lut in (list(range(255)), [0.5] * 256, [40000] * 256):
        with pytest.raises(ValueError, match="256 int16 values"):
            VOL.restore_volume(p, (8, 8, 4), lut=lut)
    # no CPU fallback
    for call in (lambda: VOL.volume_slices(v), lambda: VOL.volume_labels(v), lambda: VOL.restore_volume(p, (8, 8, 4)),
                 lambda: EM.read_labels(v), lambda: EM.restore_prediction(p, (8, 8, 4)), lambda: EW.read_volume(v, v),
                 lambda: K.volume_slices(v), lambda: K.volume_labels(v), lambda: K.volume_restore(p, v.movedim(2, 0))):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            VOL.volume_slices(np.zeros((8, 8, 4), np.float32))


# ---------------------------------------------------------------------------------------------- the table
def test_the_table_leaves_a_minus_one_out_of_that_class_only():
    from pointcloududa_amd import evaluate_mmwhs as EW
    #        Myo (LVmyo)       LA-blood          LV-blood          AA
    res = [[0.90, 1.0, 0.50, 0.80, -1, -1, 0.70, 2.0, 1.00, 0.60, 3.0, 1.50],
           [0.50, 2.0, 0.70, 0.30, 4.0, 2.25, 0.20, -1, -1, 0.10, 1.0, 0.50],
           [0.40, 4.5, 0.90, 0.10, 5.0, 1.75, 0.60, 1.0, 0.25, 0.30, -1, -1]]
    t = EW.summary_table(res)
    assert set(t) == {"DC", "HD", "ASD", "Ave"} and list(t["DC"]) == ["AA", "LAblood", "LVblood", "LVmyo"]

    def ms(vals):
        return (np.around(np.mean(np.array(vals)), 3), np.around(np.std(np.array(vals)), 3))

    assert t["DC"] == {"AA": ms([0.6, 0.1, 0.3]), "LAblood": ms([0.8, 0.3, 0.1]), "LVblood": ms([0.7, 0.2, 0.6]), "LVmyo": ms([0.9, 0.5, 0.4])}
    assert t["HD"] == {"AA": ms([3.0, 1.0]), "LAblood": ms([4.0, 5.0]), "LVblood": ms([2.0, 1.0]), "LVmyo": ms([1.0, 2.0, 4.5])}
    assert t["ASD"] == {"AA": ms([1.5, 0.5]), "LAblood": ms([2.25, 1.75]), "LVblood": ms([1.0, 0.25]), "LVmyo": ms([0.5, 0.7, 0.9])}
    assert t["HD"]["LVmyo"] == (2.5, 1.472) and t["HD"]["AA"] == (2.0, 1.0), "by hand: the patient without AA is not in AA's list"
    for metric in ("DC", "HD", "ASD"):
        cols = [t[metric][k] for k in ("AA", "LAblood", "LVblood", "LVmyo")]
        assert t["Ave"][metric] == ((cols[0][0] + cols[1][0] + cols[2][0] + cols[3][0]) / 4., (cols[0][1] + cols[1][1] + cols[2][1] + cols[3][1]) / 4.)
    assert set(EW.summary_table(res, ifhd=False)) == {"DC", "ASD", "Ave"} and set(EW.summary_table(res, ifhd=False, ifasd=False)) == {"DC", "Ave"}
    # the -save row takes the -1 entries as they are, as the reference does
    assert EW.save_row(res[0], "d1d2d4", 1003) == [float(np.mean([0.9, 0.8, 0.7, 0.6])), float(np.mean([1.0, -1, 2.0, 3.0])),
                                                   float(np.mean([0.5, -1, 1.0, 1.5])), "d1d2d4", 1003]
    # the extended lists hold five values per class; the table reads the first three
    ext = [[v for k in range(4) for v in r[3 * k:3 * k + 3] + [9.0, 9.0]] for r in res]
    assert EW.summary_table(ext, extended=True) == t and EW.save_row(ext[0], "m", 1, extended=True)[:3] == EW.save_row(res[0], "m", 1)[:3]


def test_a_class_that_is_minus_one_for_every_patient_gives_nan(capsys):
    from pointcloududa_amd import evaluate_mmwhs as EW
    res = [[0.9, 1.0, 0.5, 0.0, -1, -1, 0.7, 2.0, 1.0, 0.6, 3.0, 1.5],
           [0.5, 2.0, 0.7, 0.0, -1, -1, 0.2, 1.0, 0.5, 0.1, 1.0, 0.5]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        t = EW.summary_table(res)
        want = np.around(np.mean(np.array([])), 3)
    assert np.isnan(want) and all(np.isnan(v) for v in t["HD"]["LAblood"] + t["ASD"]["LAblood"])
    assert t["DC"]["LAblood"] == (0.0, 0.0) and t["HD"]["AA"] == (2.0, 1.0)
    assert all(np.isnan(v) for v in t["Ave"]["HD"] + t["Ave"]["ASD"]) and not any(np.isnan(v) for v in t["Ave"]["DC"])
    empty = EW.summary_table([])
    assert all(np.isnan(v) for m in ("DC", "HD", "ASD") for pair in empty[m].values() for v in pair)
    EW.print_table(t)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Ave AA DC: 0.35, 0.25, Ave LAblood DC: 0.0, 0.0, Ave LVblood DC: 0.45, 0.25, Ave LVmyo DC: 0.7, 0.2"
    assert lines[1] == "Ave Dice: 0.375, 0.175" and lines[2].startswith("Ave AA HD: 2.0, 1.0, Ave LAblood HD: nan, nan")
    assert lines[3] == "Ave HD: nan, nan" and lines[5] == "Ave ASD: nan, nan" and len(lines) == 9
    assert lines[6] == "0.35, 0.25, 0.0, 0.0, 0.45, 0.25, 0.7, 0.2"


def test_the_docs_name_the_reader_and_what_is_not_built():
    for doc in ("README.md", "DESIGN.md"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        assert "pcuda_volume_slices" in text and "utils/volume.py" in text and "reconstuct_volume" in text, doc
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert "pcuda_volume_slices" in text and "pcuda_volume_restore" in text
    design = re.sub(r"\s+", " ", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert "f13" in design and "profiles/evalprep_bench.json" in design
