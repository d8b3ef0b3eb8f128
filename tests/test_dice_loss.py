"""Dice loss, the parts that need no GPU: the two float64 restatements of tests/dice_refs.py against the fixture
scripts/make_dice_golden.py wrote from them; the C ABI of csrc/dice_loss.hip (declared, exported, bound; arguments rejected
before any launch); the switch's default and its mapping from the scripts' ``args``."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import dice_refs as D
from conftest import GOLD, ROOT

ENTRY_POINTS = ("pcuda_seg_loss_ov_workspace_size", "pcuda_seg_loss_ov_fwd", "pcuda_seg_loss_ov_bwd", "pcuda_dice_workspace_size",
                "pcuda_dice_fwd", "pcuda_dice_bwd", "pcuda_dice_labels_workspace_size", "pcuda_dice_labels_fwd",
                "pcuda_dice_labels_bwd")
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
CLASS, SAMPLE = 1, 2


@pytest.mark.parametrize("which", ["autograd", "closed_form"])
def test_both_restatements_reproduce_the_golden_file(which):
    g = np.load(os.path.join(GOLD, "dice_loss.npz"))
    eps = {"class": float(g["eps_class"]), "sample": float(g["eps_sample"])}
    assert eps == {"class": 1e-7, "sample": 1e-6}
    fn = D.dice_autograd if which == "autograd" else D.dice_closed_form
    assert len(g["shapes"]) == 3
    for i, shape in enumerate(g["shapes"]):
        logits, onehot = torch.from_numpy(g["c%d/logits" % i]), torch.from_numpy(g["c%d/onehot" % i])
        assert tuple(logits.shape) == tuple(shape) == tuple(onehot.shape)
        for mode in ("sigmoid", "softmax"):
            for reduce in ("class", "sample"):
                loss, grad = fn(logits, onehot, mode, reduce, eps[reduce])
                grad = grad.numpy() if torch.is_tensor(grad) else grad
                assert abs(float(loss) - float(g["c%d/%s/%s/loss" % (i, mode, reduce)])) <= 1e-12, (i, mode, reduce)
                assert np.abs(grad - g["c%d/%s/%s/grad" % (i, mode, reduce)]).max() <= 1e-12, (i, mode, reduce)


def test_the_two_reductions_are_different_losses():
    """not vacuous: on a batch whose samples differ, per class and per sample disagree"""
    g = np.load(os.path.join(GOLD, "dice_loss.npz"))
    assert abs(float(g["c0/softmax/class/loss"]) - float(g["c0/softmax/sample/loss"])) > 1e-4


def test_header_declares_and_library_exports_the_entry_points():
    from pointcloududa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pcuda_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), "not declared: " + name
        assert hasattr(handle, name), "not exported: " + name
        assert name in _lib.EXPORTED_SYMBOLS, "not bound: " + name
    assert re.search(r"#define\s+PCUDA_OV_DICE_CLASS\s+1\b", code) and re.search(r"#define\s+PCUDA_OV_DICE_SAMPLE\s+2\b", code)
    assert (_lib.OV_DICE_CLASS, _lib.OV_DICE_SAMPLE) == (CLASS, SAMPLE)
    assert lib.pcuda_version() == _lib.PCUDA_ABI_VERSION == 5
    assert int(re.search(r"#define\s+PCUDA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5
    mk = open(os.path.join(ROOT, "pointcloududa_amd", "csrc", "Makefile")).read()
    assert "dice_loss.hip" in mk.split("SRCS")[1].splitlines()[0] and mk.count("loss_device.h") == 2


def test_workspace_sizes():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    assert lib.pcuda_seg_loss_ov_workspace_size(2, 4, 256, CLASS) > 0 and lib.pcuda_seg_loss_ov_workspace_size(2, 4, 256, SAMPLE) > 0
    # per sample: the coefficients and the partial rows grow with the batch
    assert lib.pcuda_seg_loss_ov_workspace_size(65537, 1, 3, SAMPLE) > 65537 * (16 + 8 + 12)
    assert lib.pcuda_dice_workspace_size(65537, 1, 3, SAMPLE) > 65537 * (16 + 8 + 8)
    assert lib.pcuda_dice_labels_workspace_size(2, 16, 300) > 0
    for bad in ((0, 4, 256, CLASS), (2, 0, 256, CLASS), (2, 9, 256, SAMPLE), (2, 4, 0, CLASS), (2, 4, 256, 0), (2, 4, 256, 3)):
        assert lib.pcuda_seg_loss_ov_workspace_size(*bad) == 0, bad
    for bad in ((0, 4, 256, CLASS), (2, 0, 256, CLASS), (2, 17, 256, SAMPLE), (2, 4, 0, CLASS), (2, 4, 256, 0), (2, 4, 256, 3)):
        assert lib.pcuda_dice_workspace_size(*bad) == 0, bad
    for bad in ((0, 4, 256), (2, 0, 256), (2, 17, 256), (2, 4, 0)):
        assert lib.pcuda_dice_labels_workspace_size(*bad) == 0, bad


def test_bad_arguments_are_rejected_before_any_launch():
    """null pointers, C = 0, C above the limit, an unknown overlap / reduce and a short workspace: a negative status from
    every new entry point and not one launch (the host-side launch counter does not move; no GPU is needed to get here)"""
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)          # stands for every tensor: no call below may get as far as reading it
    p = ctypes.addressof(buf)
    big = 1 << 16
    n, c, hw = 2, 4, 16

    def ov_fwd(logits=p, onehot=p, mode=0, ov=CLASS, eps=1e-7, n=n, c=c, hw=hw, out=p, ws=p, nb=big):
        return lib.pcuda_seg_loss_ov_fwd(logits, onehot, mode, ov, eps, n, c, hw, out, ws, nb, None)

    def ov_bwd(logits=p, onehot=p, mode=0, ov=CLASS, n=n, c=c, hw=hw, d=p, ws=p, nb=big):
        return lib.pcuda_seg_loss_ov_bwd(logits, onehot, mode, ov, n, c, hw, None, None, d, ws, nb, None)

    def d_fwd(probs=p, truth=p, n=n, c=c, hw=hw, red=CLASS, loss=p, ws=p, nb=big):
        return lib.pcuda_dice_fwd(probs, truth, 1, n, c, hw, red, 1e-7, loss, ws, nb, None)

    def d_bwd(truth=p, n=n, c=c, hw=hw, red=CLASS, dp=p, ws=p, nb=big):
        return lib.pcuda_dice_bwd(truth, 1, n, c, hw, red, None, dp, ws, nb, None)

    def l_fwd(logits=p, labels=p, n=n, c=c, hw=hw, loss=p, ws=p, nb=big):
        return lib.pcuda_dice_labels_fwd(logits, labels, 0, n, c, hw, 1e-6, loss, None, ws, nb, None)

    def l_bwd(logits=p, labels=p, n=n, c=c, hw=hw, d=p, ws=p, nb=big):
        return lib.pcuda_dice_labels_bwd(logits, labels, 0, n, c, hw, None, d, ws, nb, None)

    before = lib.pcuda_launch_count(0)
    for fn, said, ptrs in ((ov_fwd, b"seg_loss_ov_fwd", ("logits", "onehot", "out")), (ov_bwd, b"seg_loss_ov_bwd", ("logits", "onehot", "d")),
                           (d_fwd, b"dice_fwd", ("probs", "truth", "loss")), (d_bwd, b"dice_bwd", ("truth", "dp")),
                           (l_fwd, b"dice_labels_fwd", ("logits", "labels", "loss")), (l_bwd, b"dice_labels_bwd", ("logits", "labels", "d"))):
        for name in ptrs:
            assert fn(**{name: None}) == BADARG, (fn.__name__, name)
            assert said in lib.pcuda_last_error()
        assert fn(ws=None) == WORKSPACE, fn.__name__
        assert fn(nb=8) == WORKSPACE, fn.__name__
        assert fn(c=0) == BADARG and fn(n=0) == BADARG and fn(hw=0) == BADARG, fn.__name__
    for fn in (ov_fwd, ov_bwd):
        assert fn(c=9) == UNSUPPORTED and fn(c=17) == UNSUPPORTED, fn.__name__
        assert fn(ov=0) == BADARG and fn(ov=3) == BADARG, fn.__name__
        assert fn(mode=2) == BADARG, fn.__name__
        # per sample the size grows with the batch: one byte less than the size function's answer is short
        assert fn(ov=SAMPLE, n=4096, hw=1, nb=lib.pcuda_seg_loss_ov_workspace_size(4096, c, 1, SAMPLE) - 1) == WORKSPACE
    for fn in (d_fwd, d_bwd):
        assert fn(c=17) == BADARG, fn.__name__
        assert fn(red=0) == BADARG and fn(red=3) == BADARG, fn.__name__
    for fn in (l_fwd, l_bwd):
        assert fn(c=17) == BADARG, fn.__name__
    assert ov_fwd(eps=-1.0) == BADARG and ov_fwd(eps=float("nan")) == BADARG
    assert lib.pcuda_launch_count(0) == before


def test_the_switch_is_off_by_default_and_maps_from_args():
    from pointcloududa_amd._epoch import _cfg_from
    from pointcloududa_amd.train_step import TrainCfg
    from pointcloududa_amd.utils import loss as L
    assert TrainCfg().dice == ""
    none = (None, None, None, None)
    assert _cfg_from(types.SimpleNamespace(), "mmwhs", none).dice == ""
    assert _cfg_from(types.SimpleNamespace(dice=False), "mmwhs", none).dice == ""
    assert _cfg_from(types.SimpleNamespace(dice=True), "mmwhs", none).dice == "class"
    assert _cfg_from(types.SimpleNamespace(dice=True), "mscmrseg", none).dice == "class"
    assert _cfg_from(types.SimpleNamespace(dice="sample"), "mmwhs", none).dice == "sample"
    assert [L.overlap_for(d) for d in ("", "class", "sample")] == ["jaccard", "dice", "dice_sample"]
    with pytest.raises(ValueError):
        L.overlap_for("tversky")


def test_python_forms_validate_before_touching_the_device():
    from pointcloududa_amd.utils import loss as L
    x, y = torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64)
    m = L.DiceLoss()
    assert m.eps == 1e-6 and isinstance(m, torch.nn.Module)
    with pytest.raises(ValueError):
        m(x[0], y)                                   # rank
    with pytest.raises(ValueError):
        m(x, y[:, None])
    with pytest.raises(ValueError):
        m(x, torch.zeros(2, 4, 5, dtype=torch.int64))           # spatial size
    with pytest.raises(ValueError):
        m(x, torch.zeros(3, 4, 4, dtype=torch.int64))           # batch
    with pytest.raises(ValueError):
        L.seg_loss(x, torch.zeros(2, 3, 4, 4, dtype=torch.uint8), "sigmoid", "tversky")
    with pytest.raises(ValueError):
        L.dice_loss(torch.zeros(2, 3, 4, 4), x, reduce="batch")
