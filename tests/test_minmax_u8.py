"""CPU checks of the fp32 -> uint8 -> fp32 joint of the MM-WHS heavy path: the two C entry points
(pcuda_quantize_u8, pcuda_augment_assemble_dequant) reject bad arguments before any launch, and the Python surface rejects an
unknown ``rescale`` before it touches a device."""
import ctypes

import numpy as np
import pytest
import torch


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)                                  # never dereferenced: rejected before any launch
    for args in ((None, 16, fake, fake), (fake, 16, None, fake), (fake, 16, fake, None), (fake, 0, fake, fake),
                 (fake, -5, fake, fake)):
        assert lib.pcuda_quantize_u8(*args, None) == -1, args
        assert b"quantize_u8" in lib.pcuda_last_error()

    def call(img=fake, lab=fake, b=2, h=16, w=16, c=3, crop=0, k=5, inv=fake, order=fake, cval=fake, mm=fake, out=fake,
             onehot=fake, full=None, labels=None, out_u8=None):
        return lib.pcuda_augment_assemble_dequant(img, lab, b, h, w, c, crop, k, inv, order, cval, mm, out, onehot, full, labels,
                                                  out_u8, None)
    for kw, what in ((dict(img=None), b"null"), (dict(inv=None), b"null"), (dict(order=None), b"null"), (dict(cval=None), b"null"),
                     (dict(mm=None), b"null pointer (minmax)"), (dict(out=None, onehot=None), b"null"), (dict(lab=None), b"null"),
                     (dict(lab=None, onehot=None, full=fake), b"null"), (dict(crop=18), b"crop larger"),
                     (dict(h=16, w=8, crop=10), b"crop larger"), (dict(k=1), b"num_classes"), (dict(b=0), b"dims"),
                     (dict(b=65536), b"dims"), (dict(h=0), b"dims"), (dict(w=-1), b"dims"), (dict(c=0), b"dims"),
                     (dict(h=1 << 15, w=1 << 15, c=2), b"dims")):
        assert call(**kw) == -1, kw
        err = lib.pcuda_last_error()
        assert what in err and err.startswith(b"augment_assemble_dequant:"), (kw, err)


def test_assemble_keeps_rejecting_the_modes_the_dequant_entry_adds():
    """rescale = 3 and (rescale = 1, uint8 images) stay errors of pcuda_augment_assemble: the uint8 min-max path has an entry of
    its own"""
    from pointcloududa_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    for u8, rescale, mm, what in ((0, 3, fake, b"rescale"), (1, 3, fake, b"rescale"), (1, 1, fake, b"min-max")):
        assert lib.pcuda_augment_assemble(fake, u8, fake, 2, 16, 16, 3, 0, 5, fake, fake, fake, rescale, mm, fake, fake, None,
                                          None, None, None) == -1
        err = lib.pcuda_last_error()
        assert what in err and err.startswith(b"augment_assemble:"), err


@pytest.mark.parametrize("rescale", ["minmax_u16", "MINMAX_U8", "", 1])
def test_unknown_rescale_is_a_value_error(rescale):
    from pointcloududa_amd.utils.augment import AugmentedBatches, augment_batch
    x, m = torch.zeros(1, 8, 8, 1), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="rescale must be"):
        augment_batch(x, m, None, 2, 0, rescale=rescale)
    for kw in (dict(preset="mmwhs_light"), dict(preset=None, heavy_preset="heavy_refpad_device"),
               dict(preset="mmwhs_light", photometric_preset="mscmrseg_aug2_photometric")):
        preset = kw.pop("preset")
        with pytest.raises(ValueError, match="rescale must be"):
            AugmentedBatches(iter(()), torch.device("cpu"), preset, np.random.default_rng(0), rescale=rescale, **kw)


def test_wrappers_refuse_host_tensors_and_wrong_dtypes():
    """no quiet fall-back: the wrappers raise before the library is called"""
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.augment import quantize_minmax
    with pytest.raises(RuntimeError, match="HIP device"):
        K.quantize_u8(torch.zeros(4), torch.zeros(2))
    with pytest.raises(TypeError):
        quantize_minmax(torch.zeros(1, 4, 4, 1, dtype=torch.uint8))
    with pytest.raises(TypeError):
        quantize_minmax(torch.zeros(4, 4, 1))
    with pytest.raises(TypeError, match="minmax is required"):
        K.augment_assemble_dequant(torch.zeros(1, 4, 4, 1, dtype=torch.uint8), None, None, None, None, None)
    with pytest.raises(TypeError, match="uint8 images"):
        K.augment_assemble_dequant(torch.zeros(1, 4, 4, 1), None, None, None, None, torch.zeros(2))
