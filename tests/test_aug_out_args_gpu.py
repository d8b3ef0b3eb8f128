"""A caller's ``out`` / ``labels_out`` is checked on the host before anything is launched (``kernels._out``): the C entry points only
see a pointer, so a tensor of the wrong dtype or shape, or a non-contiguous view, would be an out-of-bounds write.  One ``B = 1``,
``4 x 4``, ``C = 1`` image and an identity program per wrapper; every bad tensor raises ``ValueError`` with no launch, and a good one
comes back as the same object with the contents of the ``out=None`` call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _image(dev):
    return torch.arange(16, dtype=torch.uint8, device=dev).reshape(1, 4, 4, 1) * 13


def _photometric(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.photometric import PhotoProgram, upload_program
    up = upload_program(PhotoProgram.identity(1, 1), 1, 4, 4, 1, dev)
    return lambda x, **kw: K.photometric(x, *up, **kw)


def _geometric(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.geometric import GeoProgram, upload_geo_program
    up = upload_geo_program(GeoProgram.identity(1, 1), 1, 4, 4, dev)
    return lambda x, **kw: K.geometric(x, None, *up, **kw)[0]


def _stylize(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.stylize import StyleProgram, upload_style_program
    up = upload_style_program(StyleProgram.identity(1, 1), 1, 4, 4, 1, dev)
    return lambda x, **kw: K.stylize(x, *up, **kw)


def _match_hist(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.histmatch import HistReference
    ref = HistReference(np.arange(16, dtype=np.uint8).reshape(4, 4, 1)[::-1] * 7, dev)
    return lambda x, **kw: K.match_hist(x, ref.values, ref.quantiles, ref.lengths, **kw)


def _match_hist_bank(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.histmatch import HistReferenceBank
    bank = HistReferenceBank(np.arange(16, dtype=np.uint8).reshape(1, 4, 4, 1)[:, ::-1] * 7, dev)
    idx = bank.index_tensor(None, 1)
    return lambda x, **kw: K.match_hist_bank(x, bank.bank, bank.shape, idx, **kw)


WRAPPERS = {"photometric": _photometric, "geometric": _geometric, "stylize": _stylize, "match_hist": _match_hist,
            "match_hist_bank": _match_hist_bank}


def _bad(like):
    """(what is wrong, tensor): the wrong dtype, the wrong shape, a non-contiguous view of the right shape and dtype"""
    dt = torch.float32 if like.dtype != torch.float32 else torch.uint8
    big = torch.zeros(tuple(like.shape[:-1]) + (2 * like.shape[-1],), dtype=like.dtype, device=like.device)
    view = big[..., ::2]
    assert view.shape == like.shape and not view.is_contiguous()
    return (("dtype", torch.zeros(like.shape, dtype=dt, device=like.device)),
            ("shape", torch.zeros(tuple(like.shape[:-1]) + (2,), dtype=like.dtype, device=like.device) if like.dim() == 4
             else torch.zeros((1, 4, 5), dtype=like.dtype, device=like.device)),
            ("view", view))


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_out_is_checked_before_any_launch(dev, name):
    from pointcloududa_amd import kernels as K
    run, x = WRAPPERS[name](dev), _image(dev)
    want = run(x)
    assert want.dtype == torch.uint8 and want.shape == x.shape
    torch.cuda.synchronize()
    for what, out in _bad(x):
        before = K.launch_count()
        with pytest.raises(ValueError, match=r"%s: out must be a contiguous uint8 tensor of shape \[1, 4, 4, 1\]" % name):
            run(x, out=out)
        assert K.launch_count() == before, (name, what)
        assert not out.any(), "nothing was written"
    with pytest.raises(ValueError, match="out must be a contiguous"):
        run(x, out=torch.zeros(x.shape, dtype=torch.uint8))                 # a host tensor
    out = torch.full_like(x, 255)
    got = run(x, out=out)
    assert got is out and torch.equal(got, want)


def test_geometric_labels_out_is_checked_before_any_launch(dev):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.utils.geometric import GeoProgram, upload_geo_program
    up = upload_geo_program(GeoProgram.identity(1, 1), 1, 4, 4, dev)
    x = _image(dev)
    lab = (torch.arange(16, dtype=torch.int32, device=dev).reshape(1, 4, 4) % 5)
    want, want_lab = K.geometric(x, lab, *up)
    assert torch.equal(want_lab, lab) and want_lab.data_ptr() != lab.data_ptr()
    for what, lout in _bad(lab):
        before = K.launch_count()
        with pytest.raises(ValueError, match=r"geometric: labels_out must be a contiguous int32 tensor of shape \[1, 4, 4\]"):
            K.geometric(x, lab, *up, labels_out=lout)
        assert K.launch_count() == before, what
        assert not lout.any(), "nothing was written"
    out, lout = torch.full_like(x, 255), torch.full_like(lab, -1)
    got, got_lab = K.geometric(x, lab, *up, out=out, labels_out=lout)
    assert got is out and got_lab is lout and torch.equal(got, want) and torch.equal(got_lab, want_lab)
    # without labels there is no labels_out to write: it is not looked at
    assert K.geometric(x, None, *up, labels_out=lout)[1] is None
