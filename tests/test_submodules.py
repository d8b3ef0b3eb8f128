"""The segmenter's and PointNet's sub-modules called on their own (CPU side): no CPU fallback, the reference's module
trees, and the fixture tests/golden/submodules_small.npz regenerating from the reference."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

REF_SRC = "/root/reference/src"


def _gold():
    return np.load(os.path.join(GOLD, "submodules_small.npz"))


def _modules():
    from pointcloududa_amd.networks import (Bottleneck, Decoder, Encoder, PointNet, PointNetfeat, Segmentation_model_Point,
                                            STN3d, STNkd)
    seg = Segmentation_model_Point(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9)
    nobn = Segmentation_model_Point(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9, batchnorm=False)
    ext = Segmentation_model_Point(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9, extpn=True)
    return {
        "encoder": seg.encoder, "bottleneck": seg.bottleneck, "pointNet": seg.pointNet, "decoder": seg.decoder,
        "seg_nobn_encoder": nobn.encoder, "seg_nobn_decoder": nobn.decoder, "pointNet_ext": ext.pointNet,
        "standalone_encoder": Encoder(filters=4, in_channels=1), "standalone_bottleneck": Bottleneck(filters=4),
        "standalone_pointNet": PointNet(fc_inch=9, conv_inch=64), "standalone_decoder": Decoder(filters=4),
        "stn3d": STN3d(), "stnkd": STNkd(k=64), "feat": PointNetfeat(), "feat_local": PointNetfeat(global_feat=False),
        "feat_ft_ext": PointNetfeat(feature_transform=True, ext=True),
        "feat_ft_local": PointNetfeat(feature_transform=True, global_feat=False),
        "feat_nost": PointNetfeat(sample_transform=False),
    }


def test_every_submodule_refuses_cpu_inputs():
    mods = _modules()
    x = {"encoder": torch.zeros(2, 1, 32, 32), "bottleneck": torch.zeros(2, 32, 2, 2),
         "pointNet": torch.zeros(2, 64, 8, 8), "stn3d": torch.zeros(2, 3, 16), "stnkd": torch.zeros(2, 64, 16)}
    for name, m in mods.items():
        kind = next((k for k in ("encoder", "bottleneck", "pointNet", "decoder", "stn3d", "stnkd") if k in name), "feat")
        with pytest.raises(RuntimeError, match="HIP devices only"):
            if kind == "decoder":
                skip = [torch.zeros(2, 4 * 2 ** i, 32 >> i, 32 >> i) for i in range(4)]
                m(torch.zeros(2, 64, 2, 2), skip)
            else:
                m(x.get(kind, torch.zeros(2, 3, 16)))


def test_decoder_keeps_the_skip_list_on_a_refused_call():
    from pointcloududa_amd.networks import Decoder
    skip = [torch.zeros(2, 4 * 2 ** i, 32 >> i, 32 >> i) for i in range(4)]
    with pytest.raises(RuntimeError, match="HIP"):
        Decoder(filters=4)(torch.zeros(2, 64, 2, 2), skip)
    assert len(skip) == 4
    short = skip[:3]
    with pytest.raises(IndexError):
        Decoder(filters=4)(torch.zeros(2, 64, 2, 2), short)
    assert len(short) == 3


def test_refused_variants_raise_not_implemented():
    from pointcloududa_amd.networks import Decoder, Encoder, PointNetfeat
    with pytest.raises(NotImplementedError):
        Decoder(drop=True)
    with pytest.raises(NotImplementedError):
        PointNetfeat(kernel_size=3)
    with pytest.raises(NotImplementedError):
        Encoder(filters=4, in_channels=1, kernel_size=(5, 5))(torch.zeros(2, 1, 32, 32))
    with pytest.raises(NotImplementedError):
        Decoder(filters=4, padding="valid")(torch.zeros(2, 64, 2, 2), [])


def test_submodules_keep_the_reference_state_dict():
    """PointNetfeat(global_feat=False) constructs; every sub-module's keys and shapes are the reference's"""
    g = _gold()
    for name, m in _modules().items():
        key = name.replace("standalone_", "")
        sd = m.state_dict()
        assert list(sd.keys()) == list(g["keys__" + key]), name
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g["kshapes__" + key]), name


def test_submodules_in_a_network_share_its_engine():
    from pointcloududa_amd.networks import Segmentation_model, Segmentation_model_Point
    m = Segmentation_model_Point(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9)
    for name in ("encoder", "bottleneck", "pointNet", "decoder"):
        eng, P = getattr(m, name)._stage_engine()
        assert eng is m._engine
        assert all(P[k] is v for k, v in m._tensor_dict().items() if k.startswith(name + "."))
    f = Segmentation_model(filters=32, feature_dis=True)      # _build_engine runs twice: the sub-modules follow
    assert f.encoder._stage_engine()[0] is f._engine
    assert all(op.owner is f for op in f._engine.ops.values())


def test_generator_check():
    if not os.path.isdir(REF_SRC):
        pytest.skip("the reference sources are not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_submodule_golden.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
