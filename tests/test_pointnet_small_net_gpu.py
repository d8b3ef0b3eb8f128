"""PointNetCls with and without the small-tensor kernels of csrc/pointnet_small.hip (``PCUDA_PN_SMALL=0`` selects the call
sequence they replace: one element per workgroup on [B, C], the dense gradient behind the max over points).  Forward and
backward at batch 4 with 300 points in a child process per setting (tests/pointnet_small_child.py; the switch is read once
per process): every output, every parameter gradient and every running statistic must be bit-equal, for the default net and
for ``feature_transform=True, ext=True``; and the default setting must issue fewer launches.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pointnet_small_child.py")


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    out = {}
    for setting in ("1", "0"):
        path = str(tmp_path_factory.mktemp("pn_small") / ("pn_small_%s.npz" % setting))
        r = subprocess.run([sys.executable, CHILD, path], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, PCUDA_PN_SMALL=setting))
        assert r.returncode == 0, "child (PCUDA_PN_SMALL=%s) failed:\n%s\n%s" % (setting, r.stdout[-2000:], r.stderr[-4000:])
        out[setting] = dict(np.load(path))
    return out


@pytest.mark.parametrize("config", ["default", "ft_ext"])
def test_network_is_bit_equal_under_both_settings(runs, config):
    new, old = runs["1"], runs["0"]
    keys = sorted(k for k in new if k.startswith(config + "/") and not k.endswith("/launches"))
    assert keys == sorted(k for k in old if k.startswith(config + "/") and not k.endswith("/launches"))
    assert any("/grad/" in k for k in keys) and any("/buf/" in k for k in keys) and config + "/dx" in keys
    bad = [k for k in keys if new[k].tobytes() != old[k].tobytes()]
    assert not bad, "differ between PCUDA_PN_SMALL=1 and 0: %s" % bad[:10]
    assert all(np.isfinite(new[k]).all() for k in keys)
    assert float(np.abs(new[config + "/grad/feat.stn.conv1.weight"]).max()) > 0
    # 4 [B, C] BatchNorm layers per T-Net / head: 6 launches -> 2 each; one scatter less per max over points
    assert int(new[config + "/launches"]) < int(old[config + "/launches"]), (new[config + "/launches"], old[config + "/launches"])
