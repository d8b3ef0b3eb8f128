"""Child process of tests/test_pointnet_small_net_gpu.py: ``python pointnet_small_child.py <out.npz>``.

``PCUDA_PN_SMALL`` is read once per process (pointcloududa_amd.kernels), hence a process per setting.  Runs PointNetCls forward
and backward in training mode at batch 4 with 300 points, for the default net and for ``feature_transform=True, ext=True``, on
seeded parameters and inputs, and writes every output, every parameter gradient, the BatchNorm running statistics and the
number of kernel launches of the library to the .npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

CONFIGS = {"default": {}, "ft_ext": dict(feature_transform=True, ext=True)}


def main(out_path):
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.networks import PointNetCls
    dev = torch.device("cuda", 0)
    res = {}
    for name, kw in CONFIGS.items():
        torch.manual_seed(7)
        net = PointNetCls(drop=0.3, **kw)
        for k, b in net.named_buffers():      # (running_var away from 1, so that its update is visible)
            if k.endswith("running_var"):
                b.mul_(0.5)
        net = net.to(dev).train()
        x = torch.randn(4, 3, 300).to(dev).requires_grad_(True)
        mask = ((torch.rand(4, 256) < 0.7).float() / 0.7).to(dev)
        wy, wt = torch.randn(4, 1).to(dev), torch.randn(4, 3, 3).to(dev)
        n0 = K.launch_count()
        y, trans, trans_feat = net(x, drop_mask=mask)
        loss = (y * wy).sum() + (trans * wt).sum()
        if trans_feat is not None:
            loss = loss + (trans_feat * trans_feat).sum() * 0.01
        loss.backward()
        torch.cuda.synchronize()
        res[name + "/launches"] = np.int64(K.launch_count() - n0)
        res[name + "/y"] = y.detach().cpu().numpy()
        res[name + "/trans"] = trans.detach().cpu().numpy()
        if trans_feat is not None:
            res[name + "/trans_feat"] = trans_feat.detach().cpu().numpy()
        res[name + "/dx"] = x.grad.cpu().numpy()
        for k, p in net.named_parameters():
            if p.grad is not None:
                res[name + "/grad/" + k] = p.grad.cpu().numpy()
        for k, b in net.named_buffers():
            if "running" in k and ".in" not in k and not k.startswith("in"):
                res[name + "/buf/" + k] = b.cpu().numpy()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
