"""CPU check that the oracle follows the dtype (and device) of its parameters: run in float64 it equals the float32
oracle to float32 rounding, one network pass with gradients and one whole OracleTrainer.step, and its default (float32,
host) behaviour is the one the golden tests pin.  The float64 form is the reference of test_production_grads_gpu.py.

The max over points of PointNetCls (and the other argmax / sign routings) take other branches on near-ties between the
two precisions, so the float64 run is anchored to the float32 run's values (oracle.nets.anchored, as the GPU tests anchor
the reference to the HIP kernels): every anchored layer's own float64 output must match the float32 value to rounding
BEFORE it is replaced, and the gradients then compare the backward arithmetic of the two precisions."""
import numpy as np
import torch

from oracle import losses as OL
from oracle import nets as ON
from oracle.step import OracleTrainer, StepCfg
from oracle.synth import synth_batch

# float32 against float64 over the same arithmetic: each of the ~40 layers of the segmenter rounds its outputs to 2^-24
# of their scale and sums of up to ~10^4 terms add ~sqrt(n) such roundings; measured 1e-6 .. 2e-5 on these cases.  A
# dtype or device slip (an input left in float32, a constant built on the wrong type) shows up at 1e-3 or above.
FP32_TOL = 1e-4


def _recorder():
    """float32 run: the value at every anchor point, in call order"""
    seq = []

    def fn(tag, z):
        seq.append((tag, z.detach().clone()))
        return z
    return seq, fn


def _replayer(seq, worst):
    """float64 run: the same anchor points in the same order take the float32 values (layer-local error checked)"""
    it = iter(seq)

    def fn(tag, z):
        t, v = next(it)
        assert t == tag and z.dtype == torch.float64, (t, tag, z.dtype)
        e = float((z.detach() - v.double()).abs().max()) / max(1e-30, float(v.abs().max()))
        worst[0] = max(worst[0], e)
        assert e < FP32_TOL, (tag, e)
        return z + (v.double() - z).detach()
    return fn


def _grad_params(p):
    return {k: (v.clone().requires_grad_(True) if ON.is_trainable(k) else v.clone()) for k, v in p.items()}


def _worst(g32, g64, parts=None):
    """worst error relative to the gradient's scale; with ``parts`` (the source pass's share of a discriminator gradient,
    whose source and target passes largely cancel) relative to the larger part's scale"""
    worst = ("", 0.0)
    total = sum(float(g.norm()) ** 2 for g in g64.values()) ** 0.5
    for k, g in g64.items():
        assert g32[k].dtype == torch.float32 and g.dtype == torch.float64, k
        diff = float((g32[k].double() - g).abs().max())
        if float(g.norm()) < 1e-5 * total:      # a bias in front of a BatchNorm: zero gradient, rounding noise on both
            assert float(g32[k].double().norm()) < 1e-4 * total, k        # sides (anchor_helpers.compare_grads' rule)
            continue
        scale = float(g.abs().max())
        if parts is not None:
            scale = max(scale, float(parts[k].abs().max()), float((g - parts[k]).abs().max()))
        e = diff / scale
        worst = max(worst, (k, e), key=lambda t: t[1])
    return worst


def _net_pass(dt, cfg, p32, pn32, img, mask, vert, pts):
    """segmenter (softmax loss + point loss) and PointNetCls with both T-Nets: losses, gradients"""
    p = _grad_params(ON.params_to(p32, dt))
    assert p["encoder.encoder1.0.weight"].dtype == dt and p["encoder.encoder1.2.num_batches_tracked"].dtype == torch.long
    lo, ve = ON.seg_forward(p, torch.as_tensor(img, dtype=dt), cfg, training=True)
    m, j = OL.seg_loss_softmax(lo, torch.as_tensor(mask, dtype=dt))
    loss = m + j + OL.batch_nn_loss(ve, torch.as_tensor(vert, dtype=dt))
    loss.backward()
    q = _grad_params(ON.params_to(pn32, dt))          # T-Nets: the identity added to fc3 follows the dtype
    y, _, tf = ON.pointnet_cls_forward(q, torch.as_tensor(pts, dtype=dt), feature_transform=True, ext=True, drop=0.0)
    lq = OL.bce_logits_const(y, 1.0) + ON.feature_transform_regularizer(tf)
    lq.backward()
    assert lo.dtype == dt and y.dtype == dt
    return ((float(loss.detach()), float(lq.detach())),
            {k: v.grad for d in (p, q) for k, v in d.items() if ON.is_trainable(k) and v.grad is not None})


def test_fp64_oracle_networks_equal_fp32_to_rounding():
    cfg = ON.SegCfg(filters=4, in_channels=3, n_class=5, pointnet=True, fc_inch=9)
    p32 = ON.make_params(ON.seg_param_shapes(cfg), 21)
    img, mask, vert, _, _ = synth_batch(2, 3, 5, 128, seed=22)
    pn32 = ON.make_params(ON.pointnet_cls_param_shapes(True, ext=True), 23)
    pts = np.random.default_rng(24).random((3, 3, 300), dtype=np.float32)
    grads, losses = {}, {}
    seq, rec = _recorder()
    pre = [0.0]
    for dt in (torch.float32, torch.float64):
        with ON.anchored(rec if dt == torch.float32 else _replayer(seq, pre)):
            losses[dt], grads[dt] = _net_pass(dt, cfg, p32, pn32, img, mask, vert, pts)
    for a, b in zip(losses[torch.float32], losses[torch.float64]):
        assert abs(a - b) <= FP32_TOL * max(1.0, abs(b)), (a, b)
    assert set(grads[torch.float32]) == set(grads[torch.float64])
    worst = _worst(grads[torch.float32], grads[torch.float64])
    assert worst[1] < FP32_TOL, worst
    assert 0.0 < pre[0] < FP32_TOL


def test_fp64_oracle_step_equals_fp32_to_rounding():
    cfg = ON.SegCfg(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9)
    pg = ON.make_params(ON.seg_param_shapes(cfg), 31)
    p1 = ON.make_params(ON.disc_param_shapes(4), 32, std=0.02)
    p2 = ON.make_params(ON.disc_param_shapes(4), 33, std=0.02)
    p4 = ON.make_params(ON.pointnet_cls_param_shapes(), 34)
    batch = synth_batch(4, 1, 4, 128, seed=35)
    scfg = StepCfg(n_class=4)
    seq, rec = _recorder()
    o32 = OracleTrainer(cfg, scfg, pg, p1, p2, p4)
    with ON.anchored(rec):
        out32 = o32.step(*batch, keep=True)
    # the default path is untouched: the float32 trainer takes the same numbers from already-converted parameters
    o32b = OracleTrainer(cfg, scfg, *(ON.params_to(p, torch.float32) for p in (pg, p1, p2, p4)))
    assert o32b.step(*batch) == out32
    o64 = OracleTrainer(cfg, scfg, *(ON.params_to(p, torch.float64) for p in (pg, p1, p2, p4)))
    pre = [0.0]
    with ON.anchored(_replayer(seq, pre)):
        out64 = o64.step(*batch, keep=True)
    assert 0.0 < pre[0] < FP32_TOL
    assert set(out32) == set(out64)
    for k, v in out64.items():
        assert abs(out32[k] - v) <= FP32_TOL * max(1.0, abs(v)), (k, out32[k], v)
    for nm in ("grad_seg", "grad_total", "grad_d1", "grad_d2", "grad_d4"):
        worst = _worst(o32.kept[nm], o64.kept[nm], o64.kept.get(nm + "_src"))
        assert worst[1] < FP32_TOL, (nm, worst)
    # and the discriminators' parameters after their SGD steps (in torch.optim, on the float64 parameters).  (Adam's
    # first step on the segmenter is lr * g / (|g| + eps), a sign for every element: near-zero gradient elements flip it
    # between the precisions, so the segmenter's update is not a rounding-level comparison.)
    for nm, a, b in (("grad_d1", o32.dis1, o64.dis1), ("grad_d2", o32.dis2, o64.dis2), ("grad_d4", o32.dis4, o64.dis4)):
        g = o64.kept[nm]
        total = sum(float(v.norm()) ** 2 for v in g.values()) ** 0.5
        for k in b:
            if b[k].is_floating_point():
                assert b[k].dtype == torch.float64
                if k in g and float(g[k].norm()) < 1e-5 * total:
                    continue
                e = float((a[k].detach().double() - b[k].detach()).abs().max()) / max(1e-30, float(b[k].abs().max()))
                assert e < FP32_TOL, (k, e)
