"""Guarded optimiser steps through the trainer and train_epoch: TrainCfg.clip_gen / clip_dis / skip_nonfinite
(args.clip / args.clip_d / args.skip_nonfinite), decided on the device inside the step.

Configuration: filters 4, B = 2, 96 x 96 -- the smallest image the segmenter's point head accepts ((96 / 16 - 5)^2 = 1 input
of its fully connected layer); the step tests' own small cases run 128 x 128 with B = 4.

BatchNorm running statistics are not compared after a poisoned step: the forward pass that saw the NaN has written them
before any gradient exists, and the guard does not roll them back."""
import functools
import types

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

CFG_KW = dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=1)
B, HW = 2, 96


def _build(dev, seed=3100, **flags):
    from oracle import nets as ON
    from pointcloududa_amd.networks import PointNetCls, Segmentation_model_Point, UncertaintyDiscriminator
    from pointcloududa_amd.train_step import AdversarialTrainer, TrainCfg
    cfg = ON.SegCfg(**CFG_KW)
    ps = (ON.make_params(ON.seg_param_shapes(cfg), seed), ON.make_params(ON.disc_param_shapes(4), seed + 1, std=0.02),
          ON.make_params(ON.disc_param_shapes(4), seed + 2, std=0.02), ON.make_params(ON.pointnet_cls_param_shapes(), seed + 3))
    load = lambda m, p: (m.load_state_dict({k: v.clone() for k, v in p.items()}), m.to(dev).train())[1]
    return AdversarialTrainer(load(Segmentation_model_Point(**CFG_KW), ps[0]), load(UncertaintyDiscriminator(in_channel=4), ps[1]),
                              load(UncertaintyDiscriminator(in_channel=4), ps[2]), load(PointNetCls(drop=0.0), ps[3]),
                              TrainCfg(n_class=4, **flags))


@functools.lru_cache(maxsize=None)
def _batch_np(i):
    from oracle.synth import synth_batch
    return synth_batch(B, 1, 4, HW, seed=3200 + i)


def _batch(dev, i, poison=False):
    t = [torch.from_numpy(a).to(dev) for a in _batch_np(i)]
    if poison:
        t[0][0, 0, 17, 23] = float("nan")              # one pixel of img_a
    return t


def _opts(tr):
    return [("gen", tr.opt_gen), ("d1", tr.opt_d1), ("d2", tr.opt_d2), ("d4", tr.opt_d4)]


def _state(tr):
    """parameters and optimiser state of every network (not the BatchNorm running statistics)"""
    out = {}
    for nm, o in _opts(tr):
        for k in ("p", "m", "v", "buf", "step_t"):
            if getattr(o, k, None) is not None:
                out[nm + "." + k] = getattr(o, k).clone()
    return out


def _norm64(t):
    return float(np.sqrt((t.double().cpu().numpy() ** 2).sum()))


# ------------------------------------------------------------------------------------------------ 9. no regression
@gpu
def test_guard_that_never_acts_changes_no_bit(dev):
    ref, tr = _build(dev), _build(dev, clip_gen=1e30, clip_dis=1e30, skip_nonfinite=True)
    assert ref.opt_gen.guard is None and all(o.guard is not None for _, o in _opts(tr))
    for i in range(2):
        o0, o1 = ref.step(*_batch(dev, i)), tr.step(*_batch(dev, i))
        extra = {"grad_norm_" + n for n, _ in _opts(tr)} | {"skipped_" + n for n, _ in _opts(tr)}
        assert set(o1) - set(o0) == extra and set(o0) <= set(o1)
        for k in o0:
            assert torch.equal(o0[k], o1[k]), k
        assert all(float(o1["skipped_" + n]) == 0.0 and np.isfinite(float(o1["grad_norm_" + n])) for n, _ in _opts(tr))
    s0, s1 = _state(ref), _state(tr)
    assert set(s0) == set(s1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert int(tr.opt_gen.step_t) == 2 and all(int(o.guard[4]) == 2 and int(o.skipped) == 0 for _, o in _opts(tr))


# ------------------------------------------------------------------------------------------------ 10. clipping acts
@gpu
def test_reported_norm_and_clipped_update(dev):
    from pointcloududa_amd.optim import FusedSGD
    clip = 0.05
    tr = _build(dev, clip_gen=clip, clip_dis=1e30)
    # an SGD segmenter without momentum or weight decay: the first step's parameter change IS lr * the clipped gradient
    lr = 0.1
    tr.opt_gen = FusedSGD(tr.gen, lr=lr, momentum=0.0, weight_decay=0.0, max_grad_norm=clip)
    p_before = tr.opt_gen.p.clone()
    out = tr.step(*_batch(dev, 0))
    for nm, o in _opts(tr):
        want = np.float32(_norm64(o.g))                # the gradient buffer as the update saw it (zeroed by the NEXT step)
        got = np.float32(float(out["grad_norm_" + nm]))
        print(nm, "reported norm %.9g, float64 norm of the buffer %.9g" % (got, want))
        assert abs(np.float64(got) - np.float64(want)) <= np.spacing(want), (nm, got, want)
    norm = float(out["grad_norm_gen"])
    assert norm > clip, "the test's clip_gen is meant to clip (norm %g)" % norm
    delta = _norm64(tr.opt_gen.p - p_before)
    want = lr * min(norm, clip)
    print("update norm %.9g, lr * min(norm, clip) %.9g" % (delta, want))
    assert abs(delta - want) <= 1e-5 * want
    assert float(tr.opt_gen.clip_coef) < 1.0 and all(float(o.clip_coef) == 1.0 for _, o in _opts(tr)[1:])


# ------------------------------------------------------------------------------------------------ 11. poison
@gpu
def test_one_nan_pixel_skips_every_update(dev):
    tr = _build(dev, skip_nonfinite=True)
    tr.step(*_batch(dev, 0))
    before = _state(tr)
    out = tr.step(*_batch(dev, 1, poison=True))
    norms = {n: float(out["grad_norm_" + n]) for n, _ in _opts(tr)}
    print("norms of the poisoned step:", norms)
    assert all(not np.isfinite(v) for v in norms.values()), norms
    after = _state(tr)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert all(float(out["skipped_" + n]) == 1.0 for n, _ in _opts(tr))
    assert int(tr.opt_gen.step_t) == 1 and all(int(o.skipped) == 1 for _, o in _opts(tr))
    out = tr.step(*_batch(dev, 2))                     # a clean step applies
    assert all(float(out["skipped_" + n]) == 0.0 and np.isfinite(float(out["grad_norm_" + n])) for n, _ in _opts(tr))
    final = _state(tr)
    assert int(tr.opt_gen.step_t) == 2
    for nm, _ in _opts(tr):
        assert not torch.equal(final[nm + ".p"], after[nm + ".p"]), nm
        assert bool(torch.isfinite(final[nm + ".p"]).all()), nm


# ------------------------------------------------------------------------------------------------ 12. epoch
def _gen(batches, which):
    for img_a, mask_a, vert_a, img_b, vert_b in batches:
        yield (img_a, mask_a, vert_a) if which == "A" else (img_b, np.zeros_like(mask_a), vert_b)


@gpu
def test_train_epoch_counts_skipped_steps(dev):
    import pointcloududa_amd.train_mscmrseg as TM
    batches = [list(_batch_np(i)) for i in range(3)]
    bad = batches[1][0].copy()
    bad[1, 0, 40, 41] = np.nan
    batches[1][0] = bad
    base = dict(d1=True, d2=True, d4=True, dr=0.01, wp=1.0)
    today = {"seg_loss", "seg_dice", "dis1_acc1", "dis1_acc2", "dis2_acc1", "dis2_acc2", "dis4_acc1", "dis4_acc2", "ver_s_loss",
             "ver_t_loss"}

    def run(**extra):
        tr = _build(dev)
        nets = (tr.gen, tr.dis2, tr.dis4, tr.dis1)
        og = torch.optim.Adam(tr.gen.parameters(), lr=1e-3, betas=(0.9, 0.99))
        mk = lambda m: torch.optim.SGD(m.parameters(), lr=2.5e-5, momentum=0.99, weight_decay=0.0005)
        TM.args = types.SimpleNamespace(**base, **extra)
        res = TM.train_epoch(*nets, og, mk(tr.dis2), mk(tr.dis4), mk(tr.dis1), _gen(batches, "A"), _gen(batches, "B"))
        return res, tr.gen

    res, gen = run(skip_nonfinite=True)
    print(res)
    assert res["skipped_steps"] == 1.0
    assert set(res) == today | {"skipped_steps"} | {"grad_norm_" + n for n in ("gen", "d1", "d2", "d4")} | \
        {"skipped_" + n for n in ("gen", "d1", "d2", "d4")}
    assert all(abs(res["skipped_" + n] - 1.0 / 3.0) < 1e-6 for n in ("gen", "d1", "d2", "d4"))
    assert all(bool(torch.isfinite(p).all()) for p in gen.parameters())
    assert int(gen._pcuda_trainer[1].opt_gen.step_t) == 2
    res, gen = run()                                   # the option absent: today's keys, and the NaN goes through
    assert set(res) == today
    assert not all(bool(torch.isfinite(p).all()) for p in gen.parameters())


# ------------------------------------------------------------------------------------------------ 13. CPU
def test_defaults_are_off_and_allocate_nothing():
    from pointcloududa_amd.optim import FusedAdam, FusedSGD
    from pointcloududa_amd.train_step import TrainCfg
    c = TrainCfg()
    assert (c.clip_gen, c.clip_dis, c.skip_nonfinite) == (0.0, 0.0, False)
    m = torch.nn.Linear(3, 2)
    a = FusedAdam(m)
    assert a.guard is None and not a.guarded and not hasattr(a, "_norm_ws")
    s = FusedSGD(torch.nn.Linear(3, 2))
    assert s.guard is None and not s.guarded and not hasattr(s, "init_t")
    g = FusedAdam(torch.nn.Linear(3, 2), max_grad_norm=1.0)
    assert g.guarded and g.guard is not None and g.guard.numel() == 8 and g.guard.dtype == torch.int32
    g = FusedSGD(torch.nn.Linear(3, 2), skip_nonfinite=True)
    assert g.guarded and int(g.init_t) == 0 and int(g.skipped) == 0
    with pytest.raises(RuntimeError):
        a.grad_norms(["weight"])
