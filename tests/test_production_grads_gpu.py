"""Gradients at the benchmark's sizes and schedule, against a float64 reference anchored to the HIP forward values.

test_backward_exact_gpu.py holds every gradient to 1e-4 at batch 2-4 on small maps, and its whole-step case switches the
production schedule off.  The kernels the benchmark's batch sizes select (the anti-phase ``conv3ap`` and row-streaming
``conv3rs`` kernels, the ``wgrad3`` / ``wgrad3r`` rules of 128+ px maps, the 8-loads-per-lane BatchNorm finalize of the
8192-tile layers) and the schedule it runs (discriminators on side streams under the adversarial backward pass, the
frozen pass replayed for the update, source + target as one 2B backward pass) are checked here, built the way bench.py
builds each WORKLOADS entry (filters 32, its classes, channels, fc_inch, variant, PointNetCls flags and per-rank batch;
PointNetCls's dropout at 0 so that both sides draw the same mask), with the trainer's schedule and the dispatch at their
defaults.

The reference is oracle.nets / oracle.step in float64 on the GPU through stock PyTorch operators (not this project's
kernels), anchored layer by layer to the HIP values (anchor_helpers): every layer's own forward error is held to
PRE_TOL before it is anchored, then every gradient to TOL (segmenter through the whole step: SEG_CHAIN_TOL).  Each case
also pins the kernel families its launches come from, checks that no launch fell back to the generic kernels, and that
the recording hooks leave the launch sequence unchanged.
"""
import os
import re
import tempfile

import numpy as np
import pytest
import torch

from anchor_helpers import (SEG_CHAIN_TOL, TOL, anchor_from, compare_grads, disc_table, flat_named, load, pn_table,
                            rel_err, seg_table)

pytestmark = pytest.mark.gpu

# kernel families (launch tag up to its first " n<batch>" field) each case must launch at its production size: a dispatch
# rule that moves these shapes onto other kernels fails the case instead of passing on the ordinary tiles.  Required, not
# exhaustive: the first-layer direct weight-gradient kernel ("direct d1 wgrad", eligible only for 16-byte aligned inputs)
# appeared in one full_uda step run and not in another at the same shapes; families beyond these are printed.
_SEG = {"conv3ap", "conv3rs", "direct 1x1 dgrad+bnred", "direct 1x1 fwd", "igemm", "wgrad", "wgrad1", "wgrad3r"}
_ONE_CHANNEL = {"direct c1 fwd", "direct c1 wgrad"}                # first segmenter layer on a 1-channel image
_DISC = {"direct d1 fwd (mfma)", "direct d1 dgrad", "direct d5 fwd", "igemm", "wgrad"}
_PN = {"conv1d f32 fwd", "conv1d f32 dgrad", "conv1d f32 wgrad"}
FAMILIES = {
    "full_uda step": _SEG | {"wgrad3"} | _ONE_CHANNEL | _DISC | _PN,
    "mmwhs_uda step": _SEG | {"wgrad3"} | _DISC | _PN,
    "uda_512 segmenter": _SEG | {"wgrad3"} | _ONE_CHANNEL,
    "mscmrseg_224 segmenter": _SEG,
    "unet_d2 segmenter": _SEG | {"wgrad3"} | _ONE_CHANNEL,
    "uda_512 discriminator": {"igemm", "wgrad"},
    "mscmrseg_224 discriminator": _DISC | {"direct d1 wgrad"},
    "unet_d2 discriminator": _DISC | {"direct d1 wgrad"},
}


def _workload(name):
    import bench
    return bench.WORKLOADS[name]


def _family(tag):
    return re.split(r" n\d", tag, maxsplit=1)[0]


def _launch_tags(fn):
    """run ``fn`` with the library's launch profile on: -> (fn's result, the launch tags in issue order)"""
    from pointcloududa_amd import kernels as K
    torch.cuda.synchronize()
    K.prof_enable(True)
    K.prof_reset()
    try:
        res = fn()
        torch.cuda.synchronize()
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "prof.csv")
            K.prof_dump(path)
            lines = open(path).read().splitlines()[1:]
    finally:
        K.prof_enable(False)
        K.prof_reset()
    return res, [ln.split(",", 3)[3] for ln in lines]


def _check_dispatch(case, plain, hooked, fb0):
    from pointcloududa_amd import kernels as K
    assert hooked == plain, "the recording hooks changed the launch sequence (%d vs %d launches)" % (len(hooked), len(plain))
    assert K.fallback_count() == fb0, "launches fell back to the generic kernels"
    fams = sorted({_family(t) for t in plain if t})
    print("%s: %d launches, kernel families: %s" % (case, len(plain), ", ".join(fams)))
    assert FAMILIES[case] <= set(fams), (case, "missing", sorted(FAMILIES[case] - set(fams)))


def _setup(name):
    wl = _workload(name)
    nc, cin = wl.get("n_class", 4), wl.get("in_channels", 1)
    cfg_kw = dict(filters=32, in_channels=cin, n_class=nc, pointnet=wl["d4"], fc_inch=wl.get("fc_inch", 121))
    return wl, nc, cin, wl.get("hw", 256), wl.get("variant", "mscmrseg"), cfg_kw, wl.get("pn", {})


def _ref_params(p, dev):
    from oracle import nets as ON
    return ON.params_to(p, torch.float64, dev)


# ------------------------------------------------------------------------------------------------ a. the whole step
@pytest.mark.parametrize("name,seed", [("full_uda", 2000), ("mmwhs_uda", 2010)])
def test_production_step_gradients(dev, name, seed):
    """One train step of the workload at its batch with the default schedule, every oracle pass anchored to the HIP pass
    of the same network, role and samples: the segmenter's source and target passes; per image discriminator the frozen
    adversarial pass on the target batch, the source batch written in front of it (``forward_fill``) and the replay of
    the frozen pass over both (its target half IS the frozen pass); PointNetCls's three passes.  The activations the
    replay consumed must equal, bit for bit, those the frozen pass produced.  Gradients (``tr.last``) as in
    test_train_step_backward_shared_routing: segmenter SEG_CHAIN_TOL, discriminators TOL of their two parts' scale;
    losses 1e-5."""
    import oracle.step as OS
    from oracle import nets as ON
    from oracle.synth import synth_batch
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.networks import PointNetCls, Segmentation_model_Point, UncertaintyDiscriminator
    from pointcloududa_amd.train_step import AdversarialTrainer, TrainCfg
    wl, nc, cin, hw, variant, cfg_kw, pn_kw = _setup(name)
    b = wl["batch"]
    cfg = ON.SegCfg(**cfg_kw)
    pg = ON.make_params(ON.seg_param_shapes(cfg), seed)
    p1 = ON.make_params(ON.disc_param_shapes(nc), seed + 1, std=0.02)
    p2 = ON.make_params(ON.disc_param_shapes(nc), seed + 2, std=0.02)
    p4 = ON.make_params(ON.pointnet_cls_param_shapes(**pn_kw), seed + 3)
    mom = 0.95 if variant == "mmwhs" else 0.99

    def trainer():
        return AdversarialTrainer(load(Segmentation_model_Point(**cfg_kw), pg, dev),
                                  load(UncertaintyDiscriminator(in_channel=nc), p1, dev),
                                  load(UncertaintyDiscriminator(in_channel=nc), p2, dev),
                                  load(PointNetCls(drop=0.0, **pn_kw), p4, dev),
                                  TrainCfg(variant=variant, d1=wl["d1"], d2=wl["d2"], d4=wl["d4"], n_class=nc,
                                           d_momentum=mom))
    batch = synth_batch(b, cin, nc, hw, seed=seed + 100, gaussian=variant == "mmwhs")
    inputs = [torch.from_numpy(t).to(dev) for t in batch]
    fb0 = K.fallback_count()
    tr = trainer()
    _, plain = _launch_tags(lambda: tr.step(*inputs))
    del tr

    tr = trainer()
    assert tr.d_streams and tr.d_overlap and tr.d_batch and tr.early_fwd2 and tr.d_reuse and tr.d_joint
    gen, d1, d2, d4 = tr.gen, tr.dis1, tr.dis2, tr.dis4
    gen._keep_state, d1._keep_acts, d2._keep_acts, d4._keep_trace = True, True, True, True
    # per network, the anchor table of each HIP pass in the order the oracle makes the same pass
    passes = {"gen": [], "d1": [], "d2": [], "d4": []}
    frozen, replayed = {"d1": [], "d2": []}, {"d1": [], "d2": []}

    def spy(mod, name_, make):
        inner = mod.forward

        def fwd(*a, **k):
            out = inner(*a, **k)
            passes[name_].append(make(out))
            return out
        mod.forward = fwd

    def spy_disc(mod, name_):
        inner_fwd, inner_fill, inner_replay = mod.forward, mod.forward_fill, mod.replay

        def fwd(x):
            out = inner_fwd(x)
            acts = mod._last_acts
            if not frozen[name_]:       # the frozen adversarial pass (phase 2): kept for the replay's bit check
                frozen[name_].append([a.clone() for a in acts[1:]])
            if acts[0].shape[0] == 2 * b:      # a 2B pass: its source and target halves (no batch statistics in D)
                passes[name_] += [disc_table(mod, [a[:b] for a in acts], dev), disc_table(mod, [a[b:] for a in acts], dev)]
            else:
                passes[name_].append(disc_table(mod, acts, dev))
            return out

        def fill(x, slot=0):
            inner_fill(x, slot)
            c = mod._cache
            passes[name_].append(disc_table(mod, [x] + [f[slot * b:(slot + 1) * b] for f in c["full"]], dev))

        def replay():
            c = mod._cache
            room = len(c["x"]) - 1
            acts = c["full"] if c["full"] is not None else c["acts"][1:]
            replayed[name_].append([f[room * b:].clone() for f in acts])
            passes[name_].append(passes[name_][0])       # the target pass IS the frozen pass
            return inner_replay()
        mod.forward, mod.forward_fill, mod.replay = fwd, fill, replay
    spy(gen, "gen", lambda out: seg_table(gen._last_S, cfg, out[0], out[2], dev, pools=True))
    spy_disc(d1, "d1")
    spy_disc(d2, "d2")
    spy(d4, "d4", lambda out: pn_table(d4._last_trace, dev))
    out, hooked = _launch_tags(lambda: tr.step(*inputs, keep=True))
    h = AdversarialTrainer.to_host(out, tr.cfg)
    assert [len(passes[k]) for k in ("gen", "d1", "d2", "d4")] == [2, 3, 3, 3]
    # the production path ran: each image discriminator replayed its frozen pass once
    assert len(replayed["d1"]) == len(replayed["d2"]) == 1

    scfg = OS.StepCfg(variant=variant, d1=wl["d1"], d2=wl["d2"], d4=wl["d4"], n_class=nc, d_momentum=mom,
                      pn_feature_transform=bool(pn_kw.get("feature_transform")), pn_ext=bool(pn_kw.get("ext")))
    orc = OS.OracleTrainer(cfg, scfg, *(_ref_params(p, dev) for p in (pg, p1, p2, p4)))
    cur, pre, calls = {}, {k: {} for k in passes}, {k: 0 for k in passes}

    def anchor(tag, z):
        return anchor_from(cur["table"], cur["used"], pre[cur["name"]])(tag, z)
    anchor.pool = lambda tag, x: anchor_from(cur["table"], cur["used"], pre[cur["name"]]).pool(tag, x)

    def enter(name_):
        if "table" in cur:
            assert cur["used"] == set(cur["table"]), (cur["name"], set(cur["table"]) - cur["used"])
        cur["name"], cur["table"], cur["used"] = name_, passes[name_][calls[name_]], set()
        calls[name_] += 1
    real = (OS.seg_forward, OS.disc_forward, OS.pointnet_cls_forward)

    def seg_fw(p, x, c, training=True):
        enter("gen")
        return real[0](p, x, c, training=training)

    def disc_fw(p, x, ext=False):
        enter("d1" if p is orc.dis1 else "d2")
        return real[1](p, x, ext=ext)

    def pn_fw(p, x, **k):
        enter("d4")
        return real[2](p, x, **k)
    OS.seg_forward, OS.disc_forward, OS.pointnet_cls_forward = seg_fw, disc_fw, pn_fw
    try:
        with ON.anchored(anchor):
            q = orc.step(*batch, keep=True)
    finally:
        OS.seg_forward, OS.disc_forward, OS.pointnet_cls_forward = real
    assert calls == {"gen": 2, "d1": 3, "d2": 3, "d4": 3}
    assert cur["used"] == set(cur["table"])

    report = []
    for nm, mod in (("grad_seg", gen), ("grad_total", gen), ("grad_d1", d1), ("grad_d2", d2), ("grad_d4", d4)):
        w = compare_grads(flat_named(mod, tr.last[nm]), orc.kept[nm], tol=SEG_CHAIN_TOL if mod is gen else TOL,
                          parts=orc.kept.get(nm + "_src"))
        report.append("%s %s %.2e" % (nm, w[0], w[1]))
    keys = ["seg_loss", "adv_loss", "ver_s_loss", "ver_t_loss"] + ["d%d_loss_%s" % (i, t) for i in (1, 2, 4)
                                                                   for t in ("src", "tgt")]
    if variant == "mmwhs":
        keys += ["entropy_loss", "entropy_loss_T"]
    for k in keys:
        assert abs(h[k] - q[k]) <= 1e-5 * max(1.0, abs(q[k])), (k, h[k], q[k])
    for nm in ("d1", "d2"):
        for li, (a, r) in enumerate(zip(frozen[nm][0], replayed[nm][0])):
            assert torch.equal(a, r), "%s layer %d: the replay consumed other activations than the frozen pass made" % (nm, li)
    print("%s B=%d step: worst gradient errors: %s; worst layer-local forward error: %s"
          % (name, b, "; ".join(report),
             ", ".join("%s %s %.2e" % (k, v.get("tag"), v.get("e", 0.0)) for k, v in pre.items())))
    _check_dispatch(name + " step", plain, hooked, fb0)


# ------------------------------------------------------------------------------------------------ b. per network
def _seg_case(dev, name, seed):
    from oracle import losses as OL
    from oracle import nets as ON
    from oracle.synth import synth_batch
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.networks import Segmentation_model_Point
    from pointcloududa_amd.utils import loss as L
    wl, nc, cin, hw, variant, cfg_kw, _ = _setup(name)
    b = wl["batch"]
    softmax = variant == "mmwhs"
    cfg = ON.SegCfg(**cfg_kw)
    params = ON.make_params(ON.seg_param_shapes(cfg), seed)
    img, mask, vert, _, _ = synth_batch(b, cin, nc, hw, seed=seed + 1, gaussian=variant == "mmwhs")

    def run(keep):
        model = load(Segmentation_model_Point(**cfg_kw), params, dev)
        model._keep_state = keep
        x = torch.from_numpy(img).to(dev).requires_grad_(True)
        logits, _, verts = model(x)
        one = torch.ones((), device=dev)
        l_main, l_jac = L.seg_loss(logits, torch.from_numpy(mask).to(dev), "softmax" if softmax else "sigmoid")
        seeds, gs = [l_main, l_jac], [one, one]
        if cfg.pointnet:
            seeds.append(L.batch_NN_loss(verts, torch.from_numpy(vert).to(dev)))
            gs.append(one)
        torch.autograd.backward(seeds, gs)
        return model, x, logits, verts
    fb0 = K.fallback_count()
    _, plain = _launch_tags(lambda: run(False))
    (model, x, logits, verts), hooked = _launch_tags(lambda: run(True))
    table = seg_table(model._last_S, cfg, logits, verts, dev, pools=True)

    p2 = {k: (v.requires_grad_(True) if ON.is_trainable(k) else v) for k, v in _ref_params(params, dev).items()}
    xo = torch.as_tensor(img, dtype=torch.float64, device=dev).requires_grad_(True)
    used, pre = set(), {}
    with ON.anchored(anchor_from(table, used, pre)):
        lo2, ve2 = ON.seg_forward(p2, xo, cfg, training=True)
    assert used == set(table), set(table) - used
    y2 = torch.as_tensor(mask, dtype=torch.float64, device=dev)
    m2, j2 = (OL.seg_loss_softmax if softmax else OL.seg_loss_sigmoid)(lo2, y2)
    loss2 = m2 + j2
    if cfg.pointnet:
        loss2 = loss2 + OL.batch_nn_loss(ve2, torch.as_tensor(vert, dtype=torch.float64, device=dev))
    loss2.backward()
    worst = compare_grads(model.named_parameters(), {k: v.grad for k, v in p2.items() if ON.is_trainable(k)})
    e_dx = rel_err(x.grad, xo.grad)
    assert e_dx < TOL, e_dx
    print("%s segmenter B=%d %dx%dx%d: worst parameter gradient error %s %.2e, dx %.2e; worst layer-local forward error "
          "%s %.2e" % (name, b, hw, hw, cin, worst[0], worst[1], e_dx, pre.get("tag"), pre.get("e", 0.0)))
    _check_dispatch(name + " segmenter", plain, hooked, fb0)


def _disc_case(dev, name, seed):
    """an image discriminator at the 2B batch the step's update runs it at (source + target), on its class-map input"""
    from oracle import losses as OL
    from oracle import nets as ON
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.networks import UncertaintyDiscriminator
    from pointcloududa_amd.utils import loss as L
    wl, nc, _, hw, _, _, _ = _setup(name)
    b2 = 2 * wl["batch"]
    params = ON.make_params(ON.disc_param_shapes(nc), seed, std=0.02)
    xn = np.random.default_rng(seed + 1).normal(0, 1, (b2, nc, hw, hw)).astype(np.float32)

    def run(keep):
        model = load(UncertaintyDiscriminator(in_channel=nc), params, dev)
        model._keep_acts = keep
        x = torch.from_numpy(xn).to(dev).requires_grad_(True)
        L.bce_logits_const(model(x), 1.0).backward()
        return model, x
    fb0 = K.fallback_count()
    _, plain = _launch_tags(lambda: run(False))
    (model, x), hooked = _launch_tags(lambda: run(True))
    table = disc_table(model, device=dev)
    p2 = {k: v.requires_grad_(True) for k, v in _ref_params(params, dev).items()}
    xo = torch.as_tensor(xn, dtype=torch.float64, device=dev).requires_grad_(True)
    used, pre = set(), {}
    with ON.anchored(anchor_from(table, used, pre)):
        d2 = ON.disc_forward(p2, xo)
    assert used == set(table)
    OL.bce_logits_const(d2, 1.0).backward()
    worst = compare_grads(model.named_parameters(), {k: v.grad for k, v in p2.items()})
    e_dx = rel_err(x.grad, xo.grad)
    assert e_dx < TOL, e_dx
    print("%s discriminator 2B=%d %dx%dx%d: worst parameter gradient error %s %.2e, dx %.2e; worst layer-local forward "
          "error %s %.2e" % (name, b2, hw, hw, nc, worst[0], worst[1], e_dx, pre.get("tag"), pre.get("e", 0.0)))
    _check_dispatch(name + " discriminator", plain, hooked, fb0)


# uda_512 first: its maps are the only ones that reach 512 px
@pytest.mark.parametrize("name,seed", [("uda_512", 2100), ("mscmrseg_224", 2110), ("unet_d2", 2120)])
def test_production_segmenter_gradients(dev, name, seed):
    _seg_case(dev, name, seed)


@pytest.mark.parametrize("name,seed", [("uda_512", 2200), ("mscmrseg_224", 2210), ("unet_d2", 2220)])
def test_production_discriminator_gradients(dev, name, seed):
    _disc_case(dev, name, seed)
