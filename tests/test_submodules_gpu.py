"""The segmenter's and PointNet's sub-modules called on their own, on the HIP kernels.

1. Against the reference (tests/golden/submodules_small.npz, scripts/make_submodule_golden.py): outputs, running
   statistics, num_batches_tracked, the consumed skip list, batch size 1.
2. Gradients with the routing shared: the oracle's stage functions, anchored to the HIP forward pass, in float64.
3. Composition: encoder -> bottleneck -> pointNet / decoder -> classifier equals the fused network call.
4. No stale weights after a fused optimiser step.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from anchor_helpers import TOL, Grad, anchor_from, compare_grads, load, pn_table, rel_err, unlrelu
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


def _gen():
    spec = importlib.util.spec_from_file_location("make_submodule_golden",
                                                  os.path.join(ROOT, "scripts", "make_submodule_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MG = _gen()


def _gold():
    return np.load(os.path.join(GOLD, "submodules_small.npz"))


def _close(a, ref, tol, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    e = float(np.abs(a - ref).max()) / max(1e-30, float(np.abs(ref).max())) if ref.size else 0.0
    assert e < tol, (what, e)
    return e


def _seg_model(case, dev, mode):
    from pointcloududa_amd.networks import Segmentation_model_Point
    m = load(Segmentation_model_Point(**MG.SEG_CASES[case]), MG.seg_params(case), dev)
    return m.train(mode == "train")


def _project(outs, seed):
    rs = MG.projections([tuple(o.shape) for o in outs], seed)
    return sum((o * torch.from_numpy(r).to(o.device)).sum() for o, r in zip(outs, rs))


def _check_run(g, key, mod, outs, xs, worst):
    for i, o in enumerate(outs):
        worst.append(_close(MG.sample(o.detach().cpu().numpy()), g[key + "out%d" % i], 1e-3, key + "out%d" % i))
        assert list(o.shape) == [d for d in g[key + "shapes"][i] if d], (key, i, tuple(o.shape))
    # gradients against the unanchored reference: a sanity bound only -- one LeakyReLU sign or 2x2 pool argmax that the two
    # precisions break differently moves an element by percents (seen: 1.9e-2 on an encoder input gradient); the 1e-4
    # checks are the shared-routing tests below
    grads = MG.pack_grads([(k, None if p.grad is None else p.grad.cpu().numpy()) for k, p in mod.named_parameters()])
    _close(grads, g[key + "grads"], 0.1, key + "grads")
    for i, x in enumerate(xs):
        _close(MG.sample(x.grad.cpu().numpy()), g[key + "dx%d" % i], 0.1, key + "dx%d" % i)
    stats = [b.cpu().numpy().reshape(-1) for k, b in mod.named_buffers() if MG.is_stat(k)]
    if stats:
        _close(MG.sample(np.concatenate(stats), 4 * MG.NS), g[key + "stats"], 1e-4, key + "stats")
    tracked = [b.item() for k, b in mod.named_buffers() if MG.is_tracked(k)]
    assert tracked == list(g[key + "tracked"]), (key, tracked)


# ------------------------------------------------------------------------------------------------ 1. reference golden
@pytest.mark.parametrize("case", list(MG.SEG_CASES))
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_segmenter_submodules_match_reference(dev, case, mode):
    """each sub-module of a Segmentation_model_Point called on its own; only its own layers' statistics move"""
    g = _gold()
    ins = MG.seg_inputs(case)
    worst = []
    for name in MG.SEG_SUBS:
        model = _seg_model(case, dev, mode)
        mod = getattr(model, name)
        key = "%s__%s__%s__" % (case, mode, name)
        seed = MG.seg_seed(case) + 100 * MG.SEG_SUBS.index(name)
        if name == "decoder":
            xs = [torch.from_numpy(ins[k]).to(dev).requires_grad_(True) for k in ["decoder"] + ["skip%d" % i for i in range(4)]]
            skip = ["a", "b"] + xs[1:]
            outs = [mod(xs[0], skip)]
            assert len(skip) == int(g[key + "skip_len_after"]) and skip == ["a", "b"]
        else:
            xs = [torch.from_numpy(ins[name]).to(dev).requires_grad_(True)]
            res = mod(xs[0])
            outs = [res[0]] + list(res[1]) if name == "encoder" else [res]
            if name == "encoder":
                assert isinstance(res[1], list) and len(res[1]) == 4
        _project(outs, seed).backward()
        torch.cuda.synchronize()
        _check_run(g, key, mod, outs, xs, worst)
        for other, m in model.named_children():       # the other sub-modules' BatchNorm layers did not count a batch
            if other != name:
                assert all(b.item() == 0 for k, b in m.named_buffers() if k.endswith("num_batches_tracked")), other
    print("%s %s: worst output error %.2e" % (case, mode, max(worst)))


@pytest.mark.parametrize("case", list(MG.PN_CASES))
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_pointnet_submodules_match_reference(dev, case, mode):
    from pointcloududa_amd import networks as N
    g = _gold()
    cls, kw = MG.PN_CASES[case]
    mod = load(getattr(N, cls)(**kw), MG.pn_params(case), dev).train(mode == "train")
    x = torch.from_numpy(MG.pn_inputs(case)).to(dev).requires_grad_(True)
    res = mod(x)
    outs = [o for o in (res if isinstance(res, tuple) else (res,)) if o is not None]
    if case.endswith("local"):
        assert outs[0].shape == (MG.PN_B, 1088, MG.PN_N)
    _project(outs, MG.pn_seed(case)).backward()
    torch.cuda.synchronize()
    worst = []
    _check_run(g, "%s__%s__" % (case, mode), mod, outs, [x], worst)
    print("%s %s: worst output error %.2e" % (case, mode, max(worst)))


@pytest.mark.parametrize("case", list(MG.BATCH1))
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_batch_size_one_as_reference(dev, case, mode):
    from pointcloududa_amd import networks as N
    g = _gold()
    cls, kw = MG.BATCH1[case]
    mod = load(getattr(N, cls)(**kw), MG.pn_params(case), dev).train(mode == "train")
    x = torch.from_numpy(MG.pn_inputs(case, b=1)).to(dev)
    key = "b1__%s__%s__" % (case, mode)
    if int(g[key + "raises"]):
        with pytest.raises(RuntimeError):
            mod(x)
        if cls == "STN3d" or (cls == "PointNetfeat" and kw.get("sample_transform", True)):
            with pytest.raises(RuntimeError, match="InstanceNorm1d branch"):
                mod(x)
        return
    with torch.no_grad():
        y = mod(x)
    y = y[0] if isinstance(y, tuple) else y
    _close(MG.sample(y.cpu().numpy()), g[key + "out"], 1e-3, key)


# ------------------------------------------------------------------------------------------------ 2. shared routing
def _stage_table(S, eng, name, out=None, device="cpu"):
    """anchor table of one standalone stage pass (the layers of anchor_helpers.seg_table that the stage ran)"""
    t = {}
    blocks = {"encoder": ["encoder.encoder%d" % (i + 1) for i in range(eng.nb)],
              "decoder": ["decoder.decoder2_%d" % (i + 1) for i in range(eng.nb)]}.get(name, [])
    for blk in blocks:
        _, _, a0, _, a1, _ = S[blk]
        t[blk + ".0"] = unlrelu(a0, 0.01, device)
        t[blk + eng.c2] = unlrelu(a1, 0.01, device)
    if name == "encoder":
        for i in range(1, eng.nb):
            c1 = "encoder.conv1_%d.0" % (i + 1)
            t[c1] = unlrelu(S[c1][2], 0.01, device)
        for i in range(eng.nb):
            t["encoder.pool%d" % (i + 1)] = S["pool%d" % i].to(device, copy=True)
    if name == "bottleneck":
        for j, o in enumerate(S["bott_outs"]):
            t["bottleneck.bottleneck%d.0" % (j + 1)] = unlrelu(o, 0.01, device)
    if name == "pointNet":
        t["pointNet.final_conv"] = unlrelu(S["head"][1], 0.01, device)
        for nm, _, o in S["head_ext"]:
            t[nm] = unlrelu(o, 0.01, device)
        t["pointNet.final_fc"] = out.detach().to(device, copy=True)
    return t


@pytest.mark.parametrize("case", ["seg", "seg_extpn", "seg_nobn"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_segmenter_submodule_gradients_shared_routing(dev, case, mode):
    """parameter and input gradients (each skip's included) of every stage against oracle.nets' stage functions"""
    from oracle import nets as ON
    cfg = MG.seg_cfg(case)
    params = MG.seg_params(case)
    ins = MG.seg_inputs(case)
    training = mode == "train"
    for name in MG.SEG_SUBS:
        model = _seg_model(case, dev, mode)
        mod = getattr(model, name)
        mod._keep_state = True
        seed = MG.seg_seed(case) + 100 * MG.SEG_SUBS.index(name)
        keys = ["decoder"] + ["skip%d" % i for i in range(4)] if name == "decoder" else [name]
        xs = [torch.from_numpy(ins[k]).to(dev).requires_grad_(True) for k in keys]
        if name == "encoder":
            o, sk = mod(xs[0])
            outs = [o] + sk
        elif name == "decoder":
            outs = [mod(xs[0], list(xs[1:]))]
        else:
            outs = [mod(xs[0])]
        _project(outs, seed).backward()
        eng = model._engine
        table = _stage_table(mod._last_S, eng, name, outs[0], device=dev)

        p2 = ON.params_to(params, torch.float64, dev)
        for k in p2:
            if ON.is_trainable(k) and k.startswith(name + "."):
                p2[k].requires_grad_(True)
        x2 = [torch.from_numpy(ins[k]).to(dev, torch.float64).requires_grad_(True) for k in keys]
        used = set()
        with ON.anchored(anchor_from(table, used)):
            if name == "encoder":
                o2, sk2 = ON._encoder(p2, x2[0], cfg, training)
                outs2 = [o2] + sk2
            elif name == "bottleneck":
                outs2 = [ON._bottleneck(p2, x2[0], cfg)]
            elif name == "pointNet":
                outs2 = [ON._point_head(p2, x2[0], cfg)]
            else:
                outs2 = [ON._decoder(p2, x2[0], list(x2[1:]), cfg, training)]
        assert used == set(table), set(table) - used
        for a, b in zip(outs, outs2):
            assert rel_err(a, b) < 1e-4, name
        _project(outs2, seed).backward()
        ref = {k[len(name) + 1:]: v.grad for k, v in p2.items() if k.startswith(name + ".") and ON.is_trainable(k)}
        ref = {k: v for k, v in ref.items() if v is not None}
        worst = compare_grads(mod.named_parameters(), ref)
        for x, xo in zip(xs, x2):
            assert rel_err(x.grad, xo.grad) < TOL, name
        print("%s %s %s: worst parameter gradient %s %.2e" % (case, mode, name, worst[0], worst[1]))


def _feat_ref(p, x, kw, training):
    """PointNetfeat.forward (PointNetCls.py:135-168) restated from oracle.nets' _stn / _norm1d / _anc"""
    import torch.nn.functional as F
    from oracle import nets as ON
    ext, ft = kw.get("ext", False), kw.get("feature_transform", False)
    trans = trans_feat = None
    if kw.get("sample_transform", True):
        trans = ON._stn(p, "stn.", x, 3, training, has_in=True)
        x = torch.bmm(x.transpose(2, 1), trans).transpose(2, 1)

    def cbr(conv, bn, h, relu=True):
        h = ON._anc(conv, F.conv1d(h, p[conv + ".weight"], p[conv + ".bias"]))
        h = ON._norm1d(p, bn, None, h, training, True)
        return F.relu(h) if relu else h
    h = cbr("conv1", "bn1", x)
    if ext:
        h = cbr("conv1_1", "bn1_1", h)
    if ft:
        trans_feat = ON._stn(p, "fstn.", h, 64, training, has_in=False)
        h = torch.bmm(h.transpose(2, 1), trans_feat).transpose(2, 1)
    pointfeat = h
    h = cbr("conv2", "bn2", h)
    if ext:
        h = cbr("conv2_1", "bn2_1", h)
    h = cbr("conv3", "bn3", h, relu=False)
    if ext:
        h = cbr("conv3_1", "bn3_1", h)
    g = h.max(dim=2)[0]
    if not kw.get("global_feat", True):
        g = torch.cat([g.view(-1, 1024, 1).repeat(1, 1, x.shape[2]), pointfeat], 1)
    return [o for o in (g, trans, trans_feat) if o is not None]


@pytest.mark.parametrize("case", ["stn3d", "stnkd", "feat_local", "feat_ft_ext", "feat_ft_local"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_pointnet_submodule_gradients_shared_routing(dev, case, mode):
    from oracle import nets as ON
    from pointcloududa_amd import networks as N
    cls, kw = MG.PN_CASES[case]
    training = mode == "train"
    params = MG.pn_params(case)
    mod = load(getattr(N, cls)(**kw), params, dev).train(training)
    mod._keep_trace = True
    # (centred points: with inputs in [0, 1) the first layer's weight gradient behind a training-mode BatchNorm is a sum
    # that cancels to ~1e-3 of its terms, and float32 accumulation alone leaves 3e-4 against the float64 reference)
    xn = 2.0 * MG.pn_inputs(case) - 1.0
    x = torch.from_numpy(xn).to(dev).requires_grad_(True)
    res = mod(x)
    outs = [o for o in (res if isinstance(res, tuple) else (res,)) if o is not None]
    _project(outs, MG.pn_seed(case)).backward()
    table = pn_table(mod._last_trace, device=dev)
    p2 = ON.params_to(params, torch.float64, dev)
    for k in p2:
        if ON.is_trainable(k):
            p2[k].requires_grad_(True)
    x2 = torch.from_numpy(xn).to(dev, torch.float64).requires_grad_(True)
    used = set()
    with ON.anchored(anchor_from(table, used)):
        if cls == "PointNetfeat":
            outs2 = _feat_ref(p2, x2, kw, training)
        else:
            outs2 = [ON._stn(p2, "", x2, 3 if cls == "STN3d" else 64, training, has_in=cls == "STN3d")]
    assert used == set(table), set(table) - used
    for a, b in zip(outs, outs2):
        assert rel_err(a, b) < 1e-4, case
    _project(outs2, MG.pn_seed(case)).backward()
    worst = compare_grads(mod.named_parameters(), {k: v.grad for k, v in p2.items() if ON.is_trainable(k)})
    assert rel_err(x.grad, x2.grad) < TOL
    print("%s %s: worst parameter gradient %s %.2e" % (case, mode, worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------ 3. composition
class _Classifier(torch.autograd.Function):
    """the network's 1x1 classifier on its own ConvOp (a holder layer cannot be called): the composition's last step"""

    @staticmethod
    def forward(ctx, model, x, w, b):
        op = model._engine.ops["classifier"]
        h, wd = x.shape[2], x.shape[3]
        y, _, _ = op.forward(x.contiguous(), w, b, 1.0, h, wd)
        ctx.save_for_backward(x)
        ctx.model, ctx.hw = model, (h, wd)
        return y

    @staticmethod
    def backward(ctx, dy):
        from pointcloududa_amd.networks._holders import ensure_grad
        (x,) = ctx.saved_tensors
        op = ctx.model._engine.ops["classifier"]
        w, b = ctx.model.classifier.weight, ctx.model.classifier.bias
        dy = dy.contiguous()
        op.wgrad(x, dy, ensure_grad(w), ensure_grad(b), *ctx.hw)
        return None, op.dgrad(dy, w, *ctx.hw), None, None


def _record_dispatch(monkeypatch, K):
    """(method, K.last_kernel()) after every convolution launch of the engine: the kernel and plan each layer ran on"""
    log = []
    for meth in ("forward", "dgrad", "dgrad_fold"):
        inner = getattr(K.ConvOp, meth)

        def wrapped(self, *a, _inner=inner, _meth=meth, **k):
            out = _inner(self, *a, **k)
            log.append((_meth, K.last_kernel()))
            return out
        monkeypatch.setattr(K.ConvOp, meth, wrapped)
    return log


@pytest.mark.parametrize("kw,b,hw,seed", [
    (dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9), 2, 128, 3500),
    (dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9, extpn=True, batchnorm=False), 2, 128, 3510),
    (dict(filters=32, in_channels=3, n_class=4, pointnet=True, fc_inch=121), 8, 256, 3520),
])
def test_composition_equals_fused_network(dev, monkeypatch, kw, b, hw, seed):
    """encoder -> bottleneck -> pointNet / decoder -> classifier on the same weights and input as model(x): logits and
    vertices within 1e-5, parameter gradients within 1e-4 under the reference's supervised loss.  Every forward
    convolution runs on the kernel and plan the network's call picks (the affine-on-load flag aside: the standalone
    decoder and classifier read materialised BatchNorm outputs); at filters=32, 256x256 those include the anti-phase and
    the row-streaming kernels."""
    monkeypatch.setenv("PCUDA_AP_MIN_ITEMS", "0")
    monkeypatch.setenv("PCUDA_RS_MIN_ITEMS", "0")
    import re
    from oracle import nets as ON
    from oracle.synth import synth_batch
    from pointcloududa_amd import kernels as K
    from pointcloududa_amd.networks import Segmentation_model_Point
    from pointcloududa_amd.utils import loss as L
    params = ON.make_params(ON.seg_param_shapes(ON.SegCfg(**kw)), seed)
    img, mask, vert, _, _ = synth_batch(b, kw["in_channels"], kw["n_class"], hw, seed=seed + 1)
    runs = []
    fb = K.fallback_count()
    log = _record_dispatch(monkeypatch, K)
    for standalone in (False, True):
        model = load(Segmentation_model_Point(**kw), params, dev)
        x = torch.from_numpy(img).to(dev).requires_grad_(True)
        del log[:]
        if standalone:
            out, skip = model.encoder(x)
            bott = model.bottleneck(out)
            verts = model.pointNet(bott)
            dec = model.decoder(bott, skip)
            assert skip == []
            logits = _Classifier.apply(model, dec, model.classifier.weight, model.classifier.bias)
        else:
            logits, _, verts = model(x)
        fwd = [k for m, k in log if m == "forward"]
        l_main, l_jac = L.seg_loss(logits, torch.from_numpy(mask).to(dev), "sigmoid")
        l_pt = L.batch_NN_loss(verts, torch.from_numpy(vert).to(dev))
        torch.autograd.backward([l_main, l_jac, l_pt])
        torch.cuda.synchronize()
        bwd = [k for m, k in log if m != "forward"]
        stats = {k: v.detach().clone() for k, v in model.named_buffers()}
        runs.append((logits.detach(), verts.detach(), {k: p.grad.clone() for k, p in model.named_parameters()
                                                       if p.grad is not None}, x.grad.clone(), stats, fwd, bwd))
    (lo, ve, gr, dx, st, fwd, _), (lo2, ve2, gr2, dx2, st2, fwd2, bwd2) = runs
    plan = lambda ks: [re.sub(r" aff\d", "", k) for k in ks]
    assert plan(fwd2) == plan(fwd), [(a, c) for a, c in zip(fwd2, fwd) if plan([a]) != plan([c])]
    e_lo, e_ve = rel_err(lo2, lo), rel_err(ve2, ve)
    print("standalone vs fused: logits %.2e, vertices %.2e" % (e_lo, e_ve))
    assert e_lo < 1e-5 and e_ve < 1e-5
    assert set(gr) == set(gr2)
    worst = compare_grads([(k, Grad(g)) for k, g in gr2.items()], gr)
    assert rel_err(dx2, dx) < TOL
    for k, v in st.items():
        assert (torch.equal(v, st2[k]) if not v.is_floating_point() else rel_err(st2[k], v) < 1e-5), k
    assert K.fallback_count() == fb
    fams = lambda ks: sorted({k.split("|")[-1].strip() for k in ks})
    print("standalone forward kernels %s, backward %s; worst gradient %.2e %s" % (fams(fwd2), fams(bwd2), worst[1], worst[0]))
    if kw["filters"] == 32:
        assert any("conv3ap" in k for k in fwd2), fams(fwd2)
        assert any("conv3rs" in k for k in fwd2), fams(fwd2)


# ------------------------------------------------------------------------------------------------ 4. stale weights
def test_standalone_encoder_after_fused_optimiser_step(dev):
    from oracle import nets as ON
    from pointcloududa_amd.networks import Segmentation_model_Point
    from pointcloududa_amd.optim import FusedAdam, flatten_module
    kw = dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9)
    params = ON.make_params(ON.seg_param_shapes(ON.SegCfg(**kw)), 3600)
    model = load(Segmentation_model_Point(**kw), params, dev)
    flatten_module(model)
    opt = FusedAdam(model, lr=1e-2)
    x = torch.from_numpy(np.random.default_rng(3601).normal(0, 1, (2, 1, 128, 128)).astype(np.float32)).to(dev)
    model.encoder(x)                        # packs the encoder's weights
    logits, _, verts = model(x)
    (logits.square().mean() + verts.square().mean()).backward()
    opt.step()
    model.eval()
    out, skip = model.encoder(x)
    fresh = Segmentation_model_Point(**kw).to(dev)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    out2, skip2 = fresh.encoder(x)
    assert torch.equal(out, out2)
    for a, c in zip(skip, skip2):
        assert torch.equal(a, c)
    assert model.encoder.encoder1[2].num_batches_tracked.item() == 2


def test_decoder_refuses_a_wrong_skip_without_consuming_the_list(dev):
    from pointcloududa_amd.networks import Decoder
    dec = Decoder(filters=4).to(dev)
    skip = [torch.zeros(2, 4 * 2 ** i, 32 >> i, 32 >> i, device=dev) for i in range(4)]
    skip[1] = torch.zeros(2, 8, 15, 15, device=dev)
    with pytest.raises(ValueError, match="skip"):
        dec(torch.zeros(2, 64, 2, 2, device=dev), skip)
    assert len(skip) == 4
