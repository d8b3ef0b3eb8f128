"""Writes tests/golden/submodules_small.npz: the reference's segmenter and PointNet sub-modules run on their own.

    python scripts/make_submodule_golden.py            # (re)writes the fixture (needs the reference's src/ on the path)
    python scripts/make_submodule_golden.py --check    # regenerates it in memory and compares every array

Each sub-module of unet.py (Encoder, Bottleneck, PointNet, Decoder) and of PointNetCls.py (STN3d, STNkd, PointNetfeat)
is loaded with ``oracle.nets.make_params`` weights (the network prefix stripped) and called once in train mode and once
in eval mode (the random running statistics of make_params) on seeded inputs.  Stored per case and mode: strided samples
of every output (each skip tensor included), the length of the skip list after Decoder, a sample of the running
statistics afterwards, and samples of the parameter and input gradients of a seeded projection loss sum_k <out_k, R_k>.  Also
stored: which batch-size-1 calls raise in the reference, and the ``state_dict`` keys and shapes of every sub-module.
Inputs and projections are NOT stored: the numpy half of this file regenerates them from their seeds (the GPU tests
import it; the reference is imported only by ``generate``)."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "submodules_small.npz")
REF_SRC = os.environ.get("PCUDA_REFERENCE_SRC", "/root/reference/src")
NS, NG = 256, 32      # elements kept of each output and input gradient / of each parameter gradient (strided samples)

# segmenter cases: filters=4, 128x128, 1 input channel -> bottleneck maps of 8x8, point head fc_inch = 3 x 3
SEG_CASES = {
    "seg": dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9),
    "seg_extpn": dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9, extpn=True),
    "seg_nobn": dict(filters=4, in_channels=1, n_class=4, pointnet=True, fc_inch=9, batchnorm=False),
}
SEG_B, SEG_HW = 2, 128
# PointNet cases: (module, constructor arguments), B=4 point clouds of 64 points
PN_CASES = {
    "stn3d": ("STN3d", {}),
    "stnkd": ("STNkd", dict(k=64)),
    "feat": ("PointNetfeat", {}),
    "feat_local": ("PointNetfeat", dict(global_feat=False)),
    "feat_ft_ext": ("PointNetfeat", dict(feature_transform=True, ext=True)),
    "feat_ft_local": ("PointNetfeat", dict(feature_transform=True, global_feat=False)),
    "feat_nost": ("PointNetfeat", dict(sample_transform=False)),
}
PN_B, PN_N = 4, 64
# batch size 1: (module, constructor arguments) -- raises or computes, per mode, as the reference does
BATCH1 = {
    "stn3d": ("STN3d", {}),
    "stnkd": ("STNkd", dict(k=64)),
    "feat_nost": ("PointNetfeat", dict(sample_transform=False)),
    "feat_ft_nost": ("PointNetfeat", dict(feature_transform=True, sample_transform=False)),
    "feat": ("PointNetfeat", {}),
}


# ------------------------------------------------------------------------------------------------ numpy only
def sample(a, n=NS):
    """deterministic strided sample of an array (the same one oracle/make_golden.py takes)"""
    f = np.asarray(a).reshape(-1)
    step = max(1, f.size // n)
    return f[::step][:n].copy()


def seg_cfg(case):
    from oracle import nets as ON
    return ON.SegCfg(**SEG_CASES[case])


def seg_seed(case):
    return 3000 + 10 * list(SEG_CASES).index(case)


def seg_inputs(case):
    """name -> input array of each segmenter sub-module (the decoder's skips as skip0..skip{n_block-1}, outermost first)"""
    kw = SEG_CASES[case]
    f, nb, cin = kw["filters"], 4, kw["in_channels"]
    rng = np.random.default_rng(seg_seed(case) + 1)
    h = SEG_HW >> nb
    x = {"encoder": rng.normal(0, 1, (SEG_B, cin, SEG_HW, SEG_HW)),
         "bottleneck": np.abs(rng.normal(0, 1, (SEG_B, f * 2 ** (nb - 1), h, h))),
         "pointNet": np.abs(rng.normal(0, 1, (SEG_B, 512 * f // 32, h, h))),
         "decoder": rng.normal(0, 1, (SEG_B, f * 2 ** nb, h, h))}
    for i in range(nb):
        x["skip%d" % i] = rng.normal(0, 1, (SEG_B, f * 2 ** i, SEG_HW >> i, SEG_HW >> i))
    return {k: v.astype(np.float32) for k, v in x.items()}


def pn_seed(case):
    return 3100 + 10 * list(PN_CASES).index(case)


def pn_inputs(case, b=PN_B):
    cls, kw = PN_CASES.get(case) or BATCH1[case]
    cin = kw.get("k", 64) if cls == "STNkd" else 3
    rng = np.random.default_rng(pn_seed(case) if case in PN_CASES else 3300)
    return rng.random((b, cin, PN_N), dtype=np.float32)


def pack_grads(named):
    """(name, gradient array or None) pairs -> one array: NG elements sampled from each (none where there is no
    gradient: Encoder.conv1_1 never runs)"""
    parts = [sample(g, NG) for _, g in named if g is not None]
    return np.concatenate(parts).astype(np.float32) if parts else np.zeros(0, np.float32)


def is_stat(k):
    return (k.endswith("running_mean") or k.endswith("running_var")) and not (".in" in k or k.startswith("in"))


def is_tracked(k):
    return k.endswith("num_batches_tracked") and not (".in" in k or k.startswith("in"))


def projections(shapes, seed):
    """R_k of the projection loss sum_k <out_k, R_k>"""
    rng = np.random.default_rng(seed + 5)
    return [rng.normal(0, 1, s).astype(np.float32) for s in shapes]


def seg_params(case):
    """Segmentation_model_Point parameters of the case (oracle.nets.make_params: random running statistics too)"""
    from oracle import nets as ON
    return ON.make_params(ON.seg_param_shapes(seg_cfg(case)), seg_seed(case))


def pn_params(case):
    """the PointNetCls parameters the case's module takes, with the prefix stripped"""
    from oracle import nets as ON
    cls, kw = PN_CASES.get(case) or BATCH1[case]
    ft, ext = kw.get("feature_transform", cls == "STNkd"), kw.get("ext", False)
    full = ON.make_params(ON.pointnet_cls_param_shapes(ft, ext=ext), pn_seed(case) if case in PN_CASES else 3301)
    pre = {"STN3d": "feat.stn.", "STNkd": "feat.fstn.", "PointNetfeat": "feat."}[cls]
    out = {k[len(pre):]: v for k, v in full.items() if k.startswith(pre)}
    if cls == "PointNetfeat":
        out = {k: v for k, v in out.items() if not k.startswith("fstn.") or ft}
    return out


def sub_params(params, name):
    pre = name + "."
    return {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}


SEG_SUBS = ("encoder", "bottleneck", "pointNet", "decoder")


# ------------------------------------------------------------------------------------------------ reference
def _ref():
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import networks.PointNetCls as RP
    import networks.unet as RU
    return RU, RP


def seg_modules(RU, case):
    kw = SEG_CASES[case]
    f, bn = kw["filters"], kw.get("batchnorm", True)
    return {"encoder": RU.Encoder(filters=f, in_channels=kw["in_channels"], n_block=4, batch_norm=bn),
            "bottleneck": RU.Bottleneck(filters=f, n_block=4, depth=4),
            "pointNet": RU.PointNet(num_points=300, fc_inch=kw["fc_inch"], conv_inch=512 * f // 32,
                                    ext=kw.get("extpn", False)),
            "decoder": RU.Decoder(filters=f, n_block=4, batch_norm=bn)}


def _run(mod, inputs, call, seed, out):
    """one call + the projection loss's backward; stores outputs, gradients and running statistics under ``out``"""
    import torch
    xs = [torch.from_numpy(v).requires_grad_(True) for v in inputs]
    for p in mod.parameters():
        p.grad = None
    res = call(mod, xs)
    outs = [r for r in res if r is not None]
    loss = sum((o * torch.from_numpy(r)).sum() for o, r in zip(outs, projections([tuple(o.shape) for o in outs], seed)))
    loss.backward()
    arrays = {}
    for i, o in enumerate(outs):
        arrays["out%d" % i] = sample(o.detach().numpy())
    for i, x in enumerate(xs):
        arrays["dx%d" % i] = sample(x.grad.numpy())
    arrays["grads"] = pack_grads([(k, None if p.grad is None else p.grad.numpy()) for k, p in mod.named_parameters()])
    stats = [b.detach().numpy().reshape(-1) for k, b in mod.named_buffers() if is_stat(k)]
    arrays["stats"] = sample(np.concatenate(stats), 4 * NS) if stats else np.zeros(0, np.float32)
    arrays["tracked"] = np.array([b.item() for k, b in mod.named_buffers() if is_tracked(k)], dtype=np.int64)
    out.update(arrays)
    return res


def generate():
    import torch
    RU, RP = _ref()
    torch.set_num_threads(8)
    out = {}
    for case in SEG_CASES:
        params = seg_params(case)
        ins = seg_inputs(case)
        for mode in ("train", "eval"):
            mods = seg_modules(RU, case)
            for name, m in mods.items():
                m.load_state_dict({k: v.clone() for k, v in sub_params(params, name).items()}, strict=True)
                m.train(mode == "train")
            for name, m in mods.items():
                key = "%s__%s__%s__" % (case, mode, name)
                arr = {}
                seed = seg_seed(case) + 100 * SEG_SUBS.index(name)
                if name == "encoder":
                    res = _run(m, [ins["encoder"]], lambda mod, xs: (lambda o: [o[0]] + list(o[1]))(mod(xs[0])), seed, arr)
                elif name == "decoder":
                    n0 = 2

                    def call(mod, xs):
                        skip = [torch.zeros(1)] * n0 + list(xs[1:])      # two extra entries in front stay in the list
                        y = mod(xs[0], skip)
                        arr["skip_len_after"] = np.int64(len(skip))
                        return [y]
                    res = _run(m, [ins["decoder"]] + [ins["skip%d" % i] for i in range(4)], call, seed, arr)
                else:
                    res = _run(m, [ins[name]], lambda mod, xs: [mod(xs[0])], seed, arr)
                arr["shapes"] = np.array([list(r.shape) + [0] * (4 - r.dim()) for r in res], dtype=np.int64)
                out.update({key + k: v for k, v in arr.items()})
    for case, (cls, kw) in PN_CASES.items():
        params = pn_params(case)
        for mode in ("train", "eval"):
            m = getattr(RP, cls)(**kw)
            m.load_state_dict({k: v.clone() for k, v in params.items()}, strict=True)
            m.train(mode == "train")
            arr = {}
            res = _run(m, [pn_inputs(case)], lambda mod, xs: (lambda o: list(o) if isinstance(o, tuple) else [o])(mod(xs[0])),
                       pn_seed(case), arr)
            arr["shapes"] = np.array([list(r.shape) + [0] * (4 - r.dim()) for r in res if r is not None], dtype=np.int64)
            out.update({"%s__%s__%s" % (case, mode, k): v for k, v in arr.items()})
    for case, (cls, kw) in BATCH1.items():
        params = pn_params(case)
        for mode in ("train", "eval"):
            m = getattr(RP, cls)(**kw)
            m.load_state_dict({k: v.clone() for k, v in params.items()}, strict=True)
            m.train(mode == "train")
            try:
                with torch.no_grad():
                    y = m(torch.from_numpy(pn_inputs(case, b=1)))
                out["b1__%s__%s__raises" % (case, mode)] = np.int64(0)
                y = y[0] if isinstance(y, tuple) else y
                out["b1__%s__%s__out" % (case, mode)] = sample(y.numpy())
            except (RuntimeError, ValueError):
                out["b1__%s__%s__raises" % (case, mode)] = np.int64(1)
    mods = dict(seg_modules(RU, "seg"), **{"seg_nobn_" + k: v for k, v in seg_modules(RU, "seg_nobn").items()})
    mods["pointNet_ext"] = seg_modules(RU, "seg_extpn")["pointNet"]
    for case, (cls, kw) in PN_CASES.items():
        mods[case] = getattr(RP, cls)(**kw)
    for name, m in mods.items():
        sd = m.state_dict()
        out["keys__" + name] = np.array(list(sd.keys()))
        out["kshapes__" + name] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        with np.load(OUT) as g:
            have = set(g.files)
            bad = sorted(k for k in out if k not in have or not np.array_equal(g[k], out[k]))
            extra = sorted(have - set(out))
        if bad or extra:
            print("differs:", bad[:20], "extra:", extra[:20])
            sys.exit(1)
        print("ok: %d arrays equal" % len(out))
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
