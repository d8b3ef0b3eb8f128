"""Shared-routing helpers of the backward checks (test_backward_exact_gpu.py, test_production_grads_gpu.py).

The CPU restatement in ``oracle`` is ANCHORED to the HIP forward pass: every conv / linear / normalisation output takes
the value the HIP kernels produced (``z + (z_hip - z).detach()``), so both sides take the same branch everywhere while
autograd still differentiates the restatement.  The anchor tables built here hold those HIP values; by default they are
copied to the host (the float32 CPU oracle), with ``device=`` they stay on the GPU for a float64 reference that runs
there.  Every comparison is made where the reference lives, in float64.
"""
import numpy as np
import torch

TOL = 1e-4
# whole-step segmenter gradients: worst-case linear accumulation of 2 x 2^-17 per convolution layer over the 29 + 5 layers
# between the adversarial loss and the first encoder block (derivation in test_train_step_backward_shared_routing)
SEG_CHAIN_TOL = 2 * (29 + 5) * 2.0 ** -17
PRE_TOL = 2e-4      # layer-local forward bound (_anchor_from)


def rel_err(a, b):
    """conftest.rel_err's definition -- max |a-b| / max(1e-30, max |b|), in float64 -- computed on ``b``'s device"""
    b = b.detach().double()
    a = a.detach().to(b.device).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / max(1e-30, float(b.abs().max()))


def load(mod, params, dev):
    mod.load_state_dict({k: v.clone() for k, v in params.items()}, strict=True)
    return mod.to(dev).train()


def unlrelu(a, slope, device="cpu"):
    """pre-activation with the sign (and, up to one rounding, the value) the HIP kernel saw: a float32 COPY on ``device``"""
    a = a.detach().float().to(device, copy=True)
    return a if slope == 1.0 else torch.where(a > 0, a, a / slope)


def anchor_from(table, used, worst=None):
    """With every upstream output anchored, the difference between the restatement's output of a layer and the HIP
    kernels' BEFORE it is anchored is that layer's own arithmetic error (bf16x3 products, fp32 accumulation order):
    held to 2e-4 of the tensor's scale; ``worst`` collects the largest one per network for the test's report."""
    def fn(tag, z):
        if tag not in table:
            return z
        used.add(tag)
        v = table[tag]
        if isinstance(v, tuple):          # (post-ReLU value, True): share the mask, keep own value where inactive
            y = v[0].detach().float().to(z.device).reshape(z.shape)
            tgt = torch.where(y > 0, y.to(z.dtype), torch.clamp(z.detach(), max=0.0))
        else:
            tgt = v.reshape(z.shape).to(z.device, z.dtype)
        e = rel_err(z, tgt)
        if worst is not None and e > worst.get("e", 0.0):
            worst["e"], worst["tag"] = e, tag
        assert e < PRE_TOL, (tag, e)      # the two forward passes agree, layer by layer, before anchoring
        return z + (tgt - z).detach()

    def pool(tag, x):
        """2x2 max-pool through the HIP kernel's argmax (window index 2 * dy + dx per output element), which must be
        a maximum of the restatement's own window up to the layer-local bound"""
        if tag not in table:
            return torch.nn.functional.max_pool2d(x, 2)
        used.add(tag)
        n, c, h, w = x.shape
        win = x.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
        y = torch.gather(win, 4, table[tag].to(x.device).long().reshape(n, c, h // 2, w // 2, 1)).squeeze(4)
        gap = float((win.detach().amax(4) - y.detach()).max()) / max(1e-30, float(x.detach().abs().max()))
        assert gap < PRE_TOL, (tag, gap)
        return y
    fn.pool = pool
    return fn


def compare_grads(named_hip, grads_ref, tol=TOL, parts=None):
    """``parts``: name -> one of two partial gradients whose sum ``grads_ref`` is (the discriminators' source and target
    passes, which largely cancel at initialisation): the error is then taken relative to the larger PART's scale"""
    worst = ("", 0.0)
    total = sum(float(g.double().norm()) ** 2 for g in grads_ref.values() if g is not None) ** 0.5
    for k, p in named_hip:
        g = grads_ref.get(k)
        if g is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        # (a bias in front of a BatchNorm has an exactly-zero true gradient: both sides hold rounding noise there)
        if float(g.double().norm()) < 1e-5 * total:
            assert float(p.grad.double().norm()) < 1e-4 * total, k
            continue
        e = rel_err(p.grad, g)
        diff = float((p.grad.detach().to(g.device).double() - g.double()).abs().max())
        if parts is not None:
            scale = max(float(parts[k].abs().max()), float((g - parts[k]).abs().max()), float(g.abs().max()))
            e = diff / max(scale, 1e-30)
        if e >= tol and diff <= 1e-6 * total:
            continue      # a near-zero gradient (just above the floor above): rounding noise on both sides
        if e > worst[1]:
            worst = (k, e)
        assert e < tol, (k, e)
    return worst


class Grad:
    """a gradient slice wrapped the way compare_grads reads a parameter (``.grad``)"""

    def __init__(self, g):
        self.grad = g


def flat_named(mod, snap):
    """(name, Grad) per parameter of ``mod`` over a snapshot of its optimiser's flat gradient buffer (64-element aligned
    slices, in named_parameters order)"""
    out, off = [], 0
    for k, p in mod.named_parameters():
        n = p.numel()
        out.append((k, Grad(snap[off:off + n].view(p.shape))))
        off += (n + 63) // 64 * 64
    return out


def random_running_stats(params, seed):
    rng = np.random.default_rng(seed + 7)
    for k in params:
        if ".in" in k or k.startswith("in"):
            continue
        if k.endswith("running_mean"):
            params[k] = torch.from_numpy(rng.normal(0, 0.2, tuple(params[k].shape)).astype(np.float32))
        if k.endswith("running_var"):
            params[k] = torch.from_numpy(rng.uniform(0.5, 1.5, tuple(params[k].shape)).astype(np.float32))


def seg_table(S, cfg, logits, verts, device="cpu", pools=False):
    """anchor table of one segmenter forward pass: pre-activation outputs of every convolution the HIP engine kept;
    ``pools``: also the max-pool routing (at production sizes the 2x2 windows hold near-ties that the two precisions
    break differently: one such window moved a 512 px input gradient by 1.4e-4 of its scale)"""
    table = {"classifier": logits.detach().float().to(device, copy=True)}
    for blk in ["encoder.encoder%d" % (i + 1) for i in range(cfg.n_block)] + \
               ["decoder.decoder2_%d" % (i + 1) for i in range(cfg.n_block)]:
        _, _, a0, _, a1, _ = S[blk]
        table[blk + ".0"] = unlrelu(a0, 0.01, device)
        table[blk + (".3" if cfg.batchnorm else ".2")] = unlrelu(a1, 0.01, device)
    for i in range(1, cfg.n_block):
        c1 = "encoder.conv1_%d.0" % (i + 1)
        table[c1] = unlrelu(S[c1][2], 0.01, device)
    for i in range(cfg.n_block if pools else 0):      # the argmax the HIP kernel took in each 2x2 window
        table["encoder.pool%d" % (i + 1)] = S["pool%d" % i].to(device, copy=True)
    for j, o in enumerate(S["bott_outs"]):
        table["bottleneck.bottleneck%d.0" % (j + 1)] = unlrelu(o, 0.01, device)
    if cfg.pointnet:
        table["pointNet.final_conv"] = unlrelu(S["head"][1], 0.01, device)
        for nm, _, o in S["head_ext"]:
            table[nm] = unlrelu(o, 0.01, device)
        table["pointNet.final_fc"] = verts.detach().float().to(device, copy=True)
    return table


def disc_table(model, acts=None, device="cpu"):
    """anchor table of one discriminator pass: ``acts`` = [input, output of each layer] (default: the module's last
    recorded pass, ``_keep_acts``)"""
    names = [n for n, _ in model._chain]
    acts = model._last_acts if acts is None else acts
    return {n: unlrelu(acts[i + 1], 0.2 if i < len(names) - 1 else 1.0, device) for i, n in enumerate(names)}


def pn_table(trace, device="cpu"):
    table = {}
    for k, v in trace.items():
        if isinstance(v, tuple) and v[1]:
            table[k] = (v[0].detach().float().to(device, copy=True), True)
        else:
            table[k] = (v[0] if isinstance(v, tuple) else v).detach().float().to(device, copy=True)
    return table
