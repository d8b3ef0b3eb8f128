"""HIP-backed losses with the reference's function names (``src/utils/loss.py``) plus the fused
forms the train step uses.

* ``jaccard_loss(true, logits, eps, activation)`` / ``batch_NN_loss(x, y)``: the reference
  signatures (loss.py:5-37, 40-76), backed by the fused kernels.
* ``seg_loss(logits, onehot_u8, mode)``: BCE + Jaccard (train_mscmrseg.py:202-203) or the
  "double softmax" cross-entropy + Jaccard (train_mmwhs.py:212-218) in one pass each way.
  ``overlap="dice"`` / ``"dice_sample"`` puts a Dice term in the Jaccard term's place (the scripts' ``-dice``).
* ``dice_loss(true, logits, eps, activation, reduce)`` / ``DiceLoss(eps)``: Dice with ``jaccard_loss``'s signature, and an
  ``nn.Module`` with the surface of the ``kornia.losses.DiceLoss()`` both scripts build and never call.  The rule is this
  build's own (include/pcuda_hip.h): parity with any kornia version is unpinned, kornia's ``+ eps`` on its one-hot tensor is
  not reproduced.
* ``entropy_map(logits, mode, normalise)``: -p log(p + 1e-7) [/ log C] (train_mscmrseg.py:222;
  train_mmwhs.py:224,242), optionally also returning p.
* ``bce_logits_const(d_out, label, weight)``: weight * BCE-with-logits against a constant map
  (train_mscmrseg.py:224-226), with the discriminator accuracy as a by-product.
"""
from __future__ import annotations

import math

import torch

from .. import kernels as K


def _zero(dev):
    return torch.zeros((), dtype=torch.float32, device=dev)


class _SegLossFn(torch.autograd.Function):
    """main term + overlap term in one pass each way: ``overlap`` "jaccard" on the seg_loss kernels (``eps`` is theirs), a Dice
    term on the seg_loss_ov kernels"""

    @staticmethod
    def forward(ctx, logits, onehot, mode, overlap, eps):
        logits = logits.contiguous()
        if overlap == "jaccard":
            out2, ws = K.seg_loss_fwd(logits, onehot, mode)
        else:
            out2, ws = K.seg_loss_ov_fwd(logits, onehot, mode, overlap, eps)
        ctx.logits, ctx.onehot, ctx.mode, ctx.overlap, ctx.ws = logits, onehot, mode, overlap, ws
        ctx.set_materialize_grads(False)
        return out2[0], out2[1]

    @staticmethod
    def backward(ctx, g_main, g_ov):
        dev = ctx.logits.device
        g_main = _zero(dev) if g_main is None else g_main.contiguous()
        g_ov = _zero(dev) if g_ov is None else g_ov.contiguous()
        if ctx.overlap == "jaccard":
            d = K.seg_loss_bwd(ctx.logits, ctx.onehot, ctx.mode, ctx.ws, g_main, g_ov)
        else:
            d = K.seg_loss_ov_bwd(ctx.logits, ctx.onehot, ctx.mode, ctx.overlap, ctx.ws, g_main, g_ov)
        return d, None, None, None, None


# eps of the fused overlap terms: Jaccard's is inside its kernels; per class Dice takes the same value, per sample
# kornia.losses.DiceLoss's default
_OVERLAP_EPS = {"jaccard": 1e-7, "dice": 1e-7, "dice_sample": 1e-6}


def overlap_for(dice):
    """the ``dice`` setting of the train step and the validation functions ("" | "class" | "sample") -> ``seg_loss``'s overlap"""
    names = {"": "jaccard", "class": "dice", "sample": "dice_sample"}
    if dice not in names:
        raise ValueError("dice %r is none of '', 'class', 'sample'" % (dice,))
    return names[dice]


def seg_loss(logits, onehot_u8, mode="sigmoid", overlap="jaccard"):
    """-> (bce_or_ce, overlap term) scalars.  onehot_u8: uint8 one-hot [B,C,H,W] (utils.py:25-29 layout).  ``overlap``:
    "jaccard" (what the reference trains with), "dice" (per class, the Jaccard term's twin: 1 - mean_c 2 I_c / (S_c + 1e-7))
    or "dice_sample" (per sample, kornia's documented formula: mean_n (1 - 2 I_n / (S_n + 1e-6))); the Dice rules are this
    build's own."""
    if overlap not in _OVERLAP_EPS:
        raise ValueError("seg_loss: overlap %r is none of 'jaccard', 'dice', 'dice_sample'" % (overlap,))
    return _SegLossFn.apply(logits, onehot_u8, mode, overlap, _OVERLAP_EPS[overlap])


class _OverlapFn(torch.autograd.Function):
    """Jaccard (``reduce`` None) or Dice ("class" | "sample") on given probabilities"""

    @staticmethod
    def forward(ctx, probs, true, eps, reduce):
        loss, ws, truth = K.jaccard_fwd(probs, true, eps) if reduce is None else K.dice_fwd(probs, true, eps, reduce)
        ctx.truth, ctx.ws, ctx.eps, ctx.reduce, ctx.shape = truth, ws, eps, reduce, tuple(probs.shape)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, gout):
        if gout is None:
            return None, None, None, None
        gout = gout.contiguous()
        if ctx.reduce is None:
            return K.jaccard_bwd(ctx.truth, ctx.shape, ctx.eps, ctx.ws, gout), None, None, None
        return K.dice_bwd(ctx.truth, ctx.shape, ctx.reduce, ctx.ws, gout), None, None, None


def _overlap_loss(true, logits, eps, activation, reduce):
    """the branches ``jaccard_loss`` and ``dice_loss`` share (loss.py:5-37).  The reference's C == 1 branch pairs
    [sigmoid, 1 - sigmoid] with ``true`` BROADCAST over both channels (the one-hot it builds at loss.py:15-19 is overwritten
    at :27): reproduced as executed."""
    if logits.shape[1] == 1:
        pos = entropy_map(logits, "sigmoid", False, want_prob=True)[1]
        probas = torch.cat([pos, 1 - pos], dim=1)                                     # loss.py:20-22
        true = true.float().expand_as(probas).contiguous()                            # :27
    elif activation:
        probas = entropy_map(logits, "softmax", False, want_prob=True)[1]
    else:
        probas = logits
    return _OverlapFn.apply(probas, true, float(eps), reduce)


def jaccard_loss(true, logits, eps=1e-7, activation=True):
    """Reference signature and semantics (loss.py:5-37).  ``logits``: [B,C,H,W]; with ``activation=False`` (how
    train_mscmrseg.py:203 and train_mmwhs.py:218 call it) they already are probabilities, with ``activation=True``
    they go through a softmax over the channels first; ``true``: one-hot [B,C,H,W] (float or uint8).  Differentiable
    w.r.t. ``logits`` (through whatever produced them: the result is an ordinary autograd node on the HIP kernels).
    The train step itself uses the fused ``seg_loss`` above (one pass over the logits for both loss terms)."""
    return _overlap_loss(true, logits, eps, activation, None)


def dice_loss(true, logits, eps=1e-7, activation=True, reduce="class"):
    """Dice with ``jaccard_loss``'s signature and branches: ``logits`` [B,C,H,W] go through a softmax over the channels
    (``activation=True``) or already are probabilities; C == 1 pairs [sigmoid, 1 - sigmoid] with ``true`` broadcast over both
    channels, as ``jaccard_loss`` does; ``true``: one-hot [B,C,H,W] (float or uint8).  ``reduce="class"``:
    1 - mean_c 2 I_c / (S_c + eps) with the sums over (batch, pixels); ``"sample"``: mean_n (1 - 2 I_n / (S_n + eps)) with
    the sums over (classes, pixels).  This build's own rule (the reference never evaluates a Dice loss).  Differentiable
    w.r.t. ``logits``."""
    if reduce not in ("class", "sample"):
        raise ValueError("dice_loss: reduce %r is neither 'class' nor 'sample'" % (reduce,))
    return _overlap_loss(true, logits, eps, activation, reduce)


class _DiceLabelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, eps):
        logits = logits.contiguous()
        loss, ws, labels, bad = K.dice_labels_fwd(logits, labels, eps)
        ctx.logits, ctx.labels, ctx.ws = logits, labels, ws
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(bad)
        return loss, bad

    @staticmethod
    def backward(ctx, gout, gbad=None):
        if gout is None:
            return None, None, None
        return K.dice_labels_bwd(ctx.logits, ctx.labels, ctx.ws, gout.contiguous()), None, None


class DiceLoss(torch.nn.Module):
    """``kornia.losses.DiceLoss``'s surface (what both scripts build into ``dic_loss``): ``forward(input, target)`` with
    fp32 logits [B,C,H,W] and int64 or uint8 labels [B,H,W] -> mean_n (1 - 2 I_n / (S_n + eps)), I_n = sum p y,
    S_n = sum (p + y) over (classes, pixels), p = softmax(input) over the channels.  The softmax runs inside the kernel and
    no one-hot tensor is written.  This build's own rule: parity with any kornia version is unpinned and kornia's ``+ eps``
    on its one-hot tensor is not reproduced.  A label outside [0, C) belongs to no class and is counted on the device
    (``self.bad_labels`` after a call); ``check=True`` reads that counter (one synchronisation) and raises ValueError."""

    def __init__(self, eps: float = 1e-6, check: bool = False) -> None:
        super().__init__()
        self.eps, self.check, self.bad_labels = float(eps), bool(check), None

    def forward(self, input, target):       # noqa: A002 -- kornia's argument names
        if not torch.is_tensor(input) or not torch.is_tensor(target):
            raise TypeError("DiceLoss: input and target are tensors")
        if input.dim() != 4:
            raise ValueError("DiceLoss: input is [B,C,H,W], got %r" % (tuple(input.shape),))
        if target.dim() != 3:
            raise ValueError("DiceLoss: target is [B,H,W], got %r" % (tuple(target.shape),))
        if input.shape[0] != target.shape[0] or input.shape[-2:] != target.shape[-2:]:
            raise ValueError("DiceLoss: input %r and target %r differ in batch or spatial size"
                             % (tuple(input.shape), tuple(target.shape)))
        if input.device != target.device:
            raise ValueError("DiceLoss: input on %s, target on %s" % (input.device, target.device))
        loss, bad = _DiceLabelsFn.apply(input, target, self.eps)
        self.bad_labels = bad
        if self.check:
            nbad = int(bad.item())
            if nbad:
                raise ValueError("DiceLoss: %d labels outside [0, %d)" % (nbad, input.shape[1]))
        return loss


class _EntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, mode, norm, want_prob, want_mean):
        logits = logits.contiguous()
        ent, prob = K.entropy_fwd(logits, mode, norm, want_prob)
        ctx.logits, ctx.mode, ctx.norm = logits, mode, norm
        ctx.set_materialize_grads(False)
        outs = [ent]
        if want_prob:
            outs.append(prob)
        if want_mean:     # torch.mean(torch.sum(map, dim=1)): train_mmwhs.py:225,243
            outs.append(K.sum_all(ent, 1.0 / (logits.shape[0] * (logits.numel() // (logits.shape[0] * logits.shape[1])))))
        ctx.layout = (want_prob, want_mean)
        return outs[0] if len(outs) == 1 else tuple(outs)

    @staticmethod
    def backward(ctx, dent, *rest):
        want_prob, want_mean = ctx.layout
        rest = list(rest)
        dprob = rest.pop(0) if want_prob else None
        dmean = rest.pop(0) if want_mean else None
        if dent is None and dprob is None and dmean is None:
            return None, None, None, None, None
        d = K.entropy_bwd(ctx.logits, ctx.mode, ctx.norm, dent, dprob, dmean=dmean)
        return d, None, None, None, None


def entropy_map(logits, mode="sigmoid", normalise=False, want_prob=False, want_mean=False):
    """-> ent [, prob] [, mean]: ``mean`` = torch.mean(torch.sum(ent, dim=1)), the entropy loss term of the MM-WHS loop
    (train_mmwhs.py:225-230,243-247), differentiable like the map itself"""
    norm = 1.0 / math.log(logits.shape[1]) if normalise else 1.0
    return _EntropyFn.apply(logits, mode, norm, want_prob, want_mean)


class _EntropyTapFn(torch.autograd.Function):
    """(logits, entropy(logits)) with ONE gradient join: d_logits = d_tap + J^T d_ent is formed by the
    entropy kernel's accumulate store instead of a separate add (d1 sees the raw logits and d2 their
    entropy map in train_mscmrseg.py:222-241)."""

    @staticmethod
    def forward(ctx, logits, mode, norm):
        logits = logits.contiguous()
        ent, _ = K.entropy_fwd(logits, mode, norm, False)
        ctx.logits, ctx.mode, ctx.norm = logits, mode, norm
        ctx.set_materialize_grads(False)
        return logits.view_as(logits), ent

    @staticmethod
    def backward(ctx, dtap, dent):
        if dent is None:
            return dtap, None, None
        if dtap is None:
            return K.entropy_bwd(ctx.logits, ctx.mode, ctx.norm, dent, None), None, None
        dtap = dtap.contiguous()
        K.entropy_bwd(ctx.logits, ctx.mode, ctx.norm, dent, None, out=dtap, accumulate=True)
        return dtap, None, None


def logits_and_entropy(logits, mode="sigmoid", normalise=False):
    norm = 1.0 / math.log(logits.shape[1]) if normalise else 1.0
    return _EntropyTapFn.apply(logits, mode, norm)


class _BceConstFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, label, weight, want_acc):
        x = x.contiguous()
        loss, acc = K.bce_const_fwd(x, label, want_acc)
        ctx.x, ctx.label, ctx.weight = x, label, weight
        ctx.set_materialize_grads(False)
        if want_acc:
            ctx.mark_non_differentiable(acc)
            return loss, acc
        return loss

    @staticmethod
    def backward(ctx, gout, gacc=None):
        if gout is None:
            return None, None, None, None
        return K.bce_const_bwd(ctx.x, ctx.label, gout.contiguous(), ctx.weight), None, None, None


def bce_logits_const(d_out, label, weight=1.0, want_acc=False):
    """mean BCE-with-logits of ``d_out`` against the constant ``label``.  The returned scalar is the
    UNWEIGHTED loss; ``weight`` (the reference's ``args.dr``) scales its gradient, i.e. backpropagating
    the returned value with grad 1 equals backpropagating ``weight * loss``."""
    return _BceConstFn.apply(d_out, float(label), float(weight), want_acc)


class _NNLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        x, y = x.contiguous(), y.contiguous()
        loss, idx, val = K.nn_loss_fwd(x, y)
        ctx.x, ctx.y, ctx.idx, ctx.val = x, y, idx, val
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, gout):
        if gout is None:
            return None, None
        return K.nn_loss_bwd(ctx.x, ctx.y, ctx.idx, ctx.val, gout.contiguous()), None


def batch_NN_loss(x, y):
    """loss.py:40-76: symmetric nearest-neighbour (Chamfer, L2 root) distance between [B,N,3] clouds.
    Differentiable w.r.t. ``x`` (the predicted vertices); ``y`` is data."""
    return _NNLossFn.apply(x, y)
