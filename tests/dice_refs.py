"""Float64 statements of the Dice losses (csrc/dice_loss.hip, utils/loss.py), written from the definition:

  per class   I_c = sum p y, S_c = sum (p + y) over dims (0, 2, 3): loss = 1 - mean_c( 2 I_c / (S_c + eps) )
  per sample  I_n, S_n over dims (1, 2, 3):                         loss = mean_n( 1 - 2 I_n / (S_n + eps) )
  d loss / d p = -(2 / M) ( y / (S + eps) - I / (S + eps)^2 ), the sums of the element's own class or sample, M = C or N

twice and independently: ``dice_autograd`` (torch autograd over the definition) and ``dice_closed_form`` (the gradient
formula and the activation's Jacobian in plain numpy).  scripts/make_dice_golden.py writes tests/golden/dice_loss.npz from
the two; tests/test_dice_loss.py holds both to it; tests/test_dice_loss_gpu.py compares the kernels with the functions
below.  The main terms (BCE, double-softmax cross entropy) come from oracle/losses.py.  Nothing here calls a kernel."""
import numpy as np
import torch

from fp64_refs import f32, up


def _dims(ndim, reduce):
    if reduce not in ("class", "sample"):
        raise ValueError(reduce)
    return ((0,) if reduce == "class" else (1,)) + tuple(range(2, ndim))


def activate(l, mode):
    """probabilities of float64 logits: 'sigmoid', 'softmax' over the channels, or None (they are probabilities)"""
    if mode is None:
        return l
    return torch.sigmoid(l) if mode == "sigmoid" else torch.softmax(l, 1)


def dice_value(p, y, eps, reduce):
    """the definition on float64 torch tensors (differentiable)"""
    dims = _dims(p.dim(), reduce)
    inter = torch.sum(p * y, dims)
    card = torch.sum(p + y, dims)
    ratio = 2.0 * inter / (card + eps)
    return 1.0 - ratio.mean() if reduce == "class" else (1.0 - ratio).mean()


def dice_autograd(logits, truth, mode, reduce, eps):
    """(loss, d loss / d logits) by torch autograd; ``mode`` None: ``logits`` are the probabilities"""
    l = up(logits).requires_grad_(True)
    loss = dice_value(activate(l, mode), up(truth), eps, reduce)
    loss.backward()
    return loss.detach(), l.grad


def dice_closed_form(logits, truth, mode, reduce, eps):
    """(loss, d loss / d logits) as numpy float64 arrays from the closed-form gradient and the activation's Jacobian"""
    l = np.asarray(up(logits).numpy(), dtype=np.float64)
    y = np.asarray(up(truth).numpy(), dtype=np.float64)
    if mode is None:
        p = l
    elif mode == "sigmoid":
        p = 1.0 / (1.0 + np.exp(-l))
    else:
        e = np.exp(l - l.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    dims = _dims(l.ndim, reduce)
    inter = (p * y).sum(axis=dims, keepdims=True)
    den = (p + y).sum(axis=dims, keepdims=True) + eps
    m = l.shape[1] if reduce == "class" else l.shape[0]
    loss = 1.0 - (2.0 * inter / den).sum() / m
    gp = -(2.0 / m) * (y / den - inter / den ** 2)
    if mode is None:
        g = gp
    elif mode == "sigmoid":
        g = gp * p * (1.0 - p)
    else:
        g = p * (gp - (gp * p).sum(axis=1, keepdims=True))
    return np.float64(loss), g


def seg_loss_dice(logits, onehot, mode, reduce, eps, w_main=1.0, w_ov=1.0):
    """the fused form: (main, dice, d(w_main * main + w_ov * dice) / d logits); main = BCE with the clamp ('sigmoid') or
    the double-softmax cross entropy ('softmax') of oracle/losses.py"""
    from oracle import losses as OL
    l = up(logits).requires_grad_(True)
    fn = OL.seg_loss_sigmoid if mode == "sigmoid" else OL.seg_loss_softmax
    main = fn(l, onehot.cpu())[0]
    dice = dice_value(activate(l, mode), up(onehot), eps, reduce)
    (w_main * main + w_ov * dice).backward()
    return main.detach(), dice.detach(), l.grad


def dice_probs(truth, probs, eps, reduce, gout=1.0):
    """Dice on given probabilities: (loss, gout * d loss / d probs); eps as the float32 the C ABI receives"""
    p = up(probs).requires_grad_(True)
    loss = dice_value(p, up(truth), f32(eps), reduce)
    (loss * gout).backward()
    return loss.detach(), p.grad


def dice_signature(true, logits, eps, activation, reduce):
    """``dice_loss(true, logits, eps, activation, reduce)`` with ``jaccard_loss``'s branches: C == 1 pairs
    [sigmoid, 1 - sigmoid] with ``true`` broadcast over both channels -> (loss, d loss / d logits)"""
    l = up(logits).requires_grad_(True)
    t = up(true)
    if l.shape[1] == 1:
        pos = torch.sigmoid(l)
        p = torch.cat([pos, 1 - pos], dim=1)
        t = t.expand_as(p)
    else:
        p = torch.softmax(l, 1) if activation else l
    loss = dice_value(p, t, f32(eps), reduce)
    loss.backward()
    return loss.detach(), l.grad


def dice_labels(logits, labels, eps, gout=1.0):
    """``DiceLoss``: softmax over the channels, per sample, one-hot of the label map; a label outside [0, C) belongs to no
    class (an all-zero one-hot row) -> (loss, gout * d loss / d logits, number of such labels)"""
    l = up(logits).requires_grad_(True)
    lab = labels.detach().cpu().long()
    c = l.shape[1]
    valid = (lab >= 0) & (lab < c)
    y = torch.nn.functional.one_hot(torch.where(valid, lab, torch.zeros_like(lab)), c).double() * valid[..., None].double()
    y = y.movedim(-1, 1)
    loss = dice_value(torch.softmax(l, 1), y, f32(eps), "sample")
    (loss * gout).backward()
    return loss.detach(), l.grad, int((~valid).sum())
