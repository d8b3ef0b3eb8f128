"""Plain float64 statements of the memory-bound operations (BatchNorm, pooling, dense, optimisers, losses) and of the k = 1
Conv1d, written from the formulas: what the *_edges_gpu tests compare the HIP kernels with.  Inputs are the kernels'
float32 tensors (and the float32 values of their scalar arguments) cast up; nothing here calls a kernel.
tests/test_fp64_refs.py checks every function against torch autograd / torch.optim in float64 on the CPU."""
import math

import numpy as np
import torch

SMOOTHF = 1e-7          # losses.hip


def up(t):
    """float64 host copy of a tensor / array (None stays None)"""
    if t is None:
        return None
    return t.detach().double().cpu() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t), dtype=torch.float64)


def f32(v):
    """the float32 value of a scalar argument (what the C ABI receives), as a Python float"""
    return float(np.float32(v))


def _pc(v, ndim):
    return v.view((1, -1) + (1,) * (ndim - 2))


def _red(ndim):
    return (0,) + tuple(range(2, ndim))


# ------------------------------------------------------------------------------------------ BatchNorm
def bn_stats(a):
    """(mean, biased var, count) per channel of [N,C,...]"""
    a = up(a)
    dims = _red(a.dim())
    mean = a.mean(dims)
    var = ((a - _pc(mean, a.dim())) ** 2).mean(dims)
    return mean, var, a.numel() // a.shape[1]


def bn_train_forward(a, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1, relu=False):
    """y = (a - mean) / sqrt(var + eps) * gamma + beta with the batch statistics; running statistics updated with the
    UNBIASED variance (count == 1, where that is undefined: var = 0 and unbiased = var, as the kernel defines it)"""
    a, gamma, beta = up(a), up(gamma), up(beta)
    eps, momentum = f32(eps), f32(momentum)
    mean, var, count = bn_stats(a)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    y = a * _pc(scale, a.dim()) + _pc(shift, a.dim())
    if relu:
        y = torch.where(y > 0, y, torch.zeros_like(y))
    unb = var * count / (count - 1.0) if count > 1 else var
    rm = (1.0 - momentum) * up(running_mean) + momentum * mean
    rv = (1.0 - momentum) * up(running_var) + momentum * unb
    return dict(y=y, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv,
                count=count)


def bn_backward(a, dy, gamma, mean, invstd, beta=None, post_relu=False, slope=1.0, frozen=False):
    """Backward of [z -> a = lrelu(z, slope) -> BN(a)] (gradient w.r.t. z, written on a: a > 0 <=> z > 0) or of
    [a -> BN -> relu] (post_relu; gradient w.r.t. a).  ``mean`` / ``invstd``: the batch statistics, or with ``frozen`` the
    running ones: the layer is then a fixed affine, da = gamma * invstd * g.  Returns (dz, dgamma, dbeta)."""
    a, dy, gamma, mean, invstd = up(a), up(dy), up(gamma), up(mean), up(invstd)
    nd = a.dim()
    xhat = (a - _pc(mean, nd)) * _pc(invstd, nd)
    g = dy
    if post_relu:
        y = xhat * _pc(gamma, nd) + _pc(up(beta), nd)
        g = torch.where(y > 0, dy, torch.zeros_like(dy))
    dbeta = g.sum(_red(nd))
    dgamma = (g * xhat).sum(_red(nd))
    sc = _pc(gamma * invstd, nd)
    if frozen:
        da = sc * g
    else:
        cnt = a.numel() // a.shape[1]
        da = sc * (g - _pc(dbeta, nd) / cnt - xhat * _pc(dgamma, nd) / cnt)
    if not post_relu:
        da = da * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, f32(slope)))
    return da, dgamma, dbeta


def clear_gates(a, gate, lo=1e-3, to=1e-2, rounds=30):
    """Move every element of the float32 tensor ``a`` whose float64 gate value is within ``lo`` of zero to a gate value of
    +-``to`` (its own side), so that a float32 kernel and the float64 reference decide every sign alike and no element has
    to be masked out.  ``gate(a64) -> (value, d value / d a)``; repeated, because the gate of a BatchNorm depends on the
    batch statistics of ``a`` itself."""
    a = a.clone().float()
    for _ in range(rounds):
        a64 = a.double()
        y, dyda = gate(a64)
        bad = y.abs() < lo
        if not bool(bad.any()):
            return a
        target = torch.where(y >= 0, torch.full_like(y, to), torch.full_like(y, -to))
        a64 = torch.where(bad, a64 + (target - y) / dyda, a64)
        a = a64.float()
    raise AssertionError("clear_gates did not converge")


def gate_identity(a64):
    return a64, torch.ones_like(a64)


def gate_bn(gamma, beta, eps=1e-5):
    """the gate of [BN -> relu] with batch statistics"""
    def gate(a64):
        r = bn_train_forward(a64, gamma, beta, torch.zeros_like(up(gamma)), torch.ones_like(up(gamma)), eps)
        return r["y"], _pc(r["scale"], a64.dim()).expand_as(a64)
    return gate


def gate_affine(scale, shift):
    def gate(a64):
        sc = _pc(up(scale), a64.dim())
        return a64 * sc + _pc(up(shift), a64.dim()), sc.expand_as(a64)
    return gate


def channel_sum(x):
    x = up(x)
    return x.sum(_red(x.dim()))


# ------------------------------------------------------------------------------------------ pooling
def maxpool2(x, scale=None, shift=None):
    """2x2 max-pool of x * scale + shift (per channel): values and the window position 2*dy + dx of the FIRST maximum in
    row-major window order"""
    x = up(x)
    if scale is not None:
        x = x * _pc(up(scale), 4) + _pc(up(shift), 4)
    win = torch.stack([x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]], 0)
    best, idx = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.uint8)
    for k in range(1, 4):
        take = win[k] > best
        best = torch.where(take, win[k], best)
        idx = torch.where(take, torch.full_like(idx, k), idx)
    return best, idx


def maxpool2_scatter(g, idx, h, w):
    """backward of the 2x2 max-pool: g lands on position idx of its window, the other three get 0"""
    g, idx = up(g), idx.cpu()
    out = torch.zeros(g.shape[:2] + (h, w), dtype=torch.float64)
    for k in range(4):
        out[:, :, (k >> 1)::2, (k & 1)::2] = torch.where(idx == k, g, torch.zeros_like(g))
    return out


def fold2(dy):
    """backward of nearest x2 upsampling: the sum over each 2x2 block"""
    dy = up(dy)
    return dy[:, :, 0::2, 0::2] + dy[:, :, 0::2, 1::2] + dy[:, :, 1::2, 0::2] + dy[:, :, 1::2, 1::2]


# ------------------------------------------------------------------------------------------ dense
def linear(x, w, b=None):
    y = up(x) @ up(w).t()
    return y if b is None else y + up(b)


def linear_backward(dy, x, w):
    """(dx, dw, db) of y = x w^T + b"""
    dy, x, w = up(dy), up(x), up(w)
    return dy @ w, dy.t() @ x, dy.sum(0)


def bmm(a, b, ta=False, tb=False):
    a, b = up(a), up(b)
    return torch.matmul(a.transpose(1, 2) if ta else a, b.transpose(1, 2) if tb else b)


def conv1d_k1(x, w, b=None):
    """torch.nn.Conv1d(cin, cout, 1) on [B,cin,L]: (y, sum of y, sum of y^2), the sums per output channel over batch and
    points (what the BatchNorm partials of the kernel's epilogue add up to)"""
    y = torch.matmul(up(w), up(x))                                 # [cout,cin] x [B,cin,L] -> [B,cout,L]
    if b is not None:
        y = y + up(b)[None, :, None]
    return y, y.sum((0, 2)), (y * y).sum((0, 2))


def conv1d_k1_backward(dy, x, w):
    """(dx, dw, db) of y[b,o,l] = sum_c w[o,c] x[b,c,l] + bias[o]"""
    dy, x, w = up(dy), up(x), up(w)
    flat = lambda t: t.transpose(0, 1).reshape(t.shape[1], -1)    # [B,C,L] -> [C, B*L]
    return torch.matmul(w.t(), dy), flat(dy) @ flat(x).t(), dy.sum((0, 2))


def max_points(x):
    """max over the last axis of [B,C,L]; index of the first maximum"""
    x = up(x)
    v = x.max(dim=2)[0]
    first = (x == v[..., None]).to(torch.uint8).argmax(dim=2)
    return v, first


# ------------------------------------------------------------------------------------------ optimisers
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """torch.optim.Adam's single-tensor step (no amsgrad, L2 weight decay) -> (p, m, v)"""
    p, g, m, v = up(p), up(g), up(m), up(v)
    lr, beta1, beta2, eps, weight_decay, grad_scale = (f32(t) for t in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    g = g * grad_scale
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def sgd_step(p, g, buf, lr, momentum, weight_decay, first_step, grad_scale=1.0):
    """torch.optim.SGD's single-tensor step (dampening 0, no nesterov) -> (p, buf)"""
    p, g = up(p), up(g)
    lr, momentum, weight_decay, grad_scale = (f32(t) for t in (lr, momentum, weight_decay, grad_scale))
    g = g * grad_scale + weight_decay * p
    if momentum != 0:
        buf = g.clone() if first_step else momentum * up(buf) + g
        g = buf
    return p - lr * g, buf


# ------------------------------------------------------------------------------------------ losses
def seg_loss(logits, onehot, mode, w_main=1.0, w_jac=1.0):
    """(main, jaccard, d(w_main * main + w_jac * jaccard) / d logits): BCE-with-clamp + Jaccard on sigmoid probabilities,
    or the double-softmax cross entropy + Jaccard on softmax probabilities -- oracle/losses.py evaluated in float64"""
    from oracle import losses as OL
    l = up(logits).requires_grad_(True)
    fn = OL.seg_loss_sigmoid if mode == "sigmoid" else OL.seg_loss_softmax
    main, jac = fn(l, onehot.cpu())
    (w_main * main + w_jac * jac).backward()
    return main.detach(), jac.detach(), l.grad


def jaccard(truth, probs, eps=1e-7, gout=1.0):
    """(loss, gout * d loss / d probs) of oracle.losses.jaccard_loss in float64"""
    from oracle import losses as OL
    p = up(probs).requires_grad_(True)
    loss = OL.jaccard_loss(up(truth), p, f32(eps))
    (loss * gout).backward()
    return loss.detach(), p.grad


def bce_const(x, label, gout=1.0, gscale=1.0):
    """mean over elements of max(x, 0) - x * label + log(1 + exp(-|x|)) -> (loss, gradient * gout * gscale, accuracy)"""
    x = up(x).requires_grad_(True)
    loss = (x.clamp(min=0) - x * float(label) + torch.log1p(torch.exp(-x.abs()))).mean()
    (loss * gout * f32(gscale)).backward()
    acc = (x.detach() >= 0).double().mean()          # sigmoid(x) >= 0.5
    return loss.detach(), x.grad, acc


def entropy(logits, mode, norm=1.0):
    """(-p * log(p + SMOOTHF) * norm, p) per channel; p = sigmoid or softmax over channels"""
    l = logits if torch.is_tensor(logits) and logits.dtype == torch.float64 else up(logits)     # (float64: kept in its graph)
    p = torch.sigmoid(l) if mode == "sigmoid" else torch.softmax(l, 1)
    return -1.0 * p * torch.log(p + SMOOTHF) * f32(norm), p


def entropy_backward(logits, mode, norm=1.0, dent=None, dprob=None, dmean=None):
    """gradient w.r.t. the logits of sum(ent * dent) + sum(p * dprob) + dmean * mean_{n,pixels} sum_c ent"""
    l = up(logits).requires_grad_(True)
    ent, p = entropy(l, mode, norm)
    tot = torch.zeros((), dtype=torch.float64)
    if dent is not None:
        tot = tot + (ent * up(dent)).sum()
    if dprob is not None:
        tot = tot + (p * up(dprob)).sum()
    if dmean is not None:
        tot = tot + float(up(dmean)) * ent.sum() / (l.numel() // l.shape[1])
    tot.backward()
    return l.grad
