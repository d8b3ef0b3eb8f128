"""The hand-written float64 references of tests/fp64_refs.py against torch autograd / torch.optim in float64 (CPU only):
a machine without a device can check what the *_edges_gpu tests measure the kernels with.  Bound: 1e-12."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp64_refs as R
from conftest import rel_err

TOL = 1e-12


def _r(rng, *shape):
    return torch.from_numpy(rng.normal(0, 1, shape).astype(np.float32))


@pytest.mark.parametrize("shape", [(3, 4, 5, 6), (2, 3, 7), (5, 2)])
@pytest.mark.parametrize("post_relu", [False, True])
def test_batchnorm_forward_backward(shape, post_relu):
    rng = np.random.default_rng(1)
    c, slope = shape[1], 0.2
    z, dy = _r(rng, *shape), _r(rng, *shape)
    gamma, beta, rm0, rv0 = _r(rng, c) * 0.2 + 1, _r(rng, c) * 0.2, _r(rng, c) * 0.1, torch.rand(c) + 0.5
    zr = z.double().requires_grad_(True)
    g_r, b_r = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = rm0.double(), rv0.double()
    a_ref = zr if post_relu else F.leaky_relu(zr, R.f32(slope))
    y_ref = F.batch_norm(a_ref, rm, rv, g_r, b_r, True, R.f32(0.1), R.f32(1e-5))
    if post_relu:
        y_ref = F.relu(y_ref)
    y_ref.backward(dy.double())
    a = a_ref.detach()
    f = R.bn_train_forward(a, gamma, beta, rm0, rv0, relu=post_relu)
    assert rel_err(f["y"], y_ref) < TOL
    assert rel_err(f["running_mean"], rm) < TOL and rel_err(f["running_var"], rv) < TOL
    dz, dg, db = R.bn_backward(a, dy, gamma, f["mean"], f["invstd"], beta, post_relu, slope)
    assert rel_err(dz, zr.grad) < TOL and rel_err(dg, g_r.grad) < TOL and rel_err(db, b_r.grad) < TOL


def test_batchnorm_count_one_is_defined_as_the_kernel_defines_it():
    f = R.bn_train_forward(torch.tensor([[[3.0]]]), torch.tensor([2.0]), torch.tensor([0.5]), torch.tensor([1.0]),
                           torch.tensor([4.0]))
    assert float(f["var"]) == 0.0 and float(f["y"]) == 0.5
    assert abs(float(f["running_var"]) - (1.0 - R.f32(0.1)) * 4.0) < TOL          # unbiased = var = 0
    assert abs(float(f["running_mean"]) - ((1.0 - R.f32(0.1)) * 1.0 + R.f32(0.1) * 3.0)) < TOL


@pytest.mark.parametrize("shape", [(2, 3, 4, 6), (3, 2, 5)])
@pytest.mark.parametrize("post_relu", [False, True])
def test_frozen_batchnorm_backward(shape, post_relu):
    rng = np.random.default_rng(2)
    c, slope = shape[1], 0.2
    z, dy = _r(rng, *shape), _r(rng, *shape)
    gamma, beta, rm, rv = _r(rng, c) * 0.2 + 1, _r(rng, c) * 0.2, _r(rng, c) * 0.1, torch.rand(c) + 0.5
    zr = z.double().requires_grad_(True)
    g_r, b_r = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a_ref = zr if post_relu else F.leaky_relu(zr, R.f32(slope))
    y_ref = F.batch_norm(a_ref, rm.double(), rv.double(), g_r, b_r, False, 0.1, R.f32(1e-5))
    if post_relu:
        y_ref = F.relu(y_ref)
    y_ref.backward(dy.double())
    invstd = 1.0 / torch.sqrt(rv.double() + R.f32(1e-5))
    dz, dg, db = R.bn_backward(a_ref.detach(), dy, gamma, rm, invstd, beta, post_relu, slope, frozen=True)
    assert rel_err(dz, zr.grad) < TOL and rel_err(dg, g_r.grad) < TOL and rel_err(db, b_r.grad) < TOL


def test_clear_gates_moves_only_what_is_near_zero():
    rng = np.random.default_rng(3)
    a = _r(rng, 4, 3, 50)
    a[0, 0, :3] = torch.tensor([0.0, 5e-4, -5e-4])
    b = R.clear_gates(a, R.gate_identity)
    assert float(b.abs().min()) >= 1e-3 and torch.equal(b[a.abs() >= 1e-3], a[a.abs() >= 1e-3])
    assert b[0, 0, :3].tolist() == [R.f32(1e-2), R.f32(1e-2), R.f32(-1e-2)]
    gamma, beta = _r(rng, 3) * 0.2 + 1, _r(rng, 3) * 0.2
    b = R.clear_gates(a, R.gate_bn(gamma, beta))
    y = R.bn_train_forward(b, gamma, beta, torch.zeros(3), torch.ones(3))["y"]
    assert float(y.abs().min()) >= 1e-3


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (2, 3, 6, 4), (3, 2, 10, 14)])
def test_maxpool_and_fold(shape):
    rng = np.random.default_rng(4)
    x = _r(rng, *shape)
    x[0, 0, :2, :2] = 1.5                                          # a tie: the first window position wins
    xr = x.double().requires_grad_(True)
    y_ref, i_ref = F.max_pool2d(xr, 2, return_indices=True)
    g = _r(rng, *y_ref.shape)
    y_ref.backward(g.double())
    y, idx = R.maxpool2(x)
    assert torch.equal(y, y_ref.detach()) and int(idx[0, 0, 0, 0]) == 0
    h, w = shape[2], shape[3]
    flat = (2 * torch.arange(h // 2)[:, None] + idx.long() // 2) * w + 2 * torch.arange(w // 2)[None, :] + idx.long() % 2
    assert torch.equal(flat, i_ref)
    assert torch.equal(R.maxpool2_scatter(g, idx, h, w), xr.grad)
    sc, sf = torch.tensor([-2.0, 0.5, 1.0][:shape[1]]), torch.tensor([0.25, -0.5, 0.0][:shape[1]])
    y2, _ = R.maxpool2(x, sc, sf)
    assert torch.equal(y2, F.max_pool2d(x.double() * sc.double()[None, :, None, None] + sf.double()[None, :, None, None], 2))
    u = _r(rng, *shape).double().requires_grad_(True)
    up = F.interpolate(u, scale_factor=2, mode="nearest")
    gu = _r(rng, *up.shape)
    up.backward(gu.double())
    assert rel_err(R.fold2(gu), u.grad) < TOL


@pytest.mark.parametrize("m,k,n", [(1, 1, 1), (7, 13, 5), (40, 9, 3)])
def test_linear_bmm_max_points(m, k, n):
    rng = np.random.default_rng(5)
    x, w, b, g = _r(rng, m, k), _r(rng, n, k), _r(rng, n), _r(rng, m, n)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    y_ref = F.linear(xr, wr, br)
    y_ref.backward(g.double())
    assert rel_err(R.linear(x, w, b), y_ref) < TOL
    dx, dw, db = R.linear_backward(g, x, w)
    assert rel_err(dx, xr.grad) < TOL and rel_err(dw, wr.grad) < TOL and rel_err(db, br.grad) < TOL
    for ta in (False, True):
        for tb in (False, True):
            a3, b3 = _r(rng, 3, *((k, m) if ta else (m, k))), _r(rng, 3, *((n, k) if tb else (k, n)))
            ref = torch.bmm(a3.double().transpose(1, 2) if ta else a3.double(), b3.double().transpose(1, 2) if tb else b3.double())
            assert rel_err(R.bmm(a3, b3, ta, tb), ref) < TOL
    h = _r(rng, 2, 3, 70)
    h[0, 0, 7] = h[0, 0, 69] = 9.0
    v, i = R.max_points(h)
    assert torch.equal(v, h.double().max(2)[0]) and int(i[0, 0]) == 7
    assert torch.equal(h.double().gather(2, i[..., None])[..., 0], v)


@pytest.mark.parametrize("b,cin,cout,l", [(1, 1, 1, 1), (3, 5, 7, 11), (2, 33, 4, 65)])
@pytest.mark.parametrize("bias", [False, True])
def test_conv1d_k1(b, cin, cout, l, bias):
    rng = np.random.default_rng(8)
    x, w, bv, g = _r(rng, b, cin, l), _r(rng, cout, cin), (_r(rng, cout) if bias else None), _r(rng, b, cout, l)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = bv.double().requires_grad_(True) if bias else None
    y_ref = F.conv1d(xr, wr[:, :, None], br)
    y_ref.backward(g.double())
    y, s1, s2 = R.conv1d_k1(x, w, bv)
    assert y.shape == (b, cout, l) and rel_err(y, y_ref) < TOL
    yd = y_ref.detach()
    assert rel_err(s1, yd.sum((0, 2))) < TOL and rel_err(s2, (yd ** 2).sum((0, 2))) < TOL
    # the same sums as BatchNorm1d's batch statistics see them: mean = s1 / n, biased variance = s2 / n - mean^2
    n = b * l
    assert rel_err(s1 / n, yd.mean((0, 2))) < TOL
    assert float((s2 / n - (s1 / n) ** 2 - yd.var((0, 2), unbiased=False)).abs().max()) < TOL * max(1.0, float(s2.max() / n))
    dx, dw, db = R.conv1d_k1_backward(g, x, w)
    assert rel_err(dx, xr.grad) < TOL and rel_err(dw, wr.grad) < TOL
    if bias:
        assert rel_err(db, br.grad) < TOL
    else:
        assert rel_err(db, g.double().sum((0, 2))) < TOL


@pytest.mark.parametrize("numel", [1, 257])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_optimisers(numel, wd):
    rng = np.random.default_rng(6)
    p0 = _r(rng, numel)
    grads = [_r(rng, numel) for _ in range(3)]
    hp = dict(lr=R.f32(1e-3), b1=R.f32(0.9), b2=R.f32(0.99), eps=R.f32(1e-8), wd=R.f32(wd))
    pr = p0.double().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = p0, torch.zeros(numel), torch.zeros(numel)
    for i, g in enumerate(grads):
        pr.grad = g.double()
        opt.step()
        p, m, v = R.adam_step(p, g, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], i + 1)
        assert rel_err(p, pr.detach()) < TOL
    p1, _, _ = R.adam_step(p0, grads[0] * 4, torch.zeros(numel), torch.zeros(numel), 1e-3, 0.9, 0.99, 1e-8, wd, 1, grad_scale=0.25)
    p2, _, _ = R.adam_step(p0, grads[0], torch.zeros(numel), torch.zeros(numel), 1e-3, 0.9, 0.99, 1e-8, wd, 1)
    assert rel_err(p1, p2) < TOL
    for mom in (0.0, 0.99):
        pr = p0.double().requires_grad_(True)
        opt = torch.optim.SGD([pr], lr=R.f32(2.5e-2), momentum=R.f32(mom), weight_decay=hp["wd"])
        p, buf = p0, None
        for i, g in enumerate(grads):
            pr.grad = g.double()
            opt.step()
            p, buf = R.sgd_step(p, g, buf, 2.5e-2, mom, wd, i == 0)
            assert rel_err(p, pr.detach()) < TOL
        assert (buf is None) == (mom == 0.0)


@pytest.mark.parametrize("c", [1, 3])
def test_losses(c):
    rng = np.random.default_rng(7)
    logits = _r(rng, 2, c, 5, 7) * 2
    logits[0, 0, 0, :2] = torch.tensor([40.0, -40.0])
    # BCE with torch's log clamp at -100, Jaccard, double-softmax CE: the oracle's statements, evaluated in float64
    lab = rng.integers(0, c, (2, 5, 7))
    onehot = torch.from_numpy(np.moveaxis(np.eye(c, dtype=np.uint8)[lab], -1, 1).copy())
    l = logits.double()
    p = torch.sigmoid(l)
    y = onehot.double()
    bce = -(y * torch.log(p).clamp(min=-100) + (1 - y) * torch.log(1 - p).clamp(min=-100)).mean()
    inter, card = (p * y).sum((0, 2, 3)), (p + y).sum((0, 2, 3))
    jac = 1 - (inter / (card - inter + 1e-7)).mean()
    main, j, grad = R.seg_loss(logits, onehot, "sigmoid", 1.0, 0.7)
    assert abs(float(main - bce)) < TOL * max(1, float(bce)) and abs(float(j - jac)) < TOL
    assert grad.shape == logits.shape and bool(torch.isfinite(grad).all())
    sm = torch.softmax(l, 1)
    ce = -torch.log_softmax(sm, 1).gather(1, torch.from_numpy(lab)[:, None]).mean()
    main, j, _ = R.seg_loss(logits, onehot, "softmax")
    assert abs(float(main - ce)) < TOL * max(1, float(ce))
    jl, jg = R.jaccard(onehot, sm.float(), 1e-7, gout=0.5)
    pr = sm.float().double().requires_grad_(True)
    inter, card = (pr * y).sum((0, 2, 3)), (pr + y).sum((0, 2, 3))
    (0.5 * (1 - (inter / (card - inter + R.f32(1e-7))).mean())).backward()
    assert rel_err(jg, pr.grad) < TOL
    # BCE-with-logits against a constant, against torch's own
    for label in (0.0, 1.0):
        xr = l.clone().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(xr, torch.full_like(xr, label))
        (ref * 0.5).backward()
        loss, g, acc = R.bce_const(logits, label, gout=1.0, gscale=0.5)
        assert abs(float(loss - ref.detach())) < TOL and rel_err(g, xr.grad) < TOL
        assert float(acc) == float((torch.sigmoid(l) >= 0.5).double().mean())
    # entropy maps and their gradient
    for mode in ("sigmoid", "softmax"):
        norm = 1.0 / math.log(max(c, 2))
        lr_ = l.clone().requires_grad_(True)
        pp = torch.sigmoid(lr_) if mode == "sigmoid" else F.softmax(lr_, 1)
        e_ref = -pp * torch.log(pp + 1e-7) * R.f32(norm)
        w1, w2, dm = _r(rng, *logits.shape), _r(rng, *logits.shape), torch.tensor(0.3)
        ((e_ref * w1.double()).sum() + (pp * w2.double()).sum() + float(dm.double()) * e_ref.sum(1).mean()).backward()
        e, q = R.entropy(logits, mode, norm)
        assert rel_err(e, e_ref) < TOL and rel_err(q, pp) < TOL
        assert rel_err(R.entropy_backward(logits, mode, norm, w1, w2, dm), lr_.grad) < TOL
